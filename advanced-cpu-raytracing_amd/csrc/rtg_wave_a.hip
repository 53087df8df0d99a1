// Wavefront pipeline, traversal variants without large leaves (meshes / + spheres / everything) (rtg_wave.hpp).
#include "rtg_wave.hpp"

namespace rtg {

RTG_TRAV_FEATS_SMALL(RTG_WAVE_INST)

}  // namespace rtg
