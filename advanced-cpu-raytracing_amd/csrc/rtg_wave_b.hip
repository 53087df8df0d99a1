// Wavefront pipeline, traversal variants with large leaves (cooperative leaf tests) (rtg_wave.hpp).
#include "rtg_wave.hpp"

namespace rtg {

RTG_TRAV_FEATS_BIG(RTG_WAVE_INST)

}  // namespace rtg
