// Path-tracing variants of the fused kernel (rtg_mega_impl.hpp) specialised on the scene's
// shading and traversal features, as k_shade and the path tracer's step kernel are: BRDF
// shading with point / area / directional lights (+ env / spot / mesh lights), meshes and
// spheres (small or large leaves).  Scenes with textures, maps, instances or transforms take
// the general instantiation (rtg_mega.hip; the rule: rtg_variants.hpp mega_variant).  Same
// code, same results: the feature bits only drop code the scene cannot reach.

// the fused kernels keep trav_ray's ray unlaundered (rtg_walk.hpp: laundering it costs C2
// 6 %, profiles/r05ag_sphere_launder_ab.txt)
#define RTG_XFORM_LAUNDER 0
#include "rtg_kernels.hpp"
#include "rtg_mega_impl.hpp"

namespace rtg {

hipError_t launch_mega_pt(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P,
                          float* hdr, unsigned char* l, float* accum, DevCounters* cnt, hipStream_t stream) {
    return launch_special<true>(v, S, C, P, hdr, l, accum, cnt, stream);
}

}  // namespace rtg
