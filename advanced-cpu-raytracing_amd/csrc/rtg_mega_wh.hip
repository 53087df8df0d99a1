// Ray-tree (Whitted) variants of the fused kernel (rtg_mega_impl.hpp) specialised on the
// scene's shading and traversal features, as rtg_mega_pt.hip's path-tracing ones: C2-like
// scenes (BRDF shading, point / area / directional lights, meshes and spheres) below the
// ray-tree pipeline's frame size.  Same code, same results.

// the fused kernels keep trav_ray's ray unlaundered (rtg_walk.hpp: laundering it costs C2
// 6 %, profiles/r05ag_sphere_launder_ab.txt)
#define RTG_XFORM_LAUNDER 0
#include "rtg_kernels.hpp"
#include "rtg_mega_impl.hpp"

namespace rtg {

hipError_t launch_mega_wh(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P,
                          float* hdr, unsigned char* l, float* accum, DevCounters* cnt, hipStream_t stream) {
    return launch_special<false>(v, S, C, P, hdr, l, accum, cnt, stream);
}

}  // namespace rtg
