// Fused ("mega") render kernel: one thread per pixel walks the pixel's whole ray tree
// -- PerformShading (raytracer.cpp:65-134) with the recursion of ComputeMirrorReflection /
// ...Dielectric... / ...Conductor... and, for path-tracing cameras, ComputeGlobalIllumination
// (raytracer.cpp:135-191) unrolled onto an explicit per-thread stack.  Used for path
// tracing, motion blur and small ray-tree frames; other scenes take the wavefront
// pipelines (rtg_wave.hip, rtg_tree.hip).
// the fused kernels keep trav_ray's ray unlaundered (rtg_walk.hpp: laundering it costs C2
// 6 %, profiles/r05ag_sphere_launder_ab.txt)
#define RTG_XFORM_LAUNDER 0
#include "rtg_common.hpp"
#include "rtg_kernels.hpp"
#include "rtg_mega_impl.hpp"

namespace rtg {

// the general instantiations (the special ones: rtg_mega_pt.hip, rtg_mega_wh.hip)
template <bool STATS>
static hipError_t launch_general(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P,
                                 float* hdr, unsigned char* l, float* accum, DevCounters* cnt, hipStream_t stream) {
    return with_general(v, [&](auto D, auto PT) {
        return launch_render<decltype(D)::value, STATS, decltype(PT)::value>(S, C, P, hdr, l, accum, cnt, stream);
    });
}

hipError_t launch_mega(const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr, unsigned char* l,
                       float* accum, DevCounters* cnt, bool stats, int sk, int feat, hipStream_t stream,
                       hipEvent_t* ev) {
    const MegaVariant v =
        mega_variant(S.max_depth, C.path_tracing, C.russian_roulette, sk, feat, stats, mega_general());
    if (ev) (void)hipEventRecord(ev[0], stream);
    hipError_t e;
    if (v.special())
        e = v.pt ? launch_mega_pt(v, S, C, P, hdr, l, accum, cnt, stream)
                 : launch_mega_wh(v, S, C, P, hdr, l, accum, cnt, stream);
    else
        e = stats ? launch_general<true>(v, S, C, P, hdr, l, accum, cnt, stream)
                  : launch_general<false>(v, S, C, P, hdr, l, accum, cnt, stream);
    if (ev) (void)hipEventRecord(ev[1], stream);
    return e;
}

}  // namespace rtg
