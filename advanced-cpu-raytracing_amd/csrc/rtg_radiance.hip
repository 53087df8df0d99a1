// Radiance queries (rtgpu.h rtg_radiance_rays*): the fused render kernel's ray tree
// (rtg_mega_impl.hpp render_ray) below caller rays, one ray per lane.
//
//   k_radiance  ray i plays pixel p = ids ? ids[i] : first_pixel + i: sample s of it runs under
//               root_key(seed, p, s), the key k_render gives that pixel and sample, so the camera's
//               own rays (rtg_camera_rays) give the render's image bit for bit.
//
// The instantiations and their dispatch are k_render's: the uncounted render's variant
// (rtg_variants.hpp mega_variant) -- PT from the camera, MAXD from the scene's depth and the
// Russian-roulette rule, the feature-specialised (SK, FEAT) sets under the same conditions.

// the fused kernels keep trav_ray's ray unlaundered (rtg_walk.hpp: laundering it costs C2
// 6 %, profiles/r05ag_sphere_launder_ab.txt)
#define RTG_XFORM_LAUNDER 0
#include "rtg_common.hpp"
#include "rtg_kernels.hpp"
#include "rtg_mega_impl.hpp"

namespace rtg {

static_assert(sizeof(rtg_ray) == 32, "two 16-byte loads per ray");

// Lanes past n return before any walk: the cooperative large-leaf walk and the walks' ballots
// count live lanes only, as for k_query's.
// Samples: rgb = (((0 + c_0) + c_1) + ... + c_{k-1}) / (float)k per component, in float, in
// ascending sample order (no Gaussian weights: those are the render's pixel loop's).  One
// sample: c_0 itself, what k_render stores for a 1-spp camera.
template <int MAXD, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL>
__global__ __launch_bounds__(256, RTG_MEGA_WAVES) void k_radiance(const DevScene S, const DevCamera C, const RadianceParams P,
                                                  const float4* __restrict__ rays, const int* __restrict__ ids,
                                                  float4* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)P.n) return;
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
    const int pixel = ids ? ids[i] : P.first_pixel + (int)i;
    const int py = pixel / C.width, px = pixel - py * C.width;
    Ray r;
    r.o = mk(a.x, a.y, a.z);
    r.d = mk(b.x, b.y, b.z);
    const f3 eye = P.camera_eye ? ld3(C.pos) : r.o;
    Cnt<false> cn;
    float t = a.w;
    f3 color;
    if (P.sample_count <= 1) {
        color = render_ray<MAXD, false, PT, SK, FEAT>(S, C, r, b.w, a.w, eye, px, py, root_key(P.seed, pixel, P.sample_begin),
                                                      cn, t);
    } else {
        f3 acc = mk(0, 0, 0);
        for (int s = P.sample_begin; s < P.sample_begin + P.sample_count; ++s) {
            const f3 col = render_ray<MAXD, false, PT, SK, FEAT>(S, C, r, b.w, a.w, eye, px, py, root_key(P.seed, pixel, s), cn, t);
            acc.x += col.x;
            acc.y += col.y;
            acc.z += col.z;
        }
        const float k = (float)P.sample_count;
        color = mk(acc.x / k, acc.y / k, acc.z / k);
    }
    out[i] = make_float4(color.x, color.y, color.z, t);
}

template <int MAXD, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL>
static hipError_t launch_t(const DevScene& S, const DevCamera& C, const RadianceParams& P, const rtg_ray* rays,
                           const int* ids, float* rgbt, hipStream_t stream) {
    hipLaunchKernelGGL((k_radiance<MAXD, PT, SK, FEAT>), dim3((unsigned)(((long long)P.n + 255) / 256)), dim3(256), 0, stream,
                       S, C, P, reinterpret_cast<const float4*>(rays), ids, reinterpret_cast<float4*>(rgbt));
    return hipGetLastError();
}

template <bool PT>
static hipError_t launch_radiance_special(const MegaVariant& v, const DevScene& S, const DevCamera& C,
                                          const RadianceParams& P, const rtg_ray* rays, const int* ids, float* rgbt,
                                          hipStream_t stream) {
    return with_special(v, [&](auto D, auto K, auto F) {
        return launch_t<decltype(D)::value, PT, decltype(K)::value, decltype(F)::value>(S, C, P, rays, ids, rgbt, stream);
    });
}

hipError_t launch_radiance(const DevScene& S, const DevCamera& C, const RadianceParams& P, int sk, int feat,
                           const rtg_ray* rays, const int* ids, float* rgbt, hipStream_t stream) {
    // the render's variant, uncounted
    const MegaVariant v = mega_variant(S.max_depth, C.path_tracing, C.russian_roulette, sk, feat, false, mega_general());
    if (v.special())
        return v.pt ? launch_radiance_special<true>(v, S, C, P, rays, ids, rgbt, stream)
                    : launch_radiance_special<false>(v, S, C, P, rays, ids, rgbt, stream);
    return with_general(v, [&](auto D, auto PT) {
        return launch_t<decltype(D)::value, decltype(PT)::value>(S, C, P, rays, ids, rgbt, stream);
    });
}

}  // namespace rtg
