// Ray queries (rtgpu.h rtg_trace_rays*, rtg_camera_rays*): the render kernels' walks on caller
// rays, one ray per lane.
//
//   k_camera_rays  one pixel per lane: GenerateRay (camera_ray) written as an rtg_ray
//   k_query        one ray per lane: IntersectObjects (trace<>, per lane or as wave packets) or
//                  CastShadowRay (shadow_occluded: the any-hit wide walk with the reference walk
//                  where it is undecided), and optionally the hit's geometric normal (surface())
//
// The walks are the ones k_primary / k_shadow run, so a query answers exactly what a render's ray
// would: same boxes, same faces, same ties.
#include "rtg_common.hpp"
#include "rtg_kernels.hpp"

namespace rtg {

static_assert(sizeof(rtg_ray) == 32 && sizeof(rtg_hit) == 16, "two 16-byte loads per ray, one 16-byte store per hit");

__global__ __launch_bounds__(256) void k_camera_rays(const DevCamera C, const int row_begin, const int n,
                                                     const int sample, const unsigned long long seed,
                                                     float4* __restrict__ rays) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const int pixel = row_begin * C.width + (int)i;
    const int py = pixel / C.width, px = pixel - py * C.width;
    float mbTime;
    const Ray r = camera_ray(C, px, py, root_key(seed, pixel, sample), mbTime);
    rays[2 * (size_t)i] = make_float4(r.o.x, r.o.y, r.o.z, INFINITY);
    rays[2 * (size_t)i + 1] = make_float4(r.d.x, r.d.y, r.d.z, mbTime);
}

// ANY: occlusion.  PK: closest hit -- the packet walk (RTG_QUERY_COHERENT; scenes without large
// leaves); occlusion -- the any-hit wide walk (scenes with an any-hit tree), else the reference
// walk per lane.  The packet walks' decisions are per lane and exact, so incoherent rays under
// the hint cost time, never correctness.  Lanes past n take no part: the walks' ballots count
// live lanes only, as for k_primary's lanes outside the frame.
// NRM (closest hit): also the hit's normal -- its own instantiation, so that surface()'s registers
// do not weigh on the walk-only kernel.  The per-lane walk with the normal needs 66 VGPRs on plain
// scenes (12 B of scratch per lane at eight waves): that variant is compiled for seven.
constexpr int query_waves(bool any, int feat, bool pk, bool nrm) {
    if (any && pk) return RTG_WIDE_WAVES(feat);
    const int w = RTG_TRACE_WAVES(feat);
    return (nrm && !pk && w > 7) ? 7 : w;
}
template <bool ANY, int FEAT, bool PK, bool NRM = false>
__global__ __launch_bounds__(256, query_waves(ANY, FEAT, PK, NRM)) void k_query(
    const DevScene S, const float4* __restrict__ rays, const int n, int4* __restrict__ hits,
    float4* __restrict__ normals) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
    Cnt<false> cn;
    if constexpr (ANY) {
        // CastShadowRay with minT0 = limit = tmax; shadow rays carry motion-blur time 0
        const WaveBufs W{};
        const bool occ = shadow_occluded<false, FEAT, PK>(S, W, 0, a, make_float4(b.x, b.y, b.z, a.w), cn);
        hits[i] = make_int4(__float_as_int(a.w), occ ? 0 : -1, -1, 0);
    } else {
        Ray r;
        r.o = mk(a.x, a.y, a.z);
        r.d = mk(b.x, b.y, b.z);
        Hit h;
        trace<false, false, FEAT, PK>(S, r, b.w, a.w, INFINITY, h, cn);
        hits[i] = make_int4(__float_as_int(h.t), h.obj, h.face, 0);
        if constexpr (NRM) {
            float4 nn = make_float4(0.f, 0.f, 0.f, 0.f);
            if (h.obj >= 0) {
                const Surf s = surface<false, false>(S, r, b.w, h, cn);
                nn = make_float4(s.n.x, s.n.y, s.n.z, 0.f);
            }
            normals[i] = nn;
        }
    }
}

template <int FEAT>
static hipError_t launch_query_f(const DevScene& S, const rtg_ray* rays, int n, uint32_t flags, rtg_hit* hits,
                                 float4* normals, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    const float4* R = reinterpret_cast<const float4*>(rays);
    int4* H = reinterpret_cast<int4*>(hits);
    if (flags & RTG_QUERY_ANY_HIT) {
        // the wide walk where the render's shadow rays take it, without the deferral queues
        const bool fast = any_hit_wide(S, FEAT);
        if (fast) hipLaunchKernelGGL((k_query<true, FEAT, true>), grid, block, 0, st, S, R, n, H, nullptr);
        else hipLaunchKernelGGL((k_query<true, FEAT, false>), grid, block, 0, st, S, R, n, H, nullptr);
        return hipGetLastError();
    }
    if constexpr (!(FEAT & FEAT_BIGLEAF)) {
        if (flags & RTG_QUERY_COHERENT) {
            if (normals) hipLaunchKernelGGL((k_query<false, FEAT, true, true>), grid, block, 0, st, S, R, n, H, normals);
            else hipLaunchKernelGGL((k_query<false, FEAT, true>), grid, block, 0, st, S, R, n, H, nullptr);
            return hipGetLastError();
        }
    }
    if (normals) hipLaunchKernelGGL((k_query<false, FEAT, false, true>), grid, block, 0, st, S, R, n, H, normals);
    else hipLaunchKernelGGL((k_query<false, FEAT, false>), grid, block, 0, st, S, R, n, H, nullptr);
    return hipGetLastError();
}

hipError_t launch_query(const DevScene& S, int feat, const rtg_ray* rays, int n, uint32_t flags, rtg_hit* hits,
                        float4* normals, hipStream_t stream) {
    return with_trav_feat(feat, [&](auto F) {
        return launch_query_f<decltype(F)::value>(S, rays, n, flags, hits, normals, stream);
    });
}

hipError_t launch_camera_rays(const DevCamera& C, int row_begin, int row_end, int sample, unsigned long long seed,
                              rtg_ray* rays, hipStream_t stream) {
    const int n = (row_end - row_begin) * C.width;
    hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, stream, C, row_begin, n, sample,
                       seed, reinterpret_cast<float4*>(rays));
    return hipGetLastError();
}

}  // namespace rtg
