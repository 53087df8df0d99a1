// Crossing counts and signed distances (rtgpu.h rtg_count_crossings*, rtg_signed_distance_points*).
//
//   k_crossings<FEAT>         one ray per lane: the multi-hit walk counting every accepted hit
//                             instead of keeping k of them (rtg_crossings.hpp count_crossings), and
//                             how many of them enter.  One 8-byte store per ray.
//   k_signed_distance<FEAT>   one point per lane: k_closest's body (rtg_closest.hpp closest_point),
//                             then the crossing walk from the point along a wave-uniform direction,
//                             unbounded, at time 0.  The record is k_closest's with the count in
//                             pad0 and, on a hit with an odd count, the sign bit of dist set.  The
//                             phases run one after the other: the first one's registers are dead
//                             in the second, where only the candidate (6) and the point are held.
//
// There is no reference code for either: the host walks (host_query.cpp cross_one, signed_one)
// define them and these kernels repeat their decisions with the same float operations in the
// same order, so the two agree bit for bit.  No LDS, no atomics.
#include "rtg_closest.hpp"
#include "rtg_crossings.hpp"
#include "rtg_kernels.hpp"

namespace rtg {

static_assert(sizeof(rtg_ray) == 32 && sizeof(rtg_crossings) == 8, "two 16-byte loads per ray, one 8-byte store per result");
static_assert(sizeof(rtg_point) == 16 && sizeof(rtg_nearest) == 32, "one 16-byte load per point, two 16-byte stores per result");

// Waves per SIMD (the register budget is 512 / waves), from the compiler's resource report
// (profiles/r18_crossings_resource_lines.txt): per variant the highest count without scratch.
// VGPRs at that count, and the scratch per lane one count higher --
//     FEAT                 0 / 8 (meshes)   1 / 9 (+ spheres)   7 / 15 (everything)
//     k_crossings          8 (60)           6 (78)  7: 20 B     7 (72)  8: 28 B
//     k_signed_distance    8 (62)           8 (64)              6 (80)  7: 12 B
// (natural allocation 60 / 78 / 82 and 62 / 70 / 80: the large-leaf sets are the same code, leaves
// are tested in order whatever their size).  The fused kernel holds k_closest's occupancy except
// under transforms, where the walk keeps the world ray beside the local one.
constexpr int cross_waves(int feat) { return (feat & ~(FEAT_SPHERE | FEAT_BIGLEAF)) ? 7 : (feat & FEAT_SPHERE) ? 6 : 8; }
constexpr int sdf_waves(int feat) { return (feat & ~(FEAT_SPHERE | FEAT_BIGLEAF)) ? 6 : 8; }

template <int FEAT>
__global__ __launch_bounds__(256, cross_waves(FEAT)) void k_crossings(const DevScene S, const float4* __restrict__ rays,
                                                                      const int n, int2* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 ra = rays[2 * (size_t)i], rb = rays[2 * (size_t)i + 1];
    Ray r;
    r.o = mk(ra.x, ra.y, ra.z);
    r.d = mk(rb.x, rb.y, rb.z);
    const Crossings C = count_crossings<FEAT>(S, r, rb.w, ra.w);
    out[i] = make_int2(C.count, C.entering);
}

template <int FEAT>
__global__ __launch_bounds__(256, sdf_waves(FEAT)) void k_signed_distance(
    const DevScene S, const PointXf* __restrict__ xf, const float4* __restrict__ points, const int n, const float dx,
    const float dy, const float dz, int4* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 q = points[i];
    const Nearest B = closest_point<FEAT>(S, xf, mk(q.x, q.y, q.z), q.w * q.w);
    // a point that is not finite walks nothing
    const bool finite = fabsf(q.x) < INFINITY && fabsf(q.y) < INFINITY && fabsf(q.z) < INFINITY;
    int count = 0;
    if (finite) {
        Ray r;
        r.o = mk(q.x, q.y, q.z);
        r.d = mk(dx, dy, dz);
        count = count_crossings<FEAT>(S, r, 0.0f, INFINITY).count;
    }
    const bool hit = B.obj >= 0;
    const float dist = sqrtf(B.d2);
    out[2 * (size_t)i] = make_int4(__float_as_int(hit ? ((count & 1) ? -dist : dist) : q.w), B.obj, B.face, count);
    out[2 * (size_t)i + 1] = make_int4(__float_as_int(hit ? B.c.x : 0.f), __float_as_int(hit ? B.c.y : 0.f),
                                       __float_as_int(hit ? B.c.z : 0.f), 0);
}

hipError_t launch_crossings(const DevScene& S, int feat, const rtg_ray* rays, int n, rtg_crossings* out,
                            hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    return with_trav_feat(feat, [&](auto F) {
        hipLaunchKernelGGL((k_crossings<decltype(F)::value>), grid, block, 0, stream, S,
                           reinterpret_cast<const float4*>(rays), n, reinterpret_cast<int2*>(out));
        return hipGetLastError();
    });
}

hipError_t launch_signed_distance(const DevScene& S, const PointXf* xf, int feat, const rtg_point* points, int n,
                                  const float dir[3], rtg_nearest* out, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    return with_trav_feat(feat, [&](auto F) {
        hipLaunchKernelGGL((k_signed_distance<decltype(F)::value>), grid, block, 0, stream, S, xf,
                           reinterpret_cast<const float4*>(points), n, dir[0], dir[1], dir[2],
                           reinterpret_cast<int4*>(out));
        return hipGetLastError();
    });
}

}  // namespace rtg
