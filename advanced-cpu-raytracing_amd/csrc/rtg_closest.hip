// Closest-point queries (rtgpu.h rtg_closest_points*): the nearest point of the scene's surface
// to each caller point, one point per lane.
//
//   k_closest<FEAT>   the object loop of host_query.cpp closest_one: spheres in closed form, meshes
//                     by two stackless passes over the (base) mesh's pre-order nodes -- a seed
//                     descent towards the nearer child box, then walk_bvh_seq's loop with "the
//                     box is farther than the held distance" in place of the slab test -- and the
//                     region-based point-to-triangle test (Ericson 5.1.5) at every visited face.
//
// There is no reference code for this query: the host walk defines it and this file repeats its
// decisions with the same float operations in the same order (-ffp-contract=off, IEEE division
// and square root), so the two agree bit for bit.  The tests are written with selects where the
// host branches; the values are the same.  Leaves are tested in order by their own lane, large
// ones (LEAF_EXT) too: a point's nearest faces are few, and the candidate rule needs no order.
// Placement comes from the PointXf side table (rtg_pointxf.hpp), an argument of its own:
// DevScene and DevObject are the ray walks' and stay as they are.  No LDS, no atomics.
#include "rtg_closest.hpp"
#include "rtg_kernels.hpp"

namespace rtg {

static_assert(sizeof(rtg_point) == 16 && sizeof(rtg_nearest) == 32, "one 16-byte load per point, two 16-byte stores per result");

// Waves per SIMD (the register budget is 512 / waves), from the compiler's resource report
// (profiles/r15_closest_resource_lines.txt): every variant fits the 64 registers of the highest
// count, 8, without scratch -- 56 VGPRs for meshes, 62 with spheres, 63 with transforms (56 / 62 /
// 64 unconstrained: the bound costs one register; the held candidate is 6 of them).

template <int FEAT>
__global__ __launch_bounds__(256, 8) void k_closest(const DevScene S, const PointXf* __restrict__ xf,
                                                                     const float4* __restrict__ points, const int n,
                                                                     int4* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 q = points[i];
    const Nearest B = closest_point<FEAT>(S, xf, mk(q.x, q.y, q.z), q.w * q.w);
    const bool hit = B.obj >= 0;
    out[2 * (size_t)i] = make_int4(__float_as_int(hit ? sqrtf(B.d2) : q.w), B.obj, B.face, 0);
    out[2 * (size_t)i + 1] = make_int4(__float_as_int(hit ? B.c.x : 0.f), __float_as_int(hit ? B.c.y : 0.f),
                                       __float_as_int(hit ? B.c.z : 0.f), 0);
}

hipError_t launch_closest(const DevScene& S, const PointXf* xf, int feat, const rtg_point* points, int n,
                          rtg_nearest* out, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    return with_trav_feat(feat, [&](auto F) {
        hipLaunchKernelGGL((k_closest<decltype(F)::value>), grid, block, 0, stream, S, xf,
                           reinterpret_cast<const float4*>(points), n, reinterpret_cast<int4*>(out));
        return hipGetLastError();
    });
}

}  // namespace rtg
