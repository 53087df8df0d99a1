// The shadow-queue kernels shared by the wavefront and ray-tree pipelines.
#pragma once
#include "rtg_anyhit.hpp"
#include "rtg_frame.hpp"
#include "rtg_occupancy.hpp"

namespace rtg {

// Shadow queue in per-block segments (rtg_wave.hip k_shade, rtg_tree.hip k_tree_shade):
// one thread per queued shadow ray, CastShadowRay (raytracer.cpp:585-623).
// FAST (the wavefront pipeline): the RTG_SHADOW_MODE walk, its undecided rays by the
// reference walk in place (moving them to a second kernel to shed the reference walk's
// registers measured slower: the extra launch and the wide walk's own ~100 VGPRs); otherwise
// (the ray-tree pipeline, or RTG_RENDER_EXACT_SHADOW) the reference walk per lane,
// early-exit any-hit.
// grid (shade blocks, slots): block (b, c) takes entries [256c, 256c+256) of segment b
// CastShadowRay's answer for queue entry q (origin + initial minT o, direction + limit d).
// DEFER (large-leaf scenes, fast walk): the any-hit walk may queue large leaves; a ray with no
// answer of its own but queued leaves is pending (k_bigleaf_any, k_shadow_fin decide it)
enum : int { SS_PENDING = 1, SS_OCC = 2, SS_UNDECIDED = 4 };
template <bool STATS, int FEAT>
DEV int shadow_state_defer(const DevScene& S, const WaveBufs& W, size_t q, float4 o, float4 d, Cnt<STATS>& cn) {
    Ray r;
    r.o = mk(o.x, o.y, o.z);
    r.d = mk(d.x, d.y, d.z);
    AnyDefer ad{W.dq_e, W.dq_count + 2, W.dq_cap, (int)q, false};
    int res = trace_any_wide<STATS, FEAT, true>(S, r, o.w, d.w, cn, &ad);
    if (res < 0) {                                   // undecided: the reference walk (queued leaves moot)
        cn.fallback();
        Hit h;
        res = trace<true, STATS, FEAT>(S, r, 0.f, o.w, d.w, h, cn) ? 1 : 0;
    } else if (res == 0 && ad.deferred) {
        return SS_PENDING;
    }
    return res > 0 ? SS_OCC : 0;
}
template <bool STATS, int FEAT, bool FAST>
DEV bool shadow_occluded(const DevScene& S, const WaveBufs& W, size_t q, float4 o, float4 d, Cnt<STATS>& cn) {
    Ray r;
    r.o = mk(o.x, o.y, o.z);
    r.d = mk(d.x, d.y, d.z);
    int res = -1;
    if constexpr (FAST) {
        res = trace_any_wide<STATS, FEAT>(S, r, o.w, d.w, cn);
        if (res < 0) {                               // undecided: the reference walk
            cn.fallback();
            Hit h;
            res = trace<true, STATS, FEAT>(S, r, 0.f, o.w, d.w, h, cn) ? 1 : 0;
        }
    } else {
        Hit h;
        res = trace<true, STATS, FEAT>(S, r, 0.f, o.w, d.w, h, cn) ? 1 : 0;
    }
    return res > 0;
}

template <bool STATS, int FEAT, bool FAST, bool DEFER = false>
__global__ __launch_bounds__(256, FAST ? RTG_WIDE_WAVES(FEAT) : RTG_TRACE_WAVES(FEAT)) void k_shadow(
    const DevScene S, const WaveBufs W, DevCounters* counters) {
    const int k = blockIdx.y * 256 + threadIdx.x;
    const size_t q = ((size_t)blockIdx.x * W.num_slots) * 256 + k;
    Cnt<STATS> cn;
    if (k < W.q_count[blockIdx.x]) {
        if constexpr (DEFER) {
            const int st = shadow_state_defer<STATS, FEAT>(S, W, q, W.q_o[q], W.q_d[q], cn);
            W.shadow_state[q] = st;
            if (st == SS_OCC) W.occ[W.q_slot[q]] = 1;
        } else if (shadow_occluded<STATS, FEAT, FAST>(S, W, q, W.q_o[q], W.q_d[q], cn)) {
            W.occ[W.q_slot[q]] = 1;
        }
    }
    flush_counters<STATS>(cn, counters);
}

// The shadow rays' queued large leaves: one wave per entry, each lane taking entries (face
// records of the any-hit tree) 64 apart and the exact decisions of walk_wide_any_pk on each --
// a sufficient face (the leaf box passes at limit) occludes, a face reaching only at minT0
// leaves the ray undecided -- OR-ed into the ray's state.
template <int FEAT>
__global__ __launch_bounds__(256) void k_bigleaf_any(const DevScene S, const WaveBufs W) {
    const int n = min(W.dq_count[2], W.dq_cap);
    const int lane = threadIdx.x & 63;
    for (int e = (int)((blockIdx.x * 256u + threadIdx.x) >> 6); e < n; e += gridDim.x * 4) {
        const float4 a = W.dq_e[3 * (size_t)e], b = W.dq_e[3 * (size_t)e + 1], c4 = W.dq_e[3 * (size_t)e + 2];
        Ray lr;
        lr.o = mk(a.x, a.y, a.z);
        lr.d = mk(b.x, b.y, b.z);
        const float minT0 = a.w, limit = b.w;
        const int first = __float_as_int(c4.x), cnt = __float_as_int(c4.y), q = __float_as_int(c4.z);
        const bool conf = __float_as_int(c4.w) != 0;
        const RayRcp rq = ray_rcp(lr);
        int bits = 0;
        for (int x = first + lane; x < first + cnt; x += 64) {
            const float4* R = S.ahtris + 3 * (size_t)x;
            float t;
            if (!tri_test_fast_rec(R, lr, limit, t)) continue;
            const int ref = __float_as_int(R[0].w);
            const float4 na = S.nodes[2 * ref], nb = S.nodes[2 * ref + 1];
            if (!box_hit_fast(na.x, na.y, na.z, na.w, nb.x, nb.y, lr, rq, minT0)) continue;
            bits |= (conf && box_hit_fast(na.x, na.y, na.z, na.w, nb.x, nb.y, lr, rq, limit)) ? SS_OCC : SS_UNDECIDED;
        }
        const uint64_t occ = __ballot(bits & SS_OCC), und = __ballot(bits & SS_UNDECIDED);
        if (lane == 0 && (occ | und)) atomicOr(W.shadow_state + q, (occ ? SS_OCC : 0) | (und ? SS_UNDECIDED : 0));
    }
}

// A pending shadow ray's answer: occluded by a queued leaf, undecided (the reference walk), or
// not occluded; the general layout records it in occ, the one-light layout finishes the pixel.
DEV bool pending_occluded(int st) { return (st & SS_OCC) != 0; }

}  // namespace rtg
