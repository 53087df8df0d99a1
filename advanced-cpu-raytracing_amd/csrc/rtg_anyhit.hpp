// Walks of the 4-wide any-hit tree as wave packets: shadow rays (walk_wide_any_pk, trace_any_wide)
// and the opt-in ordered closest hit (walk_closest_pk, trace_closest_pk).
#pragma once
#include "rtg_walk.hpp"

namespace rtg {

// ---------------------------------------------------------------------------
// Shadow rays on the any-hit wide BVH (WNode, rtg_device.hpp)
// ---------------------------------------------------------------------------
// CastShadowRay (raytracer.cpp:585-623) answers one boolean: with minT0 = the initial minT
// (lightT + 0.01, or inf) and limit = lightT, the reference walks the objects in order,
// each with its BVH in its own order, minT shrinking to every accepted hit, and answers
// true once a hit with t < limit is found.  Until then minT_cur lies in [limit, minT0].
// For a face f of reference leaf L (box B_L), with tri_ok(f) = "IntersectFace accepts f
// with 0 < t < limit" (its early outs do not depend on minT):
//   * sufficient: tri_ok(f) and slab(B_L, limit) [and, for an instance, its world box at
//     limit].  Every ancestor box of L contains B_L (unions of face boxes, exact min/max),
//     and the slab test is monotone in the box and in minT, so every box on L's path
//     passes at any minT_cur >= limit, and f is accepted with t < limit <= minT_cur;
//   * necessary: some f with tri_ok(f) and slab(B_L, minT0) (same monotonicity).
// The wide walk visits every leaf whose box passes at minT0 (each wide child box contains
// the leaf boxes below it; the child test is conservative), in any order, and answers 1 at
// the first face meeting the sufficient condition.  A face meeting only the necessary one
// (its leaf box entry within rounding of lightT -- a light lying on a surface) or a full
// traversal stack make the answer "undecided" (-1): the caller then runs the reference
// walk for that ray.  0: no face meets the necessary condition -- not in shadow.
// (the kernels' waves per SIMD: RTG_WIDE_WAVES, rtg_occupancy.hpp)

// DEFER (large-leaf scenes, the packet walk): a leaf slot of more than RTG_DEFER_ANY_LEAF entries
// that at most RTG_DEFER_ANY_LANES lanes reach is queued for those lanes (k_bigleaf_any) instead
// of tested; the decisions are the same per face wherever they are taken, so the answer is
// unchanged.
#ifndef RTG_DEFER_ANY_LANES
#define RTG_DEFER_ANY_LANES 16
#endif
#ifndef RTG_DEFER_ANY_LEAF
#define RTG_DEFER_ANY_LEAF 16
#endif
struct AnyDefer {
    float4* e;
    int* count;
    int cap;
    int q;                            // the shadow ray's queue entry
    bool deferred;
};
// One mesh's any-hit tree (rtg_ahb.cpp; local ray lr) walked as a wave packet.  inst_conf: the
// instance's world box passes at limit (true for plain meshes).  Returns 1 / 0 / -1 as above.
// The wave visits one node sequence, the union of its live lanes' walks, so node, face and
// reference-leaf records are wave-uniform (scalar loads through the scalar cache, nothing through
// the vector memory path) and the stack is wave-uniform too (64 LDS words per wave, written by one
// live lane).  A lane tests a child, a face or a leaf box wherever the wave goes, also below boxes
// it failed itself: every decision is the
// exact one above (sufficient -> 1, necessary only -> undecided), so extra tests change no
// answer, and every leaf a lane's own walk reaches is still visited.  A lane leaves the packet
// at its first sufficient face; the wave stops when no live lane is left or the stack is empty.
// The nearest inner child of the first live lane goes next, the others onto the stack.
#define RTG_PK_STACK 64
// bound on a packet walk's steps (a walk visits each node once; past it the lanes are undecided)
#ifndef RTG_PK_MAX_STEPS
#define RTG_PK_MAX_STEPS 4096
#endif
template <bool STATS, bool DEFER = false>
DEV int walk_wide_any_pk(const DevScene& S, int node, const Ray& lr, float minT0, float limit, bool inst_conf,
                         Cnt<STATS>& c, AnyDefer* ad = nullptr) {
    // The lane state as values, every wave-level test one comparison (the mask version kept
    // live / occluded / undecided and the four child masks as SGPR pairs merged at every block
    // and spilled to VGPR lanes): livef > 0 walking (-2: occluded), the und flag, a child's hk > 0 taking it.
    const RayRcp q = ray_rcp(lr);
    const SlabCons sr = slab_cons_ray(lr, q);
    const bool fast = q.fast & sr.ok;
    const float minTc = minT0 * (1.0f + 0x1p-20f);
    const float icf = inst_conf ? 1.0f : -1.0f;
    float livef = fast ? 1.0f : -1.0f;
    int und = fast ? 0 : 1;                          // zero / tiny direction component: reference walk
    __shared__ int pk_stack[4][RTG_PK_STACK];        // the wave's stack (256-thread blocks)
    int* const stk = pk_stack[(threadIdx.x >> 6) & 3];
    int sp = 0;                                      // wave-uniform
    node = __builtin_amdgcn_readfirstlane(node);
    int steps = 0;                                   // bound: a walk visits each node once
    while (__ballot(livef > 0.0f)) {
        if (++steps > RTG_PK_MAX_STEPS) {
            und |= livef > 0.0f;
            break;
        }
        node = __builtin_amdgcn_readfirstlane(node);
        rtg_s16 na, nb;
        sload_wnode(S.anodes, rec_off<128>(node), na, nb);
        if (livef > 0.0f) c.wnode();
        float tn[4], hv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            hv[k] = slab_cons_v(__int_as_float(na[k]), __int_as_float(na[8 + k]), __int_as_float(nb[k]),
                                __int_as_float(na[4 + k]), __int_as_float(na[12 + k]), __int_as_float(nb[4 + k]), sr,
                                minTc, tn[k], livef);
        const int lead = __ffsll((long long)__ballot(livef > 0.0f)) - 1;
        int next = -1;
        float nextT = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cr = nb[8 + k], lfw = nb[12 + k];
            float hk = hv[k];
            if (cr == WCHILD_EMPTY || !__ballot(hk > 0.0f)) continue;
            if (cr >= 0) {
                const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tn[k]), lead));
                int spill = cr;
                if (t < nextT) {
                    spill = next;
                    next = cr;
                    nextT = t;
                }
                if (spill >= 0) {
                    if (sp < RTG_PK_STACK) {             // written by the first live lane
                        if ((int)(threadIdx.x & 63) == lead) stk[sp] = spill;
                        ++sp;
                    } else {
                        und |= livef > 0.0f;
                    }
                }
                continue;
            }
            const int first = lfw >> 8, cnt = lfw & 255;
            if constexpr (DEFER) {
                const uint64_t m = __ballot(hk > 0.0f);
                if (cnt > RTG_DEFER_ANY_LEAF && __popcll(m) <= RTG_DEFER_ANY_LANES) {
                    const int lane = threadIdx.x & 63, ld = __ffsll((long long)m) - 1;
                    int base = 0;
                    if (lane == ld) base = atomicAdd(ad->count, __popcll(m));
                    base = __shfl(base, ld);
                    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                    if (hk > 0.0f && slot < ad->cap) {
                        float4* qe = ad->e + 3 * (size_t)slot;
                        qe[0] = make_float4(lr.o.x, lr.o.y, lr.o.z, minT0);
                        qe[1] = make_float4(lr.d.x, lr.d.y, lr.d.z, limit);
                        qe[2] = make_float4(__int_as_float(first), __int_as_float(cnt), __int_as_float(ad->q),
                                            __int_as_float((int)inst_conf));
                        ad->deferred = true;
                        hk = -1.0f;
                    }
                }
            }
            for (int e = first; e < first + cnt; ++e) {
                rtg_s8 ra;
                rtg_s4 rb;
                sload_rec(S.ahtris, rec_off<48>(e), ra, rb);
                if (hk > 0.0f) c.template tri<true>();
                const float4 R[3] = {f4(ra[0], ra[1], ra[2], ra[3]), f4(ra[4], ra[5], ra[6], ra[7]), f4(rb[0], rb[1], rb[2], rb[3])};
                float t;
                const float okv = tri_test_pk(R, lr, limit, t, hk);
                if (!__ballot(okv > 0.0f)) continue;
                // the exact decisions on the face's reference leaf box: reachable at minT0
                // (necessary), and at limit (sufficient, for an instance whose world box passes)
                rtg_s8 rn;
                sload_node(S.nodes, rec_off<32>(ra[3]), rn);
                // (few faces get here: the exact decisions' constants are made on the spot, from a
                // laundered origin so that they are not hoisted into the walk's registers -- hoisted,
                // k_frame's scratch is 28 B per lane against 8; a lane with okv > 0 walks, so it is
                // on the fast path)
                Ray er = lr;
                asm volatile("" : "+v"(er.o.x), "+v"(er.o.y), "+v"(er.o.z));
                const SlabFma sf = slab_fma(er, q);
                const float slack0 = slab_slack0(sf, true);
                const float rv = box_pass_v(__int_as_float(rn[0]), __int_as_float(rn[1]), __int_as_float(rn[2]),
                                            __int_as_float(rn[3]), __int_as_float(rn[4]), __int_as_float(rn[5]), er, sf,
                                            minT0, okv, slack0);
                const float sv = box_pass_v(__int_as_float(rn[0]), __int_as_float(rn[1]), __int_as_float(rn[2]),
                                            __int_as_float(rn[3]), __int_as_float(rn[4]), __int_as_float(rn[5]), er, sf,
                                            limit, __builtin_elementwise_minimum(rv, icf), slack0);
                const bool suff = sv > 0.0f;
                livef = suff ? -2.0f : livef;         // (-2: occluded)
                hk = suff ? -1.0f : hk;
                und |= (rv > 0.0f) & !suff;
            }
        }
        if (!__ballot(livef > 0.0f)) break;
        if (next >= 0) {
            node = next;
            continue;
        }
        if (sp == 0) break;
        node = stk[--sp];
    }
    return livef < -1.5f ? 1 : (und ? -1 : 0);
}

// CastShadowRay on the wide BVH: objects in any order (the answer is a boolean), spheres
// exactly (a sphere hit with t < limit is accepted at any minT_cur >= limit, one with
// t >= limit never decides).  Returns 1 / 0 / -1 (undecided: run trace<true>).
template <bool STATS, int FEAT, bool DEFER = false>
DEV int trace_any_wide(const DevScene& S, const Ray& r, float minT0, float limit, Cnt<STATS>& c,
                       AnyDefer* ad = nullptr) {
    const RayRcp rq = (FEAT & FEAT_INSTANCE) ? ray_rcp(r) : RayRcp{};
    if ((FEAT & FEAT_INSTANCE) && !rq.fast) return -1;
    bool undecided = false;
    int gskip = 0;                   // packet walks: this lane skips objects below gskip
    for (int k = 0; k < S.num_objects; ++k) {
        const DevObject& ob = S.objects[k];
        if ((FEAT & FEAT_INSTANCE) && ob.group_end > k) {
            const float4 ga = S.group_box[2 * k], gb = S.group_box[2 * k + 1];
            // the packet walk needs one object (one root) per wave: a lane whose group box
            // fails sits the group out, and the wave jumps over it when every lane does
            if (k >= gskip && !box_hit_fast(ga.x, ga.y, ga.z, gb.x, gb.y, gb.z, r, rq, minT0))
                gskip = ob.group_end;
            if (!__ballot(k >= gskip)) {
                k = ob.group_end - 1;
                continue;
            }
        }
        if (k < gskip) continue;
        c.obj();
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            c.sph();
            Ray lr = trav_ray(ob, r, 0.f);
            float t;
            if (sphere_t(ob, lr, limit, t)) return 1;
            continue;
        }
        if (ob.flags & OBJF_SHADOW_SKIP) continue;
        bool conf = true;
        if ((FEAT & FEAT_INSTANCE) && ob.kind == OBJ_INSTANCE) {
            if (!box_hit_fast(ob.bmin[0], ob.bmin[1], ob.bmin[2], ob.bmax[0], ob.bmax[1], ob.bmax[2], r, rq, minT0))
                continue;
            conf = box_hit_fast(ob.bmin[0], ob.bmin[1], ob.bmin[2], ob.bmax[0], ob.bmax[1], ob.bmax[2], r, rq, limit);
        }
        const Ray lr = (FEAT & FEAT_XFORM) ? trav_ray(ob, r, 0.f) : ident_ray(r);
        if (ob.aroot < 0) return -1;                 // no any-hit tree for this mesh: reference walk
        const int res = walk_wide_any_pk<STATS, DEFER>(S, ob.aroot, lr, minT0, limit, conf, c, ad);
        if (res > 0) return 1;
        undecided |= res < 0;
    }
    return undecided ? -1 : 0;
}

// ---------------------------------------------------------------------------
// Opt-in ordered closest hit on the any-hit tree as wave packets (RTG_RENDER_ORDERED; meshes with
// identity transforms and spheres only).  Off by default; tests report its agreement with the
// reference order (tests/test_gpu_ordered.py).
// ---------------------------------------------------------------------------
// Order candidates by (t, object, face): the face index is the BVH-order one, so within a mesh
// it is the reference walk's order.  Let C be the faces IntersectFace accepts at minT = inf
// whose reference leaf box B_L passes the slab test at inf (the faces the reference can reach
// at all), and V the visible ones: B_L passes at next_up(t_f), i.e. B_L's entry is at most t_f
// (spheres count as visible).  IntersectObjects returns min(V) -- unless a face of C \ V (a
// hidden face: hit before its own leaf box's entry, by rounding alone) lies below min(V):
//   * when the reference reaches the ancestors of v = min(V) its minT exceeds t_v or is already
//     at most t_v; every ancestor box contains B_L(v), and the slab test is monotone in box and
//     minT, so the reference ends at or below v;
//   * a face f of C below the reference's answer h was not accepted although t_f < minT, so an
//     ancestor failed at some minT > t_f, hence B_L(f) fails at a minT above t_f: f is hidden.
// This walk finds min(V) on any tree whose boxes contain the reference leaf boxes (the any-hit
// tree's: unions of the B_L, exact float min / max): a child is culled only when its
// conservative slab test fails at the lane's best t, which a box holding a face of V below that
// best cannot do.  Hidden faces met in the walk are kept as a lower candidate; if one lies below
// the result, the lane takes the reference walk.  A hidden face in a culled box cannot be ruled
// out by a cheap test (its Cramer-rule t may sit below the box entry by rounding, without bound
// for rays grazing the face), so the result is checked, not proven: a lane whose
// culled boxes came within 2^-16 (relative) of its t takes the reference walk too.
//
// As a packet: the wave walks one node sequence (scalar-cache node / face / leaf records), the
// union of its lanes' walks; leaf children are tested before the inner ones (they can only lower
// t), the first lane with a passing inner child picks the nearest next, the others go onto the
// wave's LDS stack with the least entry distance of the lanes that passed them, and a popped entry
// no lane can still use is dropped (recorded as a cull at that distance).  Returns false for a lane
// whose result is not certain (caller: reference walk).
struct ClosestState {
    float bestT, hidT, cullMin;
    int bestK, bestF, hidK, hidF;
};

template <bool STATS>
DEV bool walk_closest_pk(const DevScene& S, int node, const int k, const Ray& lr, const RayRcp& q, const SlabRay& sr,
                         ClosestState& B, Cnt<STATS>& c) {
    __shared__ int ck_node[4][RTG_PK_STACK];
    __shared__ float ck_tn[4][RTG_PK_STACK];
    int* const stk = ck_node[(threadIdx.x >> 6) & 3];
    float* const stn = ck_tn[(threadIdx.x >> 6) & 3];
    // the stack is written by the first active lane (edge tiles run with partial waves)
    const bool writer = (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1;
    int sp = 0;                                      // wave-uniform
    int steps = 0;
    node = __builtin_amdgcn_readfirstlane(node);
    while (true) {
        if (++steps > RTG_PK_MAX_STEPS) return false;
        node = __builtin_amdgcn_readfirstlane(node);
        rtg_s16 na, nb;
        sload_wnode(rec_at<128>(S.anodes, node), na, nb);
        const float4 lox = f4(na[0], na[1], na[2], na[3]), hix = f4(na[4], na[5], na[6], na[7]);
        const float4 loy = f4(na[8], na[9], na[10], na[11]), hiy = f4(na[12], na[13], na[14], na[15]);
        const float4 loz = f4(nb[0], nb[1], nb[2], nb[3]), hiz = f4(nb[4], nb[5], nb[6], nb[7]);
        const int cidx[4] = {nb[8], nb[9], nb[10], nb[11]};
        const int lidx[4] = {nb[12], nb[13], nb[14], nb[15]};
        c.ewnode();
        const float minTc = cull_limit(B.bestT);
        float tn[4];
        bool h[4], hi[4];
        h[0] = slab_cons2(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, sr, minTc, tn[0], hi[0]);
        h[1] = slab_cons2(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, sr, minTc, tn[1], hi[1]);
        h[2] = slab_cons2(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, sr, minTc, tn[2], hi[2]);
        h[3] = slab_cons2(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, sr, minTc, tn[3], hi[3]);
        // leaf children first: their faces can only lower t
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cidx[j] == WCHILD_EMPTY || cidx[j] >= 0) continue;
            if (hi[j] & !h[j]) B.cullMin = fminf(B.cullMin, tn[j]);
            if (!__ballot(h[j])) continue;
            const int first = lidx[j] >> 8, cnt = lidx[j] & 255;
            for (int e = first; e < first + cnt; ++e) {
                rtg_s8 ra;
                rtg_s4 rb;
                sload_rec(rec_at<48>(S.ahtris, e), ra, rb);
                const float4 R[3] = {f4(ra[0], ra[1], ra[2], ra[3]), f4(ra[4], ra[5], ra[6], ra[7]),
                                     f4(rb[0], rb[1], rb[2], rb[3])};
                const int f = ra[7];
                if (h[j]) c.template tri<false>();
                float t;
                const bool ok = h[j] & tri_test_sel(R, lr, INFINITY, t, h[j]);
                const bool better = ok && hit_less(t, k, f, B.bestT, B.bestK, B.bestF);
                if (!__ballot(better)) continue;
                rtg_s8 rn;
                sload_node(rec_at<32>(S.nodes, ra[3]), rn);
                const float bx0 = __int_as_float(rn[0]), by0 = __int_as_float(rn[1]), bz0 = __int_as_float(rn[2]);
                const float bx1 = __int_as_float(rn[3]), by1 = __int_as_float(rn[4]), bz1 = __int_as_float(rn[5]);
                // visible: the reference leaf box passes at next_up(t) (its entry is at most t)
                const bool vis = better & box_hit_fast<true>(bx0, by0, bz0, bx1, by1, bz1, lr, q, next_up(t), better);
                const bool hcand = better & !vis;
                // a hidden face counts only if the reference can reach it at all (B_L passes at inf)
                const bool hid = hcand & box_hit_fast<true>(bx0, by0, bz0, bx1, by1, bz1, lr, q, INFINITY, hcand);
                if (vis) { B.bestT = t; B.bestK = k; B.bestF = f; }
                if (hid && hit_less(t, k, f, B.hidT, B.hidK, B.hidF)) { B.hidT = t; B.hidK = k; B.hidF = f; }
            }
        }
        // inner children against the (possibly lowered) best t: the nearest passing child of the
        // first lane that has one goes next, the others onto the stack
        const float minTc2 = cull_limit(B.bestT);
        bool h2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool inner = cidx[j] >= 0;
            h2[j] = inner & h[j] & (tn[j] < minTc2);
            if (inner & hi[j] & !h2[j]) B.cullMin = fminf(B.cullMin, tn[j]);
        }
        const uint64_t any = __ballot(h2[0] | h2[1] | h2[2] | h2[3]);
        int next = -1;
        if (any) {
            const int lead = __ffsll((long long)any) - 1;
            float nextT = INFINITY, nextTw = INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!__ballot(h2[j])) continue;
                const float tl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h2[j] ? tn[j] : INFINITY), lead));
                const float tw = wave_min_pos(h2[j] ? fmaxf(tn[j], 0.0f) : INFINITY);
                int spill = cidx[j];
                float spillT = tw;
                if (next < 0 || tl < nextT) {
                    spill = next;
                    spillT = nextTw;
                    next = cidx[j];
                    nextT = tl;
                    nextTw = tw;
                }
                if (spill >= 0) {
                    if (sp >= RTG_PK_STACK) return false;   // stack full: every lane takes the reference walk
                    if (writer) { stk[sp] = spill; stn[sp] = spillT; }
                    ++sp;
                }
            }
        }
        if (next >= 0) {
            node = next;
            continue;
        }
        // pop the next entry some lane can still use; the others are culls at their distance
        bool found = false;
        while (sp > 0) {
            --sp;
            const int n = stk[sp];
            const float tw = stn[sp];
            if (__ballot(tw < cull_limit(B.bestT))) {
                node = n;
                found = true;
                break;
            }
            B.cullMin = fminf(B.cullMin, tw);
        }
        if (!found) break;
    }
    return true;
}

// IntersectObjects on the any-hit trees (meshes with identity transforms and spheres only:
// FEAT 0 / FEAT_SPHERE).  true: h holds the reference's answer; false: take the reference walk.
template <bool STATS, int FEAT>
DEV bool trace_closest_pk(const DevScene& S, const Ray& r, Hit& h, Cnt<STATS>& c) {
    static_assert((FEAT & ~FEAT_SPHERE) == 0, "meshes with identity transforms and spheres only");
    const RayRcp q = ray_rcp(r);
    const SlabRay sr = slab_ray(r, q);
    ClosestState B;
    B.bestT = B.hidT = B.cullMin = INFINITY;
    B.bestK = B.bestF = B.hidK = B.hidF = 0x7FFFFFFF;
    bool sure = q.fast;                              // zero / tiny direction component: reference walk
    for (int k = 0; k < S.num_objects; ++k) {
        const DevObject& ob = S.objects[k];
        c.obj();
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            c.sph();
            float t;
            // a later object wins only with a strictly smaller t (sphere_t: 0 < t < minT)
            if (sphere_t(ob, r, B.bestT, t)) { B.bestT = t; B.bestK = k; B.bestF = -1; }
            continue;
        }
        if (ob.aroot < 0) return false;
        sure &= walk_closest_pk<STATS>(S, ob.aroot, k, r, q, sr, B, c);
    }
    sure &= !hit_less(B.hidT, B.hidK, B.hidF, B.bestT, B.bestK, B.bestF);
    sure &= !(B.bestT < INFINITY && B.cullMin <= B.bestT * (1.0f + 0x1p-16f));
    h.t = B.bestT;
    h.obj = B.bestT < INFINITY ? B.bestK : -1;
    h.face = B.bestT < INFINITY ? B.bestF : -1;
    h.o = r.o;
    return sure;
}

}  // namespace rtg
