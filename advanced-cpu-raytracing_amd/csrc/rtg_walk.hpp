// The reference BVH walks -- per lane, cooperative large-leaf, and the two packet forms -- and the
// object loop (trace) over them.
#pragma once
#include "rtg_isect.hpp"

namespace rtg {

// Sequential form: each lane tests its leaves' faces in order inside the walk (scenes
// whose leaves are all small: the lean kernels).
// SEL: the face test with selects (tri_test_sel) and the slab test's exact fallback as a
// wave-uniform branch (k_primary 0.238 -> 0.228 ms, C5 1488 -> 1584 Mrays/s,
// profiles/r03seq_ab.txt); false: per-lane early outs and a divergent fallback, which the kernels
// with the cooperative large-leaf walk keep (walk_bvh: C3-ton's k_shadow 0.711 -> 0.774 ms with SEL)
template <bool ANY, bool STATS, bool SEL = true>
DEV bool walk_bvh_seq(const DevScene& S, int i, const int end, const Ray& r, float& minT, int& hitFace, float limit,
                      Cnt<STATS>& c) {
    bool hit = false;
    const RayRcp q = ray_rcp(r);
    while (i < end) {
        const float4 a = S.nodes[2 * i];
        const float4 b = S.nodes[2 * i + 1];
        c.template node<ANY>();
        const int skip = __float_as_int(b.z);
        if (box_hit_fast<SEL>(a.x, a.y, a.z, a.w, b.x, b.y, r, q, minT)) {
            const int leaf = __float_as_int(b.w);
            if (leaf >= 0) {
                int first = leaf >> 8, cnt = leaf & 255;
                if (leaf == LEAF_EXT) {
                    const int2 e = S.node_ext[i];
                    first = e.x;
                    cnt = e.y;
                }
                for (int f = first; f < first + cnt; ++f) {
                    c.template tri<ANY>();
                    float t;
                    if (SEL ? tri_test_sel(S.tris + 3 * f, r, minT, t) : tri_test_fast(S, f, r, minT, t)) {
                        minT = t;
                        hitFace = f;
                        hit = true;
                        if (ANY && t < limit) return true;
                    }
                }
                i = skip;
            } else {
                i = i + 1;
            }
        } else {
            i = skip;
        }
    }
    return hit;
}

// One step's large leaves, tested by the whole wave at once.  Every lane that reached a
// large leaf in this step (`coop`) posts an event -- its ray, minT and leaf -- to the wave's
// table in LDS; the (event, face) pairs of all events are dealt over the wave's lanes, and
// each candidate hit lowers its event's (t, face) key with an LDS 64-bit atomic min.  The
// result per event is the minimum over the leaf's faces with t < minT -- what the lane's
// own sequential loop would keep -- with no per-event reduction chain, and the faces'
// loads independent of each other.  Returns the calling lane's key (~0: none).
// Block size 256 (four waves, one table each), the size of every traversal kernel.
struct CoopEvent {
    float ox, oy, oz, dx, dy, dz, minT;
    int first, cnt, start;
    unsigned long long best;
};
DEV void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
DEV uint64_t coop_leaf_tests(const DevScene& S, uint64_t coop, const Ray& r, float minT, int first, int cnt) {
    __shared__ CoopEvent table[4][64];
    CoopEvent* E = table[threadIdx.x >> 6];
    const uint64_t em = __ballot(1);
    const int lane = threadIdx.x & 63;
    const int nact = __popcll(em);
    const int rank = __popcll(em & ((1ull << lane) - 1ull));
    const int ne = __popcll(coop);
    const int slot = cnt > 0 ? __popcll(coop & ((1ull << lane) - 1ull)) : -1;
    if (slot >= 0) {
        CoopEvent& e = E[slot];
        e.ox = r.o.x; e.oy = r.o.y; e.oz = r.o.z;
        e.dx = r.d.x; e.dy = r.d.y; e.dz = r.d.z;
        e.minT = minT;
        e.first = first;
        e.cnt = cnt;
        e.best = ~0ull;
    }
    wave_lds_sync();
    int total = 0, start = 0;
    for (int k = 0; k < ne; ++k) {
        if (k == slot) start = total;
        total += E[k].cnt;
    }
    if (slot >= 0) E[slot].start = start;
    wave_lds_sync();
    for (int w = rank; w < total; w += nact) {
        int lo = 0, hi = ne - 1;                        // last event with start <= w
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (E[mid].start <= w) lo = mid;
            else hi = mid - 1;
        }
        const CoopEvent& e = E[lo];
        Ray lr;
        lr.o = mk(e.ox, e.oy, e.oz);
        lr.d = mk(e.dx, e.dy, e.dz);
        const int f = e.first + (w - e.start);
        float t;
        if (tri_test_fast(S, f, lr, e.minT, t)) atomicMin(&E[lo].best, (unsigned long long)hit_key(t, f));
    }
    wave_lds_sync();
    const uint64_t mine = slot >= 0 ? (uint64_t)E[slot].best : ~0ull;
    wave_lds_sync();                                    // the table is rewritten next step
    return mine;
}

// BVH::IntersectBVH (bvh.cpp:5-30) as a stackless pre-order walk (rtg_device.hpp).
// ANY: stop at the first accepted face with t < limit (CastShadowRay semantics).
//
// Leaves of up to kCoopLeaf faces are tested by their lane in order.  Larger leaves
// (the reference's midpoint split keeps faces with equal centroid coordinates
// together, e.g. fans around a mesh pole, in leaves of hundreds of faces) are tested
// cooperatively: the walk loop runs while any lane of the wave is active, and every
// lane that reached such a leaf in this step has it tested by all active lanes of the
// wave in parallel, followed by a (t, face) minimum reduction.  That is exactly the
// sequential result: IntersectFace's acceptance is t < minT with minT shrinking over
// the leaf, so the survivor is the smallest t -- the first face among equal t -- of the
// faces with t < minT at leaf entry; for ANY, "some face with t < min(minT, limit)".
template <bool ANY, bool STATS, bool COOP>
DEV bool walk_bvh(const DevScene& S, int i, const int end, const Ray& r, float& minT, int& hitFace, float limit,
                  Cnt<STATS>& c) {
    if constexpr (!COOP) return walk_bvh_seq<ANY, STATS>(S, i, end, r, minT, hitFace, limit, c);
    // general kernels (the fused one) on scenes without large leaves: the plain walk, without
    // the wave-uniform loop and its per-step ballots (a uniform branch)
    if (!S.coop) return walk_bvh_seq<ANY, STATS, false>(S, i, end, r, minT, hitFace, limit, c);
    bool hit = false;
    const RayRcp q = ray_rcp(r);
    bool active = i < end;
    while (__ballot(active)) {
        int coopFirst = 0, coopCnt = 0;
        if (active) {
            const float4 a = S.nodes[2 * i];
            const float4 b = S.nodes[2 * i + 1];
            c.template node<ANY>();
            const int skip = __float_as_int(b.z);
            if (box_hit_fast(a.x, a.y, a.z, a.w, b.x, b.y, r, q, minT)) {
                const int leaf = __float_as_int(b.w);
                if (leaf >= 0) {
                    int first = leaf >> 8, cnt = leaf & 255;
                    if (leaf == LEAF_EXT) {
                        const int2 e = S.node_ext[i];
                        first = e.x;
                        cnt = e.y;
                    }
                    if (cnt > kCoopLeaf) {
                        coopFirst = first;
                        coopCnt = cnt;
                    } else {
                        for (int f = first; f < first + cnt; ++f) {
                            c.template tri<ANY>();
                            float t;
                            if (tri_test_fast(S, f, r, minT, t)) {
                                minT = t;
                                hitFace = f;
                                hit = true;
                                if (ANY && t < limit) {
                                    active = false;
                                    break;
                                }
                            }
                        }
                    }
                    i = skip;
                } else {
                    i = i + 1;
                }
            } else {
                i = skip;
            }
            if (i >= end) active = false;
        }
        const uint64_t coop = __ballot(coopCnt > 0);
        if (coop) {
            const uint64_t best = coop_leaf_tests(S, coop, r, minT, coopFirst, coopCnt);
            if (coopCnt > 0) {
                // counted as the whole leaf: the wave tests every face of it, also for any-hit
                // rays, where the sequential walk stops at the first accepted face (so C3/C4
                // shadow tri_tests depend on RTG_COOP_LEAF; images do not)
                c.template tri_n<ANY>((uint32_t)coopCnt);
                if (best != ~0ull) {
                    minT = __uint_as_float((uint32_t)(best >> 32));
                    hitFace = (int)(uint32_t)best;
                    hit = true;
                    if (ANY && minT < limit) active = false;
                }
            }
        }
    }
    return hit;
}

// Deferred large leaves (FEAT_BIGLEAF scenes, camera walk of production renders; k_bigleaf /
// k_hitfix in rtg_wave.hpp).  A lane that reaches a leaf of more than kDeferLeaf faces appends
// (its local ray, minT at entry, the leaf, its object, its pixel) to a queue and walks on
// without lowering minT.  Exact: the walk then visits a superset of the reference's boxes (its
// minT never drops below the reference's: only the deferred leaves' acceptances are missing
// from it, and every face the reference accepts elsewhere it accepts too), so the minimum in
// (t, object, face) order over its accepted faces and the deferred leaves' faces with t below
// their entry minT is at or below the reference's answer h; a candidate below h was never
// reached by the reference, i.e. it was culled at a minT above its t, so its own leaf box
// enters after t (hit before its box: rounding only).  Hence a winner whose leaf box passes at
// next_up(t) IS h; k_hitfix checks exactly that and runs the reference walk otherwise.
constexpr int kDeferLeaf = 16;
// A leaf is deferred only for the lanes of a wave that reach it when they are few; when many
// reach it together the wave tests it in the walk, every lane busy (RTG_DEFER_LANES: A/B)
#ifndef RTG_DEFER_LANES
#define RTG_DEFER_LANES 16
#endif
struct DeferCtx {
    float4* e;
    int* count;
    int cap;
    int ray;                          // the pixel's work-buffer index
    bool deferred;                    // this lane appended an entry
};

// The closest-hit packet walk, exact at leaves only (walk_bvh_packet's LX; DESIGN.md §2
// "Leaf-exact walks").  Parent boxes are exact min/max unions of their children and box_hit is
// monotone in the box and in minT, and a lane's minT never rises: in the reference's pre-order walk
// a lane tests the faces of leaf L iff L's own box passes at the minT the lane holds when pre-order
// reaches L (every ancestor was tested earlier, at a minT at least as large, and contains L's box).
// So inner-node decisions change which boxes are looked at, never a hit or a tie, provided
//   1. leaves come in pre-order and each leaf box gets the exact test (box_pass_v) per lane, and
//   2. no inner test culls a box the exact test keeps (slab_cons_v's predicate: it only adds boxes).
// The inner step is therefore the conservative value alone -- no certainty term, no exact fallback
// for sure or unsure lanes -- and the lanes carry no resume / rel / act: a lane that would have
// sat a subtree out fails its leaves there on its own.  The wave descends when any lane's value
// is > 0.  Lanes that cannot use the conservative form (off the fast path, |o inv| not finite:
// kc = NaN makes their value NaN; or a NaN from the box) take box_hit at inner nodes in a
// wave-uniform branch: voting "pass" instead would drag the wave of an axis-aligned camera ray
// through the whole tree.  A leaf takes the exact test alone (profiles/r12_leaf_walk_ab.txt).
template <bool DEFER>
DEV bool walk_bvh_packet_lx(const DevScene& S, int begin, int end, const Ray& r, float& minT, int& hitFace,
                            DeferCtx* dc, int k) {
    begin = __builtin_amdgcn_readfirstlane(begin);
    end = __builtin_amdgcn_readfirstlane(end);
    const int face0 = hitFace;
    const RayRcp q = ray_rcp(r);
    const SlabCons sc = slab_cons_ray(r, q);
    // (the exact test's constants stay live beside the conservative ones: 0.2359 ms against 0.2399
    // made at each leaf, profiles/r12_leaf_walk_ab.txt)
    const SlabFma sf = slab_fma(r, q);
    const float slack0 = slab_slack0(sf, q.fast);
    const float kc = (q.fast & sc.ok) ? 1.0f + 0x1p-20f : __builtin_nanf("");
    float minTc = minT * kc;                         // follows minT: renewed after a leaf's faces
    int i = begin;                                   // wave-uniform: begin, i + 1 or a record's skip word
    if (i >= end) return false;
    // The step's scalar side (profiles/r16_node_loops_isa_blocks.txt).  An inner
    // node costs 7 SALU and 4 branches around its 22 VALU: the offset's shift, i + 1, the record's load
    // (base + offset in the instruction), the leaf word's test, the NaN lanes' vote, the ballot's
    // compare and one select between i + 1 and skip, the second leaf test, the loop test at the foot.
    //  - The inner step and the leaf step are two if-thens in a row, not an if / else: the loop holds
    //    divergent branches (box_hit, the face test's fallback), so its control flow is structurized,
    //    and an if / else of uniform conditions comes out of that with a flag set, tested and branched
    //    on in blocks of their own.  The empty asm on `leaf` keeps the compiler from threading the two
    //    tests into an if / else again.
    //  - nx starts as the record's skip word and the select writes it in place, so the leaf path needs
    //    no move and the loop test reads one register on both paths.
    //  - i + 1 is made before the load (an asm statement: the compiler would sink it below), which
    //    lets the load's result overwrite i's register: no copy of nx into i at the foot, and the loop
    //    test falls through into the next step.  The LEAF_EXT leaf recovers its index as ip1 - 1.
    do {
        rtg_s8 nd;
        const uint32_t off = rec_off<32>(i);
        int ip1;
        asm("s_add_i32 %0, %1, 1" : "=s"(ip1) : "s"(i) : "scc");
        sload_node(S.nodes, off, nd);
        const float4 a = f4(nd[0], nd[1], nd[2], nd[3]), b = f4(nd[4], nd[5], nd[6], nd[7]);
        int nx = nd[6], leaf = nd[7];                // nx: where the walk goes next, the skip link unless a lane passes an inner node
        if (leaf < 0) {
            float pv = slab_cons_pk(a.x, a.y, a.z, a.w, b.x, b.y, sc, minTc);   // > 0: the lane passes
            if (__builtin_expect(__ballot(pv != pv) != 0, 0)) {
                if (pv != pv) pv = box_hit(a.x, a.y, a.z, a.w, b.x, b.y, r, minT) ? 1.0f : -1.0f;
            }
            const uint64_t pm = __builtin_amdgcn_ballot_w64(pv > 0.0f);
            asm("s_cmp_lg_u64 %[pm], 0\n\t"
                "s_cselect_b32 %[nx], %[ip1], %[nx]"
                : [nx] "+s"(nx)
                : [pm] "s"(pm), [ip1] "s"(ip1)
                : "scc");
        }
        asm("" : "+s"(leaf));
        if (leaf >= 0) {
            // the exact decision at the lane's own minT (slack0 = inf off the fast path: box_hit)
            bool pass = box_pass_v(a.x, a.y, a.z, a.w, b.x, b.y, r, sf, minT, INFINITY, slack0) > 0.0f;
            if (__ballot(pass)) {                    // (a leaf nobody reaches costs no face test)
                int first = leaf >> 8, cnt = leaf & 255;
                if (leaf == LEAF_EXT) {
                    const int2 e = S.node_ext[ip1 - 1];
                    first = __builtin_amdgcn_readfirstlane(e.x);
                    cnt = __builtin_amdgcn_readfirstlane(e.y);
                }
                if constexpr (DEFER) {
                    const uint64_t m = __ballot(pass);
                    if (cnt > kDeferLeaf && __popcll(m) <= RTG_DEFER_LANES) {
                        // one atomic per wave for the lanes that reached the leaf
                        const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
                        int base = 0;
                        if (lane == lead) base = atomicAdd(dc->count, __popcll(m));
                        base = __shfl(base, lead);
                        const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                        if (pass && slot < dc->cap) {
                            float4* qe = dc->e + 3 * (size_t)slot;
                            qe[0] = make_float4(r.o.x, r.o.y, r.o.z, minT);
                            qe[1] = make_float4(r.d.x, r.d.y, r.d.z, __int_as_float(dc->ray));
                            qe[2] = make_float4(__int_as_float(first), __int_as_float(cnt), __int_as_float(k), 0.f);
                            dc->deferred = true;
                            pass = false;                // queued: no test here, minT unchanged
                        }
                        // (a lane whose entry did not fit tests the leaf below)
                    }
                }
                for (int f = first; f < first + cnt; ++f) {
                    rtg_s8 ra;
                    rtg_s4 rb;
                    sload_rec(S.tris, rec_off<48>(f), ra, rb);
                    const float4 R[3] = {f4(ra[0], ra[1], ra[2], ra[3]), f4(ra[4], ra[5], ra[6], ra[7]),
                                         f4(rb[0], rb[1], rb[2], rb[3])};
                    float t;
                    const bool ok = tri_test_pk(R, r, minT, t, pass ? 1.0f : -1.0f) > 0.0f;
                    minT = ok ? t : minT;
                    hitFace = ok ? f : hitFace;
                }
                minTc = minT * kc;
            }
        }
        i = nx;
    } while (i < end);
    return hitFace != face0;
}

// Packet form of walk_bvh_seq for coherent rays (a wave's 8x8 pixel tile of camera rays): the
// wave walks ONE pre-order node sequence, the union of its lanes' walks, with a wave-uniform node
// index -- the 32-B node and 48-B face records are scalar loads (inline s_load: one per wave,
// through the scalar cache, no per-lane addresses for the texture path) -- and every lane keeps
// its own walk exactly: a lane whose box test fails at node n sets resume = skip(n) and sits out
// until the wave reaches resume, i.e. it ignores n's subtree [n, skip(n)) precisely as its own
// stackless walk would.  Each lane therefore tests the same boxes and faces, in the same order,
// with the same minT, as walk_bvh_seq -- same hits, same ties, same counters -- and the wave only
// adds masked-off idle lanes.  The wave advances to i + 1 when some active lane enters node i's
// subtree, else to skip(i).  The face test (tri_test_pk) and the slab test (box_pass_pk) take
// their exact fallbacks as wave-uniform branches; lanes outside their own walk take no part in
// either.  Closest hit only: any-hit rays take the per-lane walks or the any-hit tree (trace).
// LX: the caller asks for the leaf-exact walk (trace: the variants whose kernels keep their registers)
template <bool STATS, bool DEFER = false, bool LX = false>
DEV bool walk_bvh_packet(const DevScene& S, int begin, int end, const Ray& r, float& minT, int& hitFace,
                         Cnt<STATS>& c, DeferCtx* dc = nullptr, int k = 0) {
    // counting renders (the oracle's node visits) keep the walk below, exact at every node
    if constexpr (LX && !STATS) return walk_bvh_packet_lx<DEFER>(S, begin, end, r, minT, hitFace, dc, k);
    // the node range is the object's (wave-uniform): SGPRs, so the loop index and its bound stay
    // scalar; "a face was accepted" is read off hitFace at the end instead of a lane mask kept
    // through every iteration
    begin = __builtin_amdgcn_readfirstlane(begin);
    end = __builtin_amdgcn_readfirstlane(end);
    const int face0 = hitFace;
    const RayRcp q = ray_rcp(r);
    const SlabFma sf = slab_fma(r, q);               // the fused slab distances of box_pass_pk
    const float slack0 = slab_slack0(sf, q.fast);    // box_pass_pk: a ray off the fast path is never sure
    int resume = begin;                              // per lane: first node it takes part in again
    int i = begin;                                   // wave-uniform
    while (i < end) {
        const bool act = resume <= i;
        i = __builtin_amdgcn_readfirstlane(i);
        const int ip1 = i + 1;                       // (shared by rel and the next-node select)
        rtg_s8 nd;
        sload_node(rec_at<32>(S.nodes, i), nd);
        const float4 a = f4(nd[0], nd[1], nd[2], nd[3]), b = f4(nd[4], nd[5], nd[6], nd[7]);
        // (ndr is never read.  Without these copies of the record's words the compiler orders the
        // step's first VALU around the load differently and pads it with an s_nop per node: kept,
        // so that every kernel stays byte for byte what rounds 12 to 16 measured.)
        int ndr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) ndr[u] = nd[u];
        const int skip = __float_as_int(b.z);
        const int leaf = __float_as_int(b.w);
        if (act) c.template node<false>();
        bool pass = box_pass_pk(a.x, a.y, a.z, a.w, b.x, b.y, r, sf, minT, ip1 - resume, slack0);
        // a lane inside its walk that fails the box resumes at the box's skip; lanes outside it
        // already wait for a node past this box's subtree (resume >= skip), as do lanes that pass
        resume = max(resume, pass ? 0 : skip);
        // the next node and the leaf to test in five scalar instructions (the compiler kept the
        // two wave-uniform conditions as 64-bit masks with selects and branches between them):
        // lf = the leaf word when some lane passed, else 0 (no faces); next = lf < 0 (a passed
        // inner box) ? its first child : its skip
        const int cur = i;
        int lf;
        {
            const uint64_t pm = __builtin_amdgcn_ballot_w64(pass);
            int nx;
            asm("s_cmp_lg_u64 %[pm], 0\n\t"
                "s_cselect_b32 %[lf], %[leaf], 0\n\t"
                "s_cmp_lt_i32 %[lf], 0\n\t"
                "s_cselect_b32 %[nx], %[ip1], %[skip]"
                : [lf] "=&s"(lf), [nx] "=&s"(nx)
                : [pm] "s"(pm), [leaf] "s"(leaf), [ip1] "s"(ip1), [skip] "s"(skip)
                : "scc");
            i = nx;
        }
        if (lf > 0) {
            int first = leaf >> 8, cnt = leaf & 255;
            if (leaf == LEAF_EXT) {
                const int2 e = S.node_ext[cur];
                first = __builtin_amdgcn_readfirstlane(e.x);
                cnt = __builtin_amdgcn_readfirstlane(e.y);
            }
            if constexpr (DEFER) {
                const uint64_t m = __ballot(pass);
                if (cnt > kDeferLeaf && __popcll(m) <= RTG_DEFER_LANES) {
                    // one atomic per wave for the lanes that reached the leaf
                    const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
                    int base = 0;
                    if (lane == lead) base = atomicAdd(dc->count, __popcll(m));
                    base = __shfl(base, lead);
                    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                    if (pass && slot < dc->cap) {
                        float4* q = dc->e + 3 * (size_t)slot;
                        q[0] = make_float4(r.o.x, r.o.y, r.o.z, minT);
                        q[1] = make_float4(r.d.x, r.d.y, r.d.z, __int_as_float(dc->ray));
                        q[2] = make_float4(__int_as_float(first), __int_as_float(cnt), __int_as_float(k), 0.f);
                        dc->deferred = true;
                        pass = false;                // queued: no test here, minT unchanged
                    }
                    // (a lane whose entry did not fit tests the leaf below)
                }
            }
            for (int f = first; f < first + cnt; ++f) {
                rtg_s8 ra;
                rtg_s4 rb;
                sload_rec(rec_at<48>(S.tris, f), ra, rb);
                const float4 R[3] = {f4(ra[0], ra[1], ra[2], ra[3]), f4(ra[4], ra[5], ra[6], ra[7]),
                                     f4(rb[0], rb[1], rb[2], rb[3])};
                if (pass) c.template tri<false>();
                float t;
                const bool ok = tri_test_pk(R, r, minT, t, pass ? 1.0f : -1.0f) > 0.0f;
                minT = ok ? t : minT;
                hitFace = ok ? f : hitFace;
            }
        }
    }
    return hitFace != face0;
}

#ifndef RTG_XFORM_LAUNDER
#define RTG_XFORM_LAUNDER 1
#endif
// Sphere::Intersect (sphere.cpp:13-78): root selection and acceptance; lo/ld local ray.
DEV bool sphere_t(const DevObject& ob, const Ray& lr, float minT, float& tout) {
    const f3 center = mk(ob.center[0], ob.center[1], ob.center[2]);
    const float radius = ob.center[3];
    f3 oc = sub(lr.o, center);
    float c = dot(oc, oc) - (radius * radius);
    float b = 2 * dot(lr.d, oc);
    float a = dot(lr.d, lr.d);
    float delta = b * b - (4 * a * c);
    if (delta < 0.0f) return false;
    delta = sqrtf(delta);
    a = (float)(2.0 * a);
    float t1 = (-b + delta) / a;
    float t2 = (-b - delta) / a;
    float t = t1 < t2 ? t1 : t2;
    if (t1 < t2) { t = (t1 > 0.0f) ? t1 : t2; }
    else if (t2 < t1) { t = (t2 > 0.0f) ? t2 : t1; }
    tout = t;
    return t < minT && t > 0.0f;
}

// MOTION = false: the caller never meets a motion-blurred object (surface())
template <bool MOTION = true>
DEV Ray local_ray(const DevObject& ob, const Ray& r, float mbTime) {
    Ray lr;
    lr.o = xform(ob.inv, r.o, 1.0f);
    lr.d = xform(ob.inv, r.d, 0.0f);
    if (MOTION && (ob.flags & OBJF_MOTION_BLUR)) lr.o = add(lr.o, muls(ld3(ob.mbv), mbTime));
    return lr;
}
// Traversal-only variant: an exact identity transform changes at most the sign of a zero
// component (1*x + 0*y + ...), which no triangle / sphere decision or t value depends on, so it
// is skipped; the exact slab test does depend on it and is told (Ray::ident).  Shading
// (surface()) always applies the full transform.
DEV Ray trav_ray(const DevObject& ob, const Ray& r0, float mbTime) {
    // the ray laundered, so the compiler does not hoist the transform's double conversions of
    // it out of the caller's object loop (twelve VGPRs live through every mesh walk, spilled at
    // eight waves): C5's k_tree_trace / k_shadow 28 B of scratch -> 0, C5 1 715 -> 1 787 Mrays/s
    // (profiles/r05ag_sphere_launder_ab.txt); the fused kernels (rtg_mega*.hip) set
    // RTG_XFORM_LAUNDER 0 -- C2 loses 6 % with it
    Ray r = r0;
#if RTG_XFORM_LAUNDER
    asm volatile("" : "+v"(r.o.x), "+v"(r.o.y), "+v"(r.o.z), "+v"(r.d.x), "+v"(r.d.y), "+v"(r.d.z));
#endif
    if (!(ob.flags & OBJF_IDENTITY)) return local_ray(ob, r, mbTime);
    Ray lr = ident_ray(r);
    if (ob.flags & OBJF_MOTION_BLUR) lr.o = add(lr.o, muls(ld3(ob.mbv), mbTime));
    return lr;
}

struct Hit {
    float t;
    int obj, face;     // face < 0: sphere
    f3 o;              // world ray origin when the hit was accepted (normal/uv are computed then)
};

// IntersectObjects (raytracer.cpp:625-643) / CastShadowRay (raytracer.cpp:585-623).
// Closest hit: shared minT across objects, earlier object wins ties (strict <).
// Any hit (ANY): skip emissive meshes, true as soon as a hit with t < limit exists.
// The ray is updated in place like the reference's: an instance with motion blur whose
// bbox test fails leaves its offset on the ray origin (instancedMesh.cpp:18-60).
// FEAT (scene features the caller guarantees absent when the bit is clear) lets the
// traversal kernels drop whole code paths -- and their registers -- for plain scenes.
// PK: the packet walk (coherent camera rays; closest hit only).
template <bool ANY, bool STATS, int FEAT = FEAT_ALL, bool PK = false, bool DEFER = false>
DEV bool trace(const DevScene& S, Ray& r, float mbTime, float minT, float limit, Hit& h, Cnt<STATS>& c,
               DeferCtx* dc = nullptr) {
    static_assert(!(ANY && PK), "walk_bvh_packet is the closest-hit walk: any-hit rays take the per-lane walks");
    h.t = minT;
    h.obj = -1;
    h.face = -1;
    // instance world-bbox tests: the division-free slab test (same decisions, box_hit_fast);
    // the motion-blur quirk moves r.o between objects, never r.d
    const RayRcp rq = (FEAT & FEAT_INSTANCE) ? ray_rcp(r) : RayRcp{};
    int gskip = 0;                   // packet walks: this lane skips objects below gskip
    for (int k = 0; k < S.num_objects; ++k) {
        const DevObject& ob = S.objects[k];
        // Instance groups (runs of consecutive instances without motion blur): every member's
        // world box lies inside the group's, and the slab test is monotone in the box and in
        // minT, so a group box that fails at the current minT fails for every member tested
        // after it -- the members can be skipped with the same result.
        // Packet walks keep the object index wave-uniform (walk_bvh_packet needs one node
        // range per wave): a lane whose group box fails sits the group out, and the wave
        // jumps over it when every lane does.
        if ((FEAT & FEAT_INSTANCE) && ob.group_end > k) {
            const float4 ga = S.group_box[2 * k], gb = S.group_box[2 * k + 1];
            if constexpr (PK) {
                if (k >= gskip && !box_hit_fast(ga.x, ga.y, ga.z, gb.x, gb.y, gb.z, r, rq, h.t)) gskip = ob.group_end;
                if (!__ballot(k >= gskip)) {
                    k = ob.group_end - 1;
                    continue;
                }
            } else if (!box_hit_fast(ga.x, ga.y, ga.z, gb.x, gb.y, gb.z, r, rq, h.t)) {
                k = ob.group_end - 1;
                continue;
            }
        }
        if (PK && k < gskip) continue;
        c.obj();
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            c.sph();
            Ray lr = trav_ray(ob, r, mbTime);
            float t;
            if (sphere_t(ob, lr, h.t, t)) {
                h.t = t; h.obj = k; h.face = -1; h.o = r.o;
                if (ANY && t < limit) return true;
            }
            continue;
        }
        if (ANY && (ob.flags & OBJF_SHADOW_SKIP)) continue;
        if ((FEAT & FEAT_INSTANCE) && ob.kind == OBJ_INSTANCE) {
            // InstancedMesh::Intersect (instancedMesh.cpp:16-66): world bbox first
            Ray wr = r;
            if (ob.flags & OBJF_MOTION_BLUR) wr.o = add(wr.o, muls(ld3(ob.mbv), mbTime));
            if (!box_hit_fast(ob.bmin[0], ob.bmin[1], ob.bmin[2], ob.bmax[0], ob.bmax[1], ob.bmax[2], wr, rq, h.t)) {
                r.o = wr.o;
                continue;
            }
        }
        // Mesh::Intersect (mesh.cpp:158-188); the mesh bbox test equals the root-node test
        Ray lr = (FEAT & FEAT_XFORM) ? trav_ray(ob, r, mbTime) : ident_ray(r);
        int face = -1;
        float t = h.t;
        bool found;
        // The leaf-exact walk (walk_bvh_packet_lx) for scenes of plain meshes only.  Its six
        // conservative constants are live through the walk beside the ray a sphere, an instance or a
        // transform keeps: with it those variants lose a wave (k_primary, FEAT 15: 71 -> 79 VGPRs) or
        // gain scratch (FEAT 1: k_primary 0 -> 28 B, k_query 12 -> 64 B; FEAT 7: k_frame 8 -> 20 B), so
        // they keep the walk that is exact at every node (profiles/r12_resource_lines.txt).
        constexpr bool LX = !(FEAT & (FEAT_SPHERE | FEAT_INSTANCE | FEAT_XFORM));
        if constexpr (PK)
            found = walk_bvh_packet<STATS, DEFER, LX>(S, ob.node_begin, ob.node_end, lr, t, face, c, dc, k);
        else found = walk_bvh<ANY, STATS, (FEAT & FEAT_BIGLEAF) != 0>(S, ob.node_begin, ob.node_end, lr, t, face, limit, c);
        if (found) {
            h.t = t; h.obj = k; h.face = face; h.o = r.o;
            if (ANY && t < limit) return true;
        }
    }
    return !ANY && h.obj >= 0;
}

}  // namespace rtg
