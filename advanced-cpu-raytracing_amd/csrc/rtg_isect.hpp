// Ray against box and triangle: the exact slab test and its fast and conservative forms, the
// face tests, scalar-cache record loads, hit keys and wave reductions.  The walks rest on these.
#pragma once
#include "rtg_math.hpp"

namespace rtg {

// ---------------------------------------------------------------------------
// Geometry
// ---------------------------------------------------------------------------
struct Ray {
    f3 o, d;
    // A local ray that stands for the reference's product with an exactly-identity inverse
    // transform (trav_ray skips the product; scenes without transforms never form it).  The
    // product is not quite the identity: for the identity inverse, and only for it, every row
    // ends in +0 * w, so a -0 component comes out as +0 (under any other matrix -- a translation's
    // last column is -t -- a -0 can survive, and local_ray forms that product in full) -- and the
    // slab test divides by it: for an origin in a box plane, 0 / 0 = NaN meets 1 / +0 = +inf (the
    // box passes) where 1 / -0 = -inf fails it.  Only box_hit looks at this (a ray with a zero
    // direction component is never on the fast path, and no face or sphere decision depends on
    // the sign of a zero).  A flag read in the exact branch, not a direction normalised once:
    // that keeps three more VGPRs live through every walk (DESIGN.md §5, round 17 notes).
    bool ident = false;
};
// the world ray as the local ray of an object under the identity transform
DEV Ray ident_ray(const Ray& r) {
    Ray lr = r;
    lr.ident = true;
    return lr;
}

// BoundingBox::doesIntersectWith (shape.hpp:78-100): true divisions, x-slab by
// comparison, y/z by fmin/fmax (NaN-ignoring), accept iff tmax>0 && tmax>=tmin && tmin<minT.
DEV bool box_hit(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, const Ray& r, float minT) {
    // (Ray::ident: x + 0 turns -0 into +0 and changes nothing else, as the skipped product does;
    // x + -0 changes nothing at all.  The direction is laundered so that the sums stay here, in
    // the rarely taken exact branch, instead of being hoisted into the walks' registers.)
    float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz));
    const float zero = r.ident ? 0.0f : -0.0f;
    dx += zero; dy += zero; dz += zero;
    float tx1 = (mnx - r.o.x) / dx;
    float tx2 = (mxx - r.o.x) / dx;
    float tmin = tx1, tmax = tx2;
    if (tx1 > tx2) { tmin = tx2; tmax = tx1; }
    float ty1 = (mny - r.o.y) / dy;
    float ty2 = (mxy - r.o.y) / dy;
    tmin = fmaxf(tmin, fminf(ty1, ty2));
    tmax = fminf(tmax, fmaxf(ty1, ty2));
    float tz1 = (mnz - r.o.z) / dz;
    float tz2 = (mxz - r.o.z) / dz;
    tmin = fmaxf(tmin, fminf(tz1, tz2));
    tmax = fminf(tmax, fmaxf(tz1, tz2));
    return tmax > 0 && tmax >= tmin && tmin < minT;
}

// The same predicate at a fraction of the cost.  Each slab distance (m - o) / d is
// computed as (m - o) * rcp(d): with v_rcp_f32 (<= 1 ulp) and two roundings the result is
// within 2^-22 |t| of the correctly rounded quotient, and min/max keep that bound.  Each
// of the three decisions is taken from the fast values only when they are farther than
// 4x that bound from the decision boundary; otherwise the exact division test above
// decides.  Hence the accepted set of boxes -- and every counter -- is identical.
// `fast` is false when a direction component is 0, subnormal or huge (rcp inexact /
// special values): those rays always take the exact test.
struct RayRcp {
    float ix, iy, iz;
    bool fast;
};
DEV RayRcp ray_rcp(const Ray& r) {
    RayRcp q;
    q.ix = __builtin_amdgcn_rcpf(r.d.x);
    q.iy = __builtin_amdgcn_rcpf(r.d.y);
    q.iz = __builtin_amdgcn_rcpf(r.d.z);
    const float lo = 0x1p-60f, hi = 0x1p60f;
    const float ax = fabsf(r.d.x), ay = fabsf(r.d.y), az = fabsf(r.d.z);
    q.fast = ax >= lo && ax <= hi && ay >= lo && ay <= hi && az >= lo && az <= hi;
    return q;
}
// UNI: the exact fallback as a wave-uniform branch (wave packets: every lane tests the same box)
// `on` (UNI only): lanes whose result is used -- the others do not vote for the fallback
template <bool UNI = false>
DEV bool box_hit_fast(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, const Ray& r,
                      const RayRcp& q, float minT, bool on = true) {
    // branch-free: every condition is evaluated (bitwise &, no short circuit), so the
    // common path is straight-line code with one rarely taken branch to the exact test
    const float tx1 = (mnx - r.o.x) * q.ix, tx2 = (mxx - r.o.x) * q.ix;
    const float ty1 = (mny - r.o.y) * q.iy, ty2 = (mxy - r.o.y) * q.iy;
    const float tz1 = (mnz - r.o.z) * q.iz, tz2 = (mxz - r.o.z) * q.iz;
    const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    const float atmin = fabsf(tmin), atmax = fabsf(tmax);
    const float slack = fmaf(0x1p-20f, atmin + atmax, 1e-30f);   // (fma: one rounding, tighter)
    // all three decisions clear of their boundaries.  NaN fails every comparison and an
    // infinite tmin or tmax makes the slack infinite, so both take the exact test; with both
    // finite, minT = inf passes the last test (tmax >= tmin decided, tmin < inf exact)
    const bool sure = (int)q.fast & (atmax >= 1e-30f) & (fabsf(tmax - tmin) > slack) &
                      (fabsf(tmin - minT) > fmaf(0x1p-20f, atmin, 1e-30f));
    bool hit = (tmax > 0) & (tmax >= tmin) & (tmin < minT);
    if constexpr (UNI) {
        if (__builtin_expect(__ballot(on & !sure) != 0, 0)) {
            if (on & !sure) hit = box_hit(mnx, mny, mnz, mxx, mxy, mxz, r, minT);
        }
        return hit;
    }
    if (__builtin_expect(!sure, 0)) return box_hit(mnx, mny, mnz, mxx, mxy, mxz, r, minT);
    return hit;
}

// NaN-propagating minimum of three (IEEE 754-2019 minimum; v_minimum3_f32 on gfx950):
// vmin3(a, b, c) > 0 is exactly (a > 0) & (b > 0) & (c > 0), NaN included
DEV float vmin3(float a, float b, float c) {
    return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c);
}

// box_hit_fast<true> for the camera packet walk with the lane's participation folded in, each
// predicate one comparison.  act = rel > 0 (rel = i + 1 - resume: the lane's own walk reaches
// this node).  When sure, the three decisions are clear of their boundaries, so each is the
// sign of one exactly-signed quantity -- tmax, tmax - tmin (nonzero: |.| > slack) and minT - tmin
// (a rounded difference has the sign of the exact one) -- and the conjunction is min(...) > 0;
// `sure` is min(|tmax - tmin| - slack, |tmin - minT| - slack', |tmax| - slack0) > 0 (each a rounded
// difference: exact sign; the last a hair stricter than >=), slack0 = inf when the ray's
// reciprocals are not exact enough (q.fast).  A NaN term leaves the lane unsure; a sure lane has
// no NaN among tmax, d1, d2.  Unsure lanes inside their walk take the exact test (uniform branch).
// Returns a value whose sign is the answer (> 0: the lane takes part and the box passes), so a
// caller's ballot of `> 0` is one comparison; actf > 0: the lane takes part.
// INT: actf is an integer (rel), so `act & !sure` is one comparison, !(max(su, 0.5 - actf) > 0).
// box_pass_t takes the six slab distances; the box for the exact fallback.
//
// The packet walks' slab distances are fused (SlabFma): t = fma(m, inv, n) with n = -fl(o * inv)
// computed once per (instance-local) ray, one instruction per box plane with the box coordinate
// as the scalar operand, where (m - o) * inv takes two.  Against the reference's fl(fl(m - o) / d):
// inv = (1 / d)(1 + e1), |e1| <= 2^-23 (v_rcp_f32, 1 ulp); n = -(o inv)(1 + e2), |e2| <= 2^-24; the
// fma rounds once, (1 + e3).  So t = ((m - o) / d (1 + e1) - o inv e2)(1 + e3): within
// (2^-23 + 2^-24) |t| + 2^-24 |o inv| (1 + 2^-24) of the true quotient, and the reference's two
// roundings are within 2^-23 |t| of it -- together at most
//     1.25 * 2^-22 |t| + 2^-24 A (1 + 2^-22),    A = max_k |fl(o_k inv_k)|.
// The absolute term is new: the subtract-first form cancels exactly and its error is purely
// relative.  The exact decisions keep their 2^-20 relative slack (more than 3x the relative bound
// per distance) and take the absolute term into the per-lane constant
//     slack0 = fast ? 1e-30 + 2^-21 A : inf
// (4x the absolute bound for tmin < minT and |tmax| > 0, 2x for the two distances of tmax - tmin),
// which is also the third certainty term, |tmax| - slack0: a literal became a register operand, so
// the node loop gains no instruction.  Unsure lanes take box_hit as before: every decision, node
// visit and triangle test is what it was.  (tests/test_slab_bound_model.py models both predicates.)
struct SlabFma {
    float ix, iy, iz;                 // rcp(d)
    float nx, ny, nz;                 // -fl(o * rcp(d))
    float A;                          // max |fl(o * rcp(d))|
};
DEV SlabFma slab_fma(const Ray& r, const RayRcp& q) {
    SlabFma s;
    const float px = r.o.x * q.ix, py = r.o.y * q.iy, pz = r.o.z * q.iz;
    s.ix = q.ix; s.iy = q.iy; s.iz = q.iz;
    s.nx = -px; s.ny = -py; s.nz = -pz;
    s.A = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
    return s;
}
// the exact decisions' per-lane constant (a ray off the fast path is never sure)
DEV float slab_slack0(const SlabFma& s, bool fast) { return fast ? fmaf(0x1p-21f, s.A, 1e-30f) : INFINITY; }
template <bool INT = false>
DEV float box_pass_t(float tx1, float tx2, float ty1, float ty2, float tz1, float tz2, float mnx, float mny, float mnz,
                     float mxx, float mxy, float mxz, const Ray& r, float minT, float actf, float slack0) {
    const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    const float atmin = fabsf(tmin), atmax = fabsf(tmax);
    const float d1 = tmax - tmin, d2 = minT - tmin;
    // (NaN-propagating minimum, v_minimum3_f32: any NaN term -- an infinite box face, inf - inf
    // -- leaves the lane unsure)
    const float su = vmin3(fabsf(d1) - fmaf(0x1p-20f, atmin + atmax, slack0), fabsf(d2) - fmaf(0x1p-20f, atmin, slack0),
                           atmax - slack0);
    float pv = __builtin_elementwise_minimum(fminf(fminf(tmax, d1), d2), actf);   // (a NaN actf: not taking part)
    const bool unsure = INT ? !(fmaxf(su, 0.5f - actf) > 0.0f) : (actf > 0.0f) & !(su > 0.0f);
    if (__builtin_expect(__ballot(unsure) != 0, 0)) {
        if (unsure) pv = box_hit(mnx, mny, mnz, mxx, mxy, mxz, r, minT) ? 1.0f : -1.0f;
    }
    return pv;
}
template <bool INT = false>
DEV float box_pass_v(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, const Ray& r, const SlabFma& q,
                     float minT, float actf, float slack0) {
    const float tx1 = fmaf(mnx, q.ix, q.nx), tx2 = fmaf(mxx, q.ix, q.nx);
    const float ty1 = fmaf(mny, q.iy, q.ny), ty2 = fmaf(mxy, q.iy, q.ny);
    const float tz1 = fmaf(mnz, q.iz, q.nz), tz2 = fmaf(mxz, q.iz, q.nz);
    return box_pass_t<INT>(tx1, tx2, ty1, ty2, tz1, tz2, mnx, mny, mnz, mxx, mxy, mxz, r, minT, actf, slack0);
}
DEV bool box_pass_pk(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, const Ray& r, const SlabFma& q,
                     float minT, int rel, float slack0) {
    // rel = i + 1 - resume > 0: the lane's walk reaches the node (as a float: sign exact)
    // (compared after the merge: the caller's ballot of it is then that comparison's mask)
    return box_pass_v<true>(mnx, mny, mnz, mxx, mxy, mxz, r, q, minT, (float)rel, slack0) > 0.0f;
}

// determinant (helperMath.cpp:132-138)
DEV float det3(float m00, float m01, float m02, float m10, float m11, float m12, float m20, float m21, float m22) {
    float first = m00 * (m11 * m22 - m12 * m21);
    float second = m10 * (m02 * m21 - m01 * m22);
    float third = m20 * (m01 * m12 - m11 * m02);
    return first + second + third;
}

// Mesh::IntersectFace (mesh.cpp:201-240): Cramer's rule, early outs in the same order.
// Returns t (or a value failing 0<t<minT) and beta/gamma.
DEV bool tri_test(const DevScene& S, int f, const Ray& r, float minT, float& tout, float* bg = nullptr) {
    const float4 A = S.tris[3 * f], E1 = S.tris[3 * f + 1], E2 = S.tris[3 * f + 2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    if (detA == 0) return false;
    const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
    float beta = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz) / detA;
    if (beta < 0) return false;
    float gama = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz) / detA;
    if (gama < 0 || gama + beta > 1) return false;
    float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
    if (bg) { bg[0] = beta; bg[1] = gama; }
    tout = t;
    return t > 0.0f && t < minT;
}

// Mesh::IntersectFace on a face record (any-hit tree entries: a copy of S.tris[3f..3f+2]).
DEV bool tri_test_rec(const float4* R, const Ray& r, float minT, float& tout) {
    const float4 A = R[0], E1 = R[1], E2 = R[2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    if (detA == 0) return false;
    const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
    float beta = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz) / detA;
    if (beta < 0) return false;
    float gama = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz) / detA;
    if (gama < 0 || gama + beta > 1) return false;
    float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
    tout = t;
    return t > 0.0f && t < minT;
}

// tri_test for traversal: beta and gamma from one reciprocal of detA, with the decisions
// beta<0, gamma<0 (exact signs unless a quotient underflows) and beta+gamma>1 (taken
// only when clear of 1 by 4x the error bound) identical to the division form; t itself
// is the correctly rounded quotient.  Falls back to tri_test when unsure.
DEV bool tri_test_fast(const DevScene& S, int f, const Ray& r, float minT, float& tout) {
    const float4 A = S.tris[3 * f], E1 = S.tris[3 * f + 1], E2 = S.tris[3 * f + 2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    const float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    if (detA == 0) return false;
    const float ad = fabsf(detA);
    if (ad >= 0x1p-100f && ad <= 0x1p100f) {
        const float rd = __builtin_amdgcn_rcpf(detA);
        const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
        const float nb = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz);
        const float beta = nb * rd;
        const bool bsure = nb == 0.0f || fabsf(beta) > 1e-30f;
        if (bsure) {
            if (beta < 0) return false;
            const float ng = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz);
            const float gama = ng * rd;
            const bool gsure = ng == 0.0f || fabsf(gama) > 1e-30f;
            if (gsure) {
                if (gama < 0) return false;
                const float sum = gama + beta;
                if (fabsf(sum - 1.0f) > fmaf(0x1p-19f, sum, 0x1p-22f)) {
                    if (sum > 1) return false;
                    float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
                    tout = t;
                    return t > 0.0f && t < minT;
                }
            }
        }
    }
    return tri_test(S, f, r, minT, tout);
}
// The same on a face record (any-hit tree entries).
DEV bool tri_test_fast_rec(const float4* R, const Ray& r, float minT, float& tout) {
    const float4 A = R[0], E1 = R[1], E2 = R[2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    const float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    if (detA == 0) return false;
    const float ad = fabsf(detA);
    if (ad >= 0x1p-100f && ad <= 0x1p100f) {
        const float rd = __builtin_amdgcn_rcpf(detA);
        const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
        const float nb = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz);
        const float beta = nb * rd;
        const bool bsure = nb == 0.0f || fabsf(beta) > 1e-30f;
        if (bsure) {
            if (beta < 0) return false;
            const float ng = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz);
            const float gama = ng * rd;
            const bool gsure = ng == 0.0f || fabsf(gama) > 1e-30f;
            if (gsure) {
                if (gama < 0) return false;
                const float sum = gama + beta;
                if (fabsf(sum - 1.0f) > fmaf(0x1p-19f, sum, 0x1p-22f)) {
                    if (sum > 1) return false;
                    float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
                    tout = t;
                    return t > 0.0f && t < minT;
                }
            }
        }
    }
    return tri_test_rec(R, r, minT, tout);
}

// tri_test_fast_rec with selects (wave packets, where every lane tests the same face, and the
// per-lane walk, walk_bvh_seq's SEL): the same decisions -- the early outs become lane masks,
// and the two costly parts (the t division, the exact fallback) wave-uniform branches taken
// when some lane needs them.
// `on`: lanes whose result is used (the others neither take the division nor the fallback)
DEV bool tri_test_sel(const float4* R, const Ray& r, float limit, float& tout, bool on = true) {
    const float4 A = R[0], E1 = R[1], E2 = R[2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    const float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    const float ad = fabsf(detA);
    const float rd = __builtin_amdgcn_rcpf(detA);
    const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
    const float nb = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz);
    const float ng = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz);
    const float beta = nb * rd, gama = ng * rd, sum = gama + beta;
    const bool zero = detA == 0;
    const bool range = (ad >= 0x1p-100f) & (ad <= 0x1p100f);
    const bool bsure = (nb == 0.0f) | (fabsf(beta) > 1e-30f);
    const bool gsure = (ng == 0.0f) | (fabsf(gama) > 1e-30f);
    const bool ssure = fabsf(sum - 1.0f) > fmaf(0x1p-19f, sum, 0x1p-22f);
    // tri_test_fast_rec's decision tree: false / t test / exact fallback
    const bool b_out = range & bsure & (beta < 0);
    const bool g_out = range & bsure & !(beta < 0) & gsure & (gama < 0);
    const bool s_ok = range & bsure & !(beta < 0) & gsure & !(gama < 0) & ssure;
    const bool no = zero | b_out | g_out | (s_ok & (sum > 1)) | !on;
    const bool tt = on & !zero & s_ok & !(sum > 1);
    bool hit = false;
    if (__ballot(tt)) {
        const float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
        tout = t;
        hit = tt & (t > 0.0f) & (t < limit);
    }
    const bool unsure = !no & !tt;
    if (__builtin_expect(__ballot(unsure) != 0, 0)) {
        if (unsure) hit = tri_test_rec(R, r, limit, tout);
    }
    return hit;
}

// tri_test_sel with every decision a single comparison of a value (the packet walks' face
// tests; lanes with onf > 0 take part).  Returns a value > 0 exactly when IntersectFace
// accepts the face with 0 < t < limit (t in tout).  Sure candidates: |detA| in range (strict),
// beta and gama above 1e-30 and 1 - sum above the bound of tri_test_fast_rec (each a rounded
// difference, so its sign is the comparison's); sure rejections: detA == 0, or in range and
// beta or gama below -1e-30 or sum - 1 above the bound (any one decides, in whatever order the
// reference tests them: each makes IntersectFace return false).  Everything else -- also the
// exact zeros nb == 0 / ng == 0 that tri_test_fast_rec takes as sure -- takes the exact test
// (uniform branch).  AND is the NaN-propagating minimum, OR the NaN-dropping max.
DEV float tri_test_pk(const float4* R, const Ray& r, float limit, float& tout, float onf) {
    const float4 A = R[0], E1 = R[1], E2 = R[2];
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    const float detA = det3(E1.x, E2.x, dx, E1.y, E2.y, dy, E1.z, E2.z, dz);
    const float ad = fabsf(detA);
    const float rd = __builtin_amdgcn_rcpf(detA);
    const float sx = A.x - r.o.x, sy = A.y - r.o.y, sz = A.z - r.o.z;
    const float nb = det3(sx, E2.x, dx, sy, E2.y, dy, sz, E2.z, dz);
    const float ng = det3(E1.x, sx, dx, E1.y, sy, dy, E1.z, sz, dz);
    const float beta = nb * rd, gama = ng * rd, sum = gama + beta;
    const float sslack = fmaf(0x1p-19f, sum, 0x1p-22f);
    const float rng = __builtin_elementwise_minimum(ad - 0x1p-100f, 0x1p100f - ad);
    const float ttv = __builtin_elementwise_minimum(vmin3(beta - 1e-30f, gama - 1e-30f, (1.0f - sum) - sslack),
                                                    __builtin_elementwise_minimum(rng, onf));
    const float rjv = __builtin_elementwise_minimum(fmaxf(fmaxf(-1e-30f - beta, -1e-30f - gama), (sum - 1.0f) - sslack),
                                                    rng);
    float hv = -1.0f;
    if (__ballot(ttv > 0.0f)) {
        const float t = det3(E1.x, E2.x, sx, E1.y, E2.y, sy, E1.z, E2.z, sz) / detA;
        tout = t;
        hv = vmin3(ttv, t, limit - t);               // 0 < t < limit (rounded difference: exact sign)
    }
    const bool unsure = (onf > 0.0f) & !(ttv > 0.0f) & !(rjv > 0.0f) & (detA != 0.0f);
    if (__builtin_expect(__ballot(unsure) != 0, 0)) {
        if (unsure) hv = tri_test_rec(R, r, limit, tout) ? 1.0f : -1.0f;
    }
    return hv;
}

// Wave-uniform records through the scalar cache (the compiler keeps vector loads here: the
// kernels store to global memory, so it cannot prove the records unclobbered).  Read-only
// scene data, written by copies before the launch.
typedef int rtg_s16 __attribute__((ext_vector_type(16)));
typedef int rtg_s8 __attribute__((ext_vector_type(8)));
typedef int rtg_s4 __attribute__((ext_vector_type(4)));
DEV const void* uniform_ptr(const void* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const void*)(((uint64_t)hi << 32) | lo);
}
DEV void sload_wnode(const WNode* p, rtg_s16& a, rtg_s16& b) {   // 128 B
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(uniform_ptr(p)) : "memory");
}
DEV void sload_rec(const float4* p, rtg_s8& a, rtg_s4& b) {      // 48 B: a face record
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(uniform_ptr(p)) : "memory");
}
DEV void sload_node(const float4* p, rtg_s8& a) {                // 32 B: a reference BVH node
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a) : "s"(uniform_ptr(p)) : "memory");
}
// The same records at base + a 32-bit byte offset held in an SGPR (rec_off below): the load adds
// the two itself, zero-extending the offset as rec_at does, and the address's s_add_u32 /
// s_addc_u32 pair goes (walk_bvh_packet_lx, walk_wide_any_pk).
DEV void sload_wnode(const WNode* base, uint32_t off, rtg_s16& a, rtg_s16& b) {
    asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %3 offset:0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(uniform_ptr(base)), "s"(off) : "memory");
}
DEV void sload_rec(const float4* base, uint32_t off, rtg_s8& a, rtg_s4& b) {
    asm volatile("s_load_dwordx8 %0, %2, %3\n\ts_load_dwordx4 %1, %2, %3 offset:0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(uniform_ptr(base)), "s"(off) : "memory");
}
DEV void sload_node(const float4* base, uint32_t off, rtg_s8& a) {
    asm volatile("s_load_dwordx8 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a) : "s"(uniform_ptr(base)), "s"(off) : "memory");
}
DEV float4 f4(int x, int y, int z, int w) {
    return make_float4(__int_as_float(x), __int_as_float(y), __int_as_float(z), __int_as_float(w));
}
// 64-bit lexicographic (t, face) key of a candidate hit; t > 0, so the float bits order
// like the values.  Non-candidates: ~0.
DEV uint64_t hit_key(float t, int f) { return ((uint64_t)__float_as_uint(t) << 32) | (uint32_t)f; }

// Minimum of `key` over the lanes set in `em` (the wave's active lanes).  A butterfly
// needs every lane; with a partial exec mask (image-edge tiles, rays that skip an
// instance, the fused kernel's ray trees) the active lanes' keys are read one by one.
DEV uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
DEV uint64_t wave_min_key(uint64_t key, uint64_t em) {
    if (em == ~0ull) {
        const int lane = threadIdx.x & 63;
        for (int m = 1; m < 64; m <<= 1) {
            const uint64_t other = shfl64(key, lane ^ m);
            if (other < key) key = other;
        }
        return key;
    }
    uint64_t acc = ~0ull;
    while (em) {
        const int l = __ffsll((long long)em) - 1;
        em &= em - 1;
        const uint64_t v = shfl64(key, l);
        if (v < acc) acc = v;
    }
    return acc;
}

// packet walks address their scalar records by 32-bit byte offsets: two scalar ops fewer per
// record than a 64-bit index; scenes are limited to 2^25 faces (rtg_scene_create), which keeps
// every node, wide node and face-record array below 4 GiB (k_primary 0.1881 -> 0.1828 ms,
// profiles/r04aa_addr_on_ab.txt)
template <int BYTES, typename T>
DEV const T* rec_at(const T* base, int i) {
    return (const T*)((const char*)base + (uint32_t)i * (uint32_t)BYTES);
}
template <int BYTES>
DEV uint32_t rec_off(int i) {
    return (uint32_t)i * (uint32_t)BYTES;
}

// (t, object, face) as one 64-bit key: t > 0 orders like its bits; objects < 2^12, faces < 2^20
// (defer_ok); a sphere's face field is all ones
DEV uint64_t obj_key(float t, int k, int f) {
    return ((uint64_t)__float_as_uint(t) << 32) | ((uint64_t)(uint32_t)k << 20) | (uint64_t)((uint32_t)f & 0xFFFFFu);
}

// Conservative slab test: accepts every box the exact test (box_hit) accepts at minT.  The
// fast slab distances (m - o) * rcp(d) are within 2^-22 |t| of the exact quotients (RayRcp,
// q.fast), so exact tmax > 0, tmax >= tmin, tmin < minT imply the tests below on the fast
// values (minTc at least minT (1 + 2^-21); the 1e-30 terms cover subnormal products).
// slab_cons2 (the ordered closest walk) is this subtract-first form, its error purely relative;
// hinf: the box passes at minT = inf.  slab_cons_v / slab_cons_pk below are the fused form.
struct SlabRay {
    f3 o;
    float ix, iy, iz;
};
DEV SlabRay slab_ray(const Ray& r, const RayRcp& q) {
    SlabRay s;
    s.o = r.o;
    s.ix = q.ix; s.iy = q.iy; s.iz = q.iz;
    return s;
}
DEV bool slab_cons2(float lx, float ly, float lz, float hx, float hy, float hz, const SlabRay& s, float minTc,
                    float& tnear, bool& hinf) {
    const float tx1 = (lx - s.o.x) * s.ix, tx2 = (hx - s.o.x) * s.ix;
    const float ty1 = (ly - s.o.y) * s.iy, ty2 = (hy - s.o.y) * s.iy;
    const float tz1 = (lz - s.o.z) * s.iz, tz2 = (hz - s.o.z) * s.iz;
    const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    tnear = tmin;
    hinf = (tmax > -1e-30f) & (tmax >= fmaf(tmin, 1.0f - 0x1p-21f, -1e-30f));
    return hinf & (tmin < minTc);
}

// The conservative test as a value (> 0: it passes and the lane walks, livef > 0), on fused
// slab distances (SlabFma above) whose absolute error term is folded into the per-ray constants,
// axis by axis.  A ray-wide slack of 2^-22 max_k |o_k inv_k| in the three comparisons would keep
// boxes for nothing whenever one direction component is small: that axis's |o inv| is huge and
// would swamp the -eps / d of a ray leaving a flat box on another axis (`spheres`: 692 face tests
// where the reference's walk has none).  Instead each axis carries two constants,
//     a_k = n_k - s_k e_k  (with the box minimum),   b_k = n_k + s_k e_k  (with the maximum),
//     n_k = -fl(o_k inv_k),  e_k = 2^-22 |n_k|,  s_k = sign(inv_k),
// so the axis's entry distance -- fma(lo, inv, a) for inv > 0, fma(hi, inv, b) for inv < 0 -- is
// lowered by e_k and its exit distance raised by e_k: four times the fused form's absolute error
// 2^-24 |n_k| (1 + 2^-22), less the 2^-24 |n_k| of rounding a_k / b_k themselves.  min / max pick
// entry and exit as before (entry - e <= exit + e).  What is left is relative, 1.25 * 2^-22 |t| per
// distance: exact tmax > 0, tmax >= tmin, tmin < minT imply tmax + 1e-30 > 0,
// tmax - (tmin (1 - 2^-20) - 1e-30) + 1e-30 > 0 (two distances carry 2.5 * 2^-22 together: 2^-20
// covers it with margin, 2^-21 would not) and minTc - tmin > 0 with minTc = minT (1 + 2^-20); the
// 1e-30 terms cover subnormal products.  Rounded sums and differences keep their signs, so each
// is one strict comparison.  The test only has to keep every box the exact test keeps
// (walk_wide_any_pk: extra boxes change no answer).  Six constants per ray instead of three
// origin components; no instruction in the loop beyond the six fused distances.
struct SlabCons {
    float ix, iy, iz;
    float ax, ay, az, bx, by, bz;
    bool ok;                          // |o inv| finite (else the ray takes the reference walk)
};
DEV SlabCons slab_cons_ray(const Ray& r, const RayRcp& q) {
    SlabCons s;
    const float px = r.o.x * q.ix, py = r.o.y * q.iy, pz = r.o.z * q.iz;
    const float ex = copysignf(0x1p-22f * fabsf(px), q.ix), ey = copysignf(0x1p-22f * fabsf(py), q.iy),
                ez = copysignf(0x1p-22f * fabsf(pz), q.iz);
    s.ix = q.ix; s.iy = q.iy; s.iz = q.iz;
    s.ax = -px - ex; s.ay = -py - ey; s.az = -pz - ez;
    s.bx = -px + ex; s.by = -py + ey; s.bz = -pz + ez;
    s.ok = fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) <= 0x1p100f;
    return s;
}
DEV float slab_cons_v(float lx, float ly, float lz, float hx, float hy, float hz, const SlabCons& s, float minTc,
                      float& tnear, float livef) {
    const float tx1 = fmaf(lx, s.ix, s.ax), tx2 = fmaf(hx, s.ix, s.bx);
    const float ty1 = fmaf(ly, s.iy, s.ay), ty2 = fmaf(hy, s.iy, s.by);
    const float tz1 = fmaf(lz, s.iz, s.az), tz2 = fmaf(hz, s.iz, s.bz);
    const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    tnear = tmin;
    return __builtin_elementwise_minimum(
        vmin3(tmax + 1e-30f, (tmax - fmaf(tmin, 1.0f - 0x1p-20f, -1e-30f)) + 1e-30f, minTc - tmin), livef);
}
// the same value without the entry distance and the lane's participation (walk_bvh_packet_lx)
DEV float slab_cons_pk(float lx, float ly, float lz, float hx, float hy, float hz, const SlabCons& s, float minTc) {
    const float tx1 = fmaf(lx, s.ix, s.ax), tx2 = fmaf(hx, s.ix, s.bx);
    const float ty1 = fmaf(ly, s.iy, s.ay), ty2 = fmaf(hy, s.iy, s.by);
    const float tz1 = fmaf(lz, s.iz, s.az), tz2 = fmaf(hz, s.iz, s.bz);
    const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    return vmin3(tmax + 1e-30f, (tmax - fmaf(tmin, 1.0f - 0x1p-20f, -1e-30f)) + 1e-30f, minTc - tmin);
}

// The ordered closest walk's helpers (rtg_anyhit.hpp walk_closest_pk, k_hitfix in rtg_wave.hpp).
// wave minimum of a non-negative float (the lanes that do not take part hold +inf)
DEV float wave_min_pos(float v) {
    uint32_t u = __float_as_uint(v);
    for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)u, m);
        u = o < u ? o : u;
    }
    return __uint_as_float(u);
}
DEV float cull_limit(float t) { return t * (1.0f + 0x1p-20f); }   // inf stays inf
// Smallest float above a positive x (inf stays inf): "minT = next_up(t)" accepts t' <= t.
DEV float next_up(float x) { return x == INFINITY ? x : __uint_as_float(__float_as_uint(x) + 1u); }
DEV bool hit_less(float t, int k, int f, float bt, int bk, int bf) {
    return (t < bt) | ((t == bt) & ((k < bk) | ((k == bk) & (f < bf))));
}

}  // namespace rtg
