// The closest-point walk (rtg_closest.hip k_closest, rtg_crossings.hip k_signed_distance): the held
// candidate, the point-to-box and point-to-triangle tests, the two passes over a mesh's nodes and
// the object loop of host_query.cpp closest_one.  The notes on arithmetic are rtg_closest.hip's.
#pragma once
#include "rtg_isect.hpp"
#include "rtg_pointxf.hpp"

namespace rtg {

// The held candidate (host_query.cpp Nearest): obj = -1 while nothing is held, below every
// candidate's, so the tie clause is false then; a NaN d2 fails both comparisons.
struct Nearest {
    float d2;
    int obj, face;
    f3 c;
};
DEV void offer(Nearest& B, float d2, int o, int f, f3 c) {
    const bool take = d2 < B.d2 || (d2 == B.d2 && (o < B.obj || (o == B.obj && f < B.face)));
    B.d2 = take ? d2 : B.d2;
    B.obj = take ? o : B.obj;
    B.face = take ? f : B.face;
    B.c.x = take ? c.x : B.c.x;
    B.c.y = take ? c.y : B.c.y;
    B.c.z = take ? c.z : B.c.z;
}

// rows as ((m0 x + m1 y) + m2 z) + m3; m is wave-uniform (scalar loads)
DEV f3 xf_point(const float* m, f3 v) {
    return mk(((m[0] * v.x + m[1] * v.y) + m[2] * v.z) + m[3], ((m[4] * v.x + m[5] * v.y) + m[6] * v.z) + m[7],
              ((m[8] * v.x + m[9] * v.y) + m[10] * v.z) + m[11]);
}
DEV f3 xf_vector(const float* m, f3 v) {
    return mk((m[0] * v.x + m[1] * v.y) + m[2] * v.z, (m[4] * v.x + m[5] * v.y) + m[6] * v.z,
              (m[8] * v.x + m[9] * v.y) + m[10] * v.z);
}

// squared distance from p to the box of node record (a, b); fmaxf drops a NaN operand
DEV float box_d2(const float4 a, const float4 b, f3 p) {
    const float ex = fmaxf(fmaxf(a.x - p.x, p.x - a.w), 0.f);
    const float ey = fmaxf(fmaxf(a.y - p.y, p.y - b.x), 0.f);
    const float ez = fmaxf(fmaxf(a.z - p.z, p.z - b.y), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}

// host_query.cpp tri_closest: the first region that holds of A, B, AB, C, AC, BC, else the
// interior; each region's one quotient through a single division
DEV float tri_closest(f3 a, f3 ab, f3 ac, f3 p, f3& c) {
    const f3 ap = sub(p, a);
    const f3 bp = sub(ap, ab);
    const f3 cp = sub(ap, ac);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    int reg = 6;
    reg = (va <= 0.f && e43 >= 0.f && e56 >= 0.f) ? 5 : reg;
    reg = (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) ? 4 : reg;
    reg = (d6 >= 0.f && d5 <= d6) ? 3 : reg;
    reg = (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) ? 2 : reg;
    reg = (d3 >= 0.f && d4 <= d3) ? 1 : reg;
    reg = (d1 <= 0.f && d2 <= 0.f) ? 0 : reg;
    const float num = reg == 2 ? d1 : reg == 4 ? d2 : reg == 5 ? e43 : 1.f;
    const float den = reg == 2 ? d1 - d3 : reg == 4 ? d2 - d6 : reg == 5 ? e43 + e56 : reg == 6 ? (va + vb) + vc : 1.f;
    const float q = num / den;
    const float v = reg == 1 ? 1.f : reg == 2 ? q : reg == 5 ? 1.f - q : reg == 6 ? vb * q : 0.f;
    const float w = reg == 3 ? 1.f : (reg == 4 || reg == 5) ? q : reg == 6 ? vc * q : 0.f;
    c = add(add(a, muls(ab, v)), muls(ac, w));
    const f3 d = sub(p, c);
    return dot(d, d);
}

// every face of the leaf at node i, in order (host_query.cpp closest_leaf)
template <bool XF>
DEV void closest_leaf(const DevScene& S, const PointXf& X, bool ident, int i, int leaf, f3 p, Nearest& B, int obj) {
    int first = leaf >> 8, cnt = leaf & 255;
    if (leaf == LEAF_EXT) {
        const int2 e = S.node_ext[i];
        first = e.x;
        cnt = e.y;
    }
    for (int f = first; f < first + cnt; ++f) {
        const float4 t0 = S.tris[3 * f], t1 = S.tris[3 * f + 1], t2 = S.tris[3 * f + 2];
        f3 a = mk(t0.x, t0.y, t0.z);
        f3 ab = mk(-t1.x, -t1.y, -t1.z);
        f3 ac = mk(-t2.x, -t2.y, -t2.z);
        if (XF && !ident) {
            a = xf_point(X.fwd, a);
            ab = xf_vector(X.fwd, ab);
            ac = xf_vector(X.fwd, ac);
        }
        f3 c;
        const float d2 = tri_closest(a, ab, ac, p, c);
        offer(B, d2, obj, f, c);
    }
}

// One mesh object's nodes [begin, end): p the world point, pl the point its boxes are tested against
template <bool XF>
DEV void walk_closest(const DevScene& S, const PointXf& X, bool ident, const int begin, const int end, f3 p, f3 pl,
                      float lip2, Nearest& B, int obj) {
    // pass 1: to the leaf whose boxes are nearer at every level; l = i + 1, r = skip(l); a tie, or
    // a false comparison, goes left
    int i = begin;
    int leaf = __float_as_int(S.nodes[2 * i + 1].w);
    while (leaf < 0) {
        const int l = i + 1;
        const float4 la = S.nodes[2 * l], lb = S.nodes[2 * l + 1];
        const int r = __float_as_int(lb.z);
        const float4 ra = S.nodes[2 * r], rb = S.nodes[2 * r + 1];
        const bool right = box_d2(ra, rb, pl) < box_d2(la, lb, pl);
        i = right ? r : l;
        leaf = __float_as_int(right ? rb.w : lb.w);
    }
    closest_leaf<XF>(S, X, ident, i, leaf, p, B, obj);
    // pass 2: walk_bvh_seq's loop, a node skipped iff its box is farther than the held distance
    i = begin;
    while (i < end) {
        const float4 a = S.nodes[2 * i];
        const float4 b = S.nodes[2 * i + 1];
        const int skip = __float_as_int(b.z);
        if (box_d2(a, b, pl) > B.d2 * lip2) {
            i = skip;
        } else {
            const int leaf = __float_as_int(b.w);
            if (leaf >= 0) {
                closest_leaf<XF>(S, X, ident, i, leaf, p, B, obj);
                i = skip;
            } else {
                i = i + 1;
            }
        }
    }
}

// The object loop (host_query.cpp closest_one): the nearest candidate of the scene within
// max_d2 = max_dist squared (obj = -1: none).  A point with a coordinate that is not finite meets
// no object.  The scene by value: by reference the sphere and transform variants of k_closest
// allocate 64 VGPRs instead of 62 / 63 (the same code otherwise).
template <int FEAT>
DEV Nearest closest_point(const DevScene S, const PointXf* xf, const f3 p, const float max_d2) {
    Nearest B;
    B.d2 = max_d2;
    B.obj = -1;
    B.face = -1;
    B.c = mk(0.f, 0.f, 0.f);
    constexpr bool XF = (FEAT & (FEAT_INSTANCE | FEAT_XFORM)) != 0;
    const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
    const int num = finite ? S.num_objects : 0;
    for (int o = 0; o < num; ++o) {
        const DevObject& ob = S.objects[o];
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            const PointXf& X = xf[o];
            f3 centre = mk(ob.center[0], ob.center[1], ob.center[2]);
            float radius = ob.center[3];
            if (!(X.flags & PXF_IDENTITY)) {
                centre = xf_point(X.fwd, centre);
                radius = radius * X.scale;
            }
            const f3 v = sub(p, centre);
            const float l = sqrtf(dot(v, v));
            const float dd = fabsf(l - radius);
            const f3 c = l == 0.f ? add(centre, mk(radius, 0.f, 0.f)) : add(centre, muls(v, radius / l));
            offer(B, dd * dd, o, -1, c);
            continue;
        }
        if (ob.node_end <= ob.node_begin) continue;
        const PointXf& X = xf[o];
        const bool ident = !XF || (X.flags & PXF_IDENTITY);
        const f3 pl = ident ? p : xf_point(X.inv, p);
        walk_closest<XF>(S, X, ident, ob.node_begin, ob.node_end, p, pl, ident ? 1.0f : X.lip2, B, o);
    }
    return B;
}

}  // namespace rtg
