// The crossing walk (rtg_crossings.hip k_crossings, k_signed_distance): k_multihit's walk with two
// counters in place of the hit list.  Nothing is kept, so minT is tmax from start to end and every
// accepted hit counts (host_query.cpp cross_one defines it; the same exact-decision tests --
// box_hit_fast, tri_test_sel, sphere_t's arithmetic -- so the device decides as the host does).
#pragma once
#include "rtg_walk.hpp"

namespace rtg {

// accepted hits, and those of them at which the ray goes against the geometric normal
struct Crossings {
    int count, entering;
};

// walk_bvh_multi (rtg_multihit.hip) counting: leaves in order by their own lane, large ones
// (LEAF_EXT) too; a face enters where the local ray goes against its normal (face_n, read per hit)
DEV void walk_bvh_cross(const DevScene& S, int i, const int end, const Ray& r, const float tmax, Crossings& C) {
    const RayRcp q = ray_rcp(r);
    while (i < end) {
        const float4 a = S.nodes[2 * i];
        const float4 b = S.nodes[2 * i + 1];
        const int skip = __float_as_int(b.z);
        if (box_hit_fast<true>(a.x, a.y, a.z, a.w, b.x, b.y, r, q, tmax)) {
            const int leaf = __float_as_int(b.w);
            if (leaf >= 0) {
                int first = leaf >> 8, cnt = leaf & 255;
                if (leaf == LEAF_EXT) {
                    const int2 e = S.node_ext[i];
                    first = e.x;
                    cnt = e.y;
                }
                for (int f = first; f < first + cnt; ++f) {
                    float t;
                    if (tri_test_sel(S.tris + 3 * f, r, tmax, t)) {
                        const float4 n = S.face_n[f];
                        C.count += 1;
                        C.entering += dot(r.d, mk(n.x, n.y, n.z)) < 0.0f;
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
}

// Sphere::Intersect's two roots (sphere.cpp:13-70, sphere_t's arithmetic): `in` = (-b - delta) / a,
// where the ray enters, `out` the other.  False: no real root.
DEV bool sphere_in_out(const DevObject& ob, const Ray& lr, float& in, float& out) {
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
    out = (-b + delta) / a;
    in = (-b - delta) / a;
    return true;
}

// k_multihit's object loop (trace<>'s per-lane path; the comments there) on two counters.  The
// ray by value: a missed motion-blurred instance moves its origin.
template <int FEAT>
DEV Crossings count_crossings(const DevScene& S, Ray r, const float mbTime, const float tmax) {
    Crossings C{0, 0};
    const RayRcp rq = (FEAT & FEAT_INSTANCE) ? ray_rcp(r) : RayRcp{};
    for (int o = 0; o < S.num_objects; ++o) {
        const DevObject& ob = S.objects[o];
        if ((FEAT & FEAT_INSTANCE) && ob.group_end > o) {
            const float4 ga = S.group_box[2 * o], gb = S.group_box[2 * o + 1];
            if (!box_hit_fast(ga.x, ga.y, ga.z, gb.x, gb.y, gb.z, r, rq, tmax)) {
                o = ob.group_end - 1;
                continue;
            }
        }
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            const Ray lr = trav_ray(ob, r, mbTime);
            float in, out;
            if (sphere_in_out(ob, lr, in, out)) {
                // each distinct root under t > 0 && t < tmax; a double root once, as entering
                const bool ci = in < tmax && in > 0.0f;
                const bool co = out != in && out < tmax && out > 0.0f;
                C.count += (int)ci + (int)co;
                C.entering += (int)ci;
            }
            continue;
        }
        if ((FEAT & FEAT_INSTANCE) && ob.kind == OBJ_INSTANCE) {
            Ray wr = r;
            if (ob.flags & OBJF_MOTION_BLUR) wr.o = add(wr.o, muls(ld3(ob.mbv), mbTime));
            if (!box_hit_fast(ob.bmin[0], ob.bmin[1], ob.bmin[2], ob.bmax[0], ob.bmax[1], ob.bmax[2], wr, rq, tmax)) {
                r.o = wr.o;
                continue;
            }
        }
        const Ray lr = (FEAT & FEAT_XFORM) ? trav_ray(ob, r, mbTime) : ident_ray(r);
        walk_bvh_cross(S, ob.node_begin, ob.node_end, lr, tmax, C);
    }
    return C;
}

}  // namespace rtg
