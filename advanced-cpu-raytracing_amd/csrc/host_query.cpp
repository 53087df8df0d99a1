// rtg_desc_trace_rays: the reference's ray queries restated on the host over a scene
// description, with no device -- the yardstick the device queries (rtg_query.hip) are tested
// against bit for bit.  A plain restatement: true divisions, recursive BVH descent, sequential
// leaf loops, every float operation in the reference's order (this file is compiled with
// -ffp-contract=off like the rest of the host code).
//
//   IntersectObjects / CastShadowRay   raytracer.cpp:625-643, :585-623
//   BVH::IntersectBVH                  bvh.cpp:5-30
//   Mesh::Intersect / IntersectFace    mesh.cpp:158-240
//   Sphere::Intersect                  sphere.cpp:13-70
//   InstancedMesh::Intersect           instancedMesh.cpp:16-66
//   BoundingBox::doesIntersectWith     shape.hpp:78-100
//
// rtg_desc_trace_rays_multi: the same walk with the ray keeping its k smallest accepted distances
// (multi_one below) -- the same box_hit / face_hit and sphere arithmetic, minT the k-th distance.
//
// rtg_desc_closest_points: the nearest surface point to a point (closest_one below).  No reference
// code stands behind it: this walk is the definition that k_closest (rtg_closest.hip) repeats.
//
// rtg_desc_count_crossings: the multi-hit walk counting every accepted hit instead of keeping k
// (cross_one below); rtg_desc_signed_distance_points: closest_one, then cross_one from the point
// (signed_one).  Both define what k_crossings / k_signed_distance (rtg_crossings.hip) repeat.
#include "host_query.hpp"

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "host_math.hpp"
#include "rtg_pointxf.hpp"

namespace rtg {
namespace {

struct HRay {
    V3 o, d;
};

// matrix.hpp:56-81 on a row-major double[16]: double accumulation, narrowed to float
V3 xform(const double* m, const V3& v, float w) {
    return V3((float)(m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3] * w),
              (float)(m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7] * w),
              (float)(m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11] * w));
}

// BoundingBox::doesIntersectWith: the x slab by comparison, y / z by fmin / fmax
bool box_hit(const float* mn, const float* mx, const HRay& r, float minT) {
    float tx1 = (mn[0] - r.o.x) / r.d.x;
    float tx2 = (mx[0] - r.o.x) / r.d.x;
    float tmin = tx1, tmax = tx2;
    if (tx1 > tx2) { tmin = tx2; tmax = tx1; }
    float ty1 = (mn[1] - r.o.y) / r.d.y;
    float ty2 = (mx[1] - r.o.y) / r.d.y;
    tmin = std::fmax(tmin, std::fmin(ty1, ty2));
    tmax = std::fmin(tmax, std::fmax(ty1, ty2));
    float tz1 = (mn[2] - r.o.z) / r.d.z;
    float tz2 = (mx[2] - r.o.z) / r.d.z;
    tmin = std::fmax(tmin, std::fmin(tz1, tz2));
    tmax = std::fmin(tmax, std::fmax(tz1, tz2));
    return tmax > 0 && tmax >= tmin && tmin < minT;
}

// determinant (helperMath.cpp:132-138)
float det3(float m00, float m01, float m02, float m10, float m11, float m12, float m20, float m21, float m22) {
    float first = m00 * (m11 * m22 - m12 * m21);
    float second = m10 * (m02 * m21 - m01 * m22);
    float third = m20 * (m01 * m12 - m11 * m02);
    return first + second + third;
}

// Mesh::IntersectFace: Cramer's rule, the early outs in the reference's order
bool face_hit(const rtg_face& F, const HRay& r, float minT, float& tout) {
    const float e1x = F.v0.x - F.v1.x, e1y = F.v0.y - F.v1.y, e1z = F.v0.z - F.v1.z;
    const float e2x = F.v0.x - F.v2.x, e2y = F.v0.y - F.v2.y, e2z = F.v0.z - F.v2.z;
    const float dx = r.d.x, dy = r.d.y, dz = r.d.z;
    float detA = det3(e1x, e2x, dx, e1y, e2y, dy, e1z, e2z, dz);
    if (detA == 0) return false;
    const float sx = F.v0.x - r.o.x, sy = F.v0.y - r.o.y, sz = F.v0.z - r.o.z;
    float beta = det3(sx, e2x, dx, sy, e2y, dy, sz, e2z, dz) / detA;
    if (beta < 0) return false;
    float gama = det3(e1x, sx, dx, e1y, sy, dy, e1z, sz, dz) / detA;
    if (gama < 0 || gama + beta > 1) return false;
    float t = det3(e1x, e2x, sx, e1y, e2y, sy, e1z, e2z, sz) / detA;
    tout = t;
    return t > 0.0f && t < minT;
}

// Sphere::Intersect's root selection and acceptance on the local ray
bool sphere_hit(const rtg_object& ob, const HRay& lr, float minT, float& tout) {
    const V3 center = from_f3(ob.center);
    V3 oc = lr.o - center;
    float c = dot(oc, oc) - (ob.radius * ob.radius);
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

// the world ray in the object's local space (mesh.cpp:164-170, sphere.cpp:23-29,
// instancedMesh.cpp:33-39)
HRay local_ray(const rtg_object& ob, const HRay& r, float time) {
    HRay lr;
    lr.o = xform(ob.inv_transform, r.o, 1.0f);
    lr.d = xform(ob.inv_transform, r.d, 0.0f);
    if (ob.flags & RTG_OBJF_MOTION_BLUR) lr.o = lr.o + from_f3(ob.motion_blur) * time;
    return lr;
}

struct MeshWalk {
    const rtg_bvh_node* nodes;    // the mesh's nodes
    const rtg_face* faces;        // the mesh's faces (BVH order)
    HRay r;                       // local ray
    float minT;
    int face = -1;                // mesh-local index of the last accepted face
    bool any = false;             // stop at the first accepted face
    bool done = false;
};

// BVH::IntersectBVH
bool intersect_bvh(MeshWalk& w, int k) {
    const rtg_bvh_node& n = w.nodes[k];
    if (!box_hit(n.bmin, n.bmax, w.r, w.minT)) return false;
    bool hasHit = false;
    if (n.left < 0) {
        for (int i = n.first; i < n.first + n.count; ++i) {
            float t;
            if (face_hit(w.faces[i], w.r, w.minT, t)) {
                w.minT = t;
                w.face = i;
                hasHit = true;
                if (w.any) {
                    w.done = true;
                    return true;
                }
            }
        }
    } else {
        const bool hitLeft = intersect_bvh(w, n.left);
        if (w.done) return true;
        const bool hitRight = intersect_bvh(w, n.left + 1);
        hasHit = hitLeft || hitRight;
    }
    return hasHit;
}

// One ray through the object loop.  any: CastShadowRay with minT0 = limit = tmax -- every
// accepted hit has t < limit, so the first one answers; emissive meshes are skipped and the
// motion-blur time is 0.
void trace_one(const rtg_scene_desc* d, const rtg_ray& q, bool any, rtg_hit& out, float* normal) {
    HRay r;
    r.o = V3(q.ox, q.oy, q.oz);
    r.d = V3(q.dx, q.dy, q.dz);
    const float time = any ? 0.0f : q.time;
    float minT = q.tmax;
    int obj = -1, face = -1;
    V3 hitOrigin;                 // the world origin the accepted hit's object saw
    for (int k = 0; k < d->num_objects; ++k) {
        const rtg_object& ob = d->objects[k];
        if (ob.kind == RTG_OBJ_SPHERE) {
            float t;
            if (sphere_hit(ob, local_ray(ob, r, time), minT, t)) {
                minT = t; obj = k; face = -1; hitOrigin = r.o;
                if (any) break;
            }
            continue;
        }
        if (any && (ob.flags & RTG_OBJF_SHADOW_SKIP)) continue;
        const rtg_mesh& M = d->meshes[ob.mesh];
        if (ob.kind == RTG_OBJ_INSTANCE) {
            // the world box first, on the blurred origin; a miss leaves the offset on the ray
            // (instancedMesh.cpp:23-29: the origin is restored only inside the branch)
            HRay wr = r;
            if (ob.flags & RTG_OBJF_MOTION_BLUR) wr.o = wr.o + from_f3(ob.motion_blur) * time;
            if (!box_hit(ob.bbox_min, ob.bbox_max, wr, minT)) {
                r.o = wr.o;
                continue;
            }
        }
        MeshWalk w;
        w.nodes = d->nodes + M.node_offset;
        w.faces = d->faces + M.face_offset;
        w.r = local_ray(ob, r, time);
        w.minT = minT;
        w.any = any;
        // Mesh::Intersect tests the mesh's own box before its BVH (mesh.cpp:172)
        if (ob.kind == RTG_OBJ_MESH && !box_hit(ob.bbox_min, ob.bbox_max, w.r, minT)) continue;
        if (M.node_count <= 0) continue;
        if (intersect_bvh(w, 0)) {
            minT = w.minT; obj = k; face = M.face_offset + w.face; hitOrigin = r.o;
            if (any) break;
        }
    }
    out.t = minT;
    out.object = any ? (obj >= 0 ? 0 : -1) : obj;
    out.face = any ? -1 : face;
    out.pad = 0;
    if (!normal || any) return;
    normal[0] = normal[1] = normal[2] = normal[3] = 0.f;
    if (obj < 0) return;
    const rtg_object& ob = d->objects[obj];
    V3 n;
    if (face < 0) {               // sphere.cpp:66,84 and the normal's transform
        HRay hr;
        hr.o = hitOrigin;
        hr.d = r.d;
        const HRay lr = local_ray(ob, hr, time);
        const V3 lp = lr.o + lr.d * minT;
        n = makeUnit(lp - from_f3(ob.center));
    } else {                      // mesh.cpp:241, :362-364, :179 / instancedMesh.cpp:57
        n = from_f3(d->faces[face].n);
        if (ob.flags & RTG_OBJF_NORMAL_TWICE) n = makeUnit(xform(ob.base_inv_transpose, n, 0.0f));
    }
    n = makeUnit(xform(ob.inv_transpose, n, 0.0f));
    normal[0] = n.x; normal[1] = n.y; normal[2] = n.z;
}

// ---- multi-hit: the same walk keeping the k smallest accepted distances (rtg_desc_trace_rays_multi)

// The held hits in ascending t.  minT is the k-th distance, or tmax while fewer are held.
struct HitList {
    int k;
    float tmax;
    int n = 0;
    float t[RTG_MULTIHIT_MAX];
    int obj[RTG_MULTIHIT_MAX], face[RTG_MULTIHIT_MAX];
    float minT() const { return n < k ? tmax : t[k - 1]; }
    // an accepted hit (tn < minT): after every held hit of equal t; the last falls off a full list
    void insert(float tn, int o, int f) {
        int j = n < k ? n++ : k - 1;
        for (; j > 0 && tn < t[j - 1]; --j) {
            t[j] = t[j - 1]; obj[j] = obj[j - 1]; face[j] = face[j - 1];
        }
        t[j] = tn; obj[j] = o; face[j] = f;
    }
};

// Sphere::Intersect with both roots: sphere_hit's arithmetic and selection; `sel` is the root the
// reference reports, `other` the one it leaves.  False: no real root.
bool sphere_roots(const rtg_object& ob, const HRay& lr, float& sel, float& other) {
    const V3 center = from_f3(ob.center);
    V3 oc = lr.o - center;
    float c = dot(oc, oc) - (ob.radius * ob.radius);
    float b = 2 * dot(lr.d, oc);
    float a = dot(lr.d, lr.d);
    float delta = b * b - (4 * a * c);
    if (delta < 0.0f) return false;
    delta = sqrtf(delta);
    a = (float)(2.0 * a);
    float t1 = (-b + delta) / a;
    float t2 = (-b - delta) / a;
    sel = t2; other = t1;                                          // t1 == t2, or unordered
    if (t1 < t2) { if (t1 > 0.0f) { sel = t1; other = t2; } }      // else t2, as above
    else if (t2 < t1) { if (!(t2 > 0.0f)) { sel = t1; other = t2; } }
    return true;
}

struct MultiWalk {
    const rtg_bvh_node* nodes;
    const rtg_face* faces;
    HRay r;                       // local ray
    HitList* L;
    int obj, face_offset;
};

// BVH::IntersectBVH, every accepted face into the list
void intersect_bvh_multi(MultiWalk& w, int k) {
    const rtg_bvh_node& n = w.nodes[k];
    if (!box_hit(n.bmin, n.bmax, w.r, w.L->minT())) return;
    if (n.left < 0) {
        for (int i = n.first; i < n.first + n.count; ++i) {
            float t;
            if (face_hit(w.faces[i], w.r, w.L->minT(), t)) w.L->insert(t, w.obj, w.face_offset + i);
        }
    } else {
        intersect_bvh_multi(w, n.left);
        intersect_bvh_multi(w, n.left + 1);
    }
}

// trace_one's object loop (closest hit) on a list
void multi_one(const rtg_scene_desc* d, const rtg_ray& q, int kk, rtg_hit* out, int32_t* count) {
    HRay r;
    r.o = V3(q.ox, q.oy, q.oz);
    r.d = V3(q.dx, q.dy, q.dz);
    const float time = q.time;
    HitList L;
    L.k = kk;
    L.tmax = q.tmax;
    for (int k = 0; k < d->num_objects; ++k) {
        const rtg_object& ob = d->objects[k];
        if (ob.kind == RTG_OBJ_SPHERE) {
            float t, u;
            if (sphere_roots(ob, local_ray(ob, r, time), t, u)) {
                if (t < L.minT() && t > 0.0f) L.insert(t, k, -1);
                if (u != t && u < L.minT() && u > 0.0f) L.insert(u, k, -2);
            }
            continue;
        }
        const rtg_mesh& M = d->meshes[ob.mesh];
        if (ob.kind == RTG_OBJ_INSTANCE) {
            HRay wr = r;
            if (ob.flags & RTG_OBJF_MOTION_BLUR) wr.o = wr.o + from_f3(ob.motion_blur) * time;
            if (!box_hit(ob.bbox_min, ob.bbox_max, wr, L.minT())) {
                r.o = wr.o;
                continue;
            }
        }
        MultiWalk w;
        w.nodes = d->nodes + M.node_offset;
        w.faces = d->faces + M.face_offset;
        w.r = local_ray(ob, r, time);
        w.L = &L;
        w.obj = k;
        w.face_offset = M.face_offset;
        if (ob.kind == RTG_OBJ_MESH && !box_hit(ob.bbox_min, ob.bbox_max, w.r, L.minT())) continue;
        if (M.node_count <= 0) continue;
        intersect_bvh_multi(w, 0);
    }
    for (int j = 0; j < kk; ++j) {
        const bool filled = j < L.n;
        out[j].t = filled ? L.t[j] : q.tmax;
        out[j].object = filled ? L.obj[j] : -1;
        out[j].face = filled ? L.face[j] : -1;
        out[j].pad = 0;
    }
    if (count) *count = L.n;
}

// ---- crossing counts (rtg_desc_count_crossings): multi_one's walk with nothing kept, so minT is
// tmax from start to end and every accepted hit is counted.  No reference code: this walk is the
// definition that k_crossings (rtg_crossings.hip) repeats.

struct CrossWalk {
    const rtg_bvh_node* nodes;
    const rtg_face* faces;
    HRay r;                       // local ray
    float tmax;
    rtg_crossings* C;
};

// BVH::IntersectBVH, every accepted face counted; it enters where the local ray goes against
// the face's normal
void intersect_bvh_cross(CrossWalk& w, int k) {
    const rtg_bvh_node& n = w.nodes[k];
    if (!box_hit(n.bmin, n.bmax, w.r, w.tmax)) return;
    if (n.left < 0) {
        for (int i = n.first; i < n.first + n.count; ++i) {
            float t;
            if (face_hit(w.faces[i], w.r, w.tmax, t)) {
                w.C->count += 1;
                if (dot(w.r.d, from_f3(w.faces[i].n)) < 0.0f) w.C->entering += 1;
            }
        }
    } else {
        intersect_bvh_cross(w, n.left);
        intersect_bvh_cross(w, n.left + 1);
    }
}

// Sphere::Intersect's two roots, sphere_hit's arithmetic: `in` = (-b - delta) / a, where the ray
// enters, `out` the other.  False: no real root.
bool sphere_in_out(const rtg_object& ob, const HRay& lr, float& in, float& out) {
    const V3 center = from_f3(ob.center);
    V3 oc = lr.o - center;
    float c = dot(oc, oc) - (ob.radius * ob.radius);
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

// multi_one's object loop on two counters
void cross_one(const rtg_scene_desc* d, const rtg_ray& q, rtg_crossings& C) {
    HRay r;
    r.o = V3(q.ox, q.oy, q.oz);
    r.d = V3(q.dx, q.dy, q.dz);
    const float time = q.time, tmax = q.tmax;
    C.count = 0;
    C.entering = 0;
    for (int k = 0; k < d->num_objects; ++k) {
        const rtg_object& ob = d->objects[k];
        if (ob.kind == RTG_OBJ_SPHERE) {
            // multi_one takes the selected root, then the other if it differs, each under
            // t > 0 && t < minT: with minT fixed that is each distinct root under the same test
            float in, out;
            if (sphere_in_out(ob, local_ray(ob, r, time), in, out)) {
                if (in < tmax && in > 0.0f) { C.count += 1; C.entering += 1; }
                if (out != in && out < tmax && out > 0.0f) C.count += 1;
            }
            continue;
        }
        const rtg_mesh& M = d->meshes[ob.mesh];
        if (ob.kind == RTG_OBJ_INSTANCE) {
            HRay wr = r;
            if (ob.flags & RTG_OBJF_MOTION_BLUR) wr.o = wr.o + from_f3(ob.motion_blur) * time;
            if (!box_hit(ob.bbox_min, ob.bbox_max, wr, tmax)) {
                r.o = wr.o;
                continue;
            }
        }
        CrossWalk w;
        w.nodes = d->nodes + M.node_offset;
        w.faces = d->faces + M.face_offset;
        w.r = local_ray(ob, r, time);
        w.tmax = tmax;
        w.C = &C;
        if (ob.kind == RTG_OBJ_MESH && !box_hit(ob.bbox_min, ob.bbox_max, w.r, tmax)) continue;
        if (M.node_count <= 0) continue;
        intersect_bvh_cross(w, 0);
    }
}

// ---- closest-point queries (rtg_desc_closest_points): the nearest surface point to a point.
// No ray and no reference code: rtgpu.h states the semantics, this walk defines them operation by
// operation, and k_closest (rtg_closest.hip) repeats its decisions with the same arithmetic.

// The held candidate.  Everything is compared on the squared distance; among equal ones the
// lexicographically smaller (object, face) stays.  With nothing held obj is -1, below every
// candidate's, so only d2 < best accepts; a NaN d2 fails both comparisons.
struct Nearest {
    float d2;
    int obj = -1, face = -1;
    V3 c;
    void offer(float nd2, int o, int f, const V3& nc) {
        if (nd2 < d2 || (nd2 == d2 && (o < obj || (o == obj && f < face)))) {
            d2 = nd2; obj = o; face = f; c = nc;
        }
    }
};

V3 xf_point(const float* m, const V3& v) {
    return V3(((m[0] * v.x + m[1] * v.y) + m[2] * v.z) + m[3], ((m[4] * v.x + m[5] * v.y) + m[6] * v.z) + m[7],
              ((m[8] * v.x + m[9] * v.y) + m[10] * v.z) + m[11]);
}
V3 xf_vector(const float* m, const V3& v) {
    return V3((m[0] * v.x + m[1] * v.y) + m[2] * v.z, (m[4] * v.x + m[5] * v.y) + m[6] * v.z,
              (m[8] * v.x + m[9] * v.y) + m[10] * v.z);
}

// squared distance from p to the box; fmaxf drops a NaN operand
float box_d2(const float* mn, const float* mx, const V3& p) {
    const float ex = fmaxf(fmaxf(mn[0] - p.x, p.x - mx[0]), 0.f);
    const float ey = fmaxf(fmaxf(mn[1] - p.y, p.y - mx[1]), 0.f);
    const float ez = fmaxf(fmaxf(mn[2] - p.z, p.z - mx[2]), 0.f);
    return (ex * ex + ey * ey) + ez * ez;
}

// Closest point of the triangle (a, a + ab, a + ac) to p by its Voronoi regions (Ericson,
// Real-Time Collision Detection 5.1.5), regions in the order A, B, AB, C, AC, BC, interior;
// c = a + ab v + ac w.  Returns the squared distance.
float tri_closest(const V3& a, const V3& ab, const V3& ac, const V3& p, V3& c) {
    const V3 ap = p - a;
    const V3 bp = ap - ab;
    const V3 cp = ap - ac;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    float v, w;
    if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }
    else if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = d1 / (d1 - d3); w = 0.f; }
    else if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }
    else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = d2 / (d2 - d6); }
    else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.f - w;
    } else {
        const float den = 1.f / ((va + vb) + vc);
        v = vb * den;
        w = vc * den;
    }
    c = (a + ab * v) + ac * w;
    const V3 d = p - c;
    return dot(d, d);
}

struct PointWalk {
    const rtg_bvh_node* nodes;
    const rtg_face* faces;
    const PointXf* X;
    V3 p, pl;                     // the world point; the point the boxes are tested against
    Nearest* best;
    int obj, face_offset;
};

// every face of a leaf, in order: the walk record's {v0, v0 - v1, v0 - v2} (the differences
// formed in float first, as face_tables / k_write_faces store them), carried to world space
void closest_leaf(PointWalk& w, const rtg_bvh_node& n) {
    for (int i = n.first; i < n.first + n.count; ++i) {
        const rtg_face& F = w.faces[i];
        V3 a = from_f3(F.v0);
        const float e1x = F.v0.x - F.v1.x, e1y = F.v0.y - F.v1.y, e1z = F.v0.z - F.v1.z;
        const float e2x = F.v0.x - F.v2.x, e2y = F.v0.y - F.v2.y, e2z = F.v0.z - F.v2.z;
        V3 ab(-e1x, -e1y, -e1z), ac(-e2x, -e2y, -e2z);
        if (!(w.X->flags & PXF_IDENTITY)) {
            a = xf_point(w.X->fwd, a);
            ab = xf_vector(w.X->fwd, ab);
            ac = xf_vector(w.X->fwd, ac);
        }
        V3 c;
        const float d2 = tri_closest(a, ab, ac, w.p, c);
        w.best->offer(d2, w.obj, w.face_offset + i, c);
    }
}

// pass 2: the pre-order walk, a node skipped iff its box is farther than the held distance
// (local d2 <= lip2 * world d2); a false comparison descends
void closest_bvh(PointWalk& w, int k) {
    const rtg_bvh_node& n = w.nodes[k];
    if (box_d2(n.bmin, n.bmax, w.pl) > w.best->d2 * w.X->lip2) return;
    if (n.left < 0) {
        closest_leaf(w, n);
    } else {
        closest_bvh(w, n.left);
        closest_bvh(w, n.left + 1);
    }
}

void closest_one(const rtg_scene_desc* d, const PointXf* xf, const rtg_point& q, rtg_nearest& out) {
    const V3 p(q.x, q.y, q.z);
    Nearest best;
    best.d2 = q.max_dist * q.max_dist;
    const bool finite = fabsf(q.x) < INFINITY && fabsf(q.y) < INFINITY && fabsf(q.z) < INFINITY;
    for (int k = 0; finite && k < d->num_objects; ++k) {
        const rtg_object& ob = d->objects[k];
        const PointXf& X = xf[k];
        if (ob.kind == RTG_OBJ_SPHERE) {
            V3 centre = from_f3(ob.center);
            float radius = ob.radius;
            if (!(X.flags & PXF_IDENTITY)) {
                centre = xf_point(X.fwd, centre);
                radius = radius * X.scale;
            }
            const V3 v = p - centre;
            const float l = sqrtf(dot(v, v));
            const float dd = fabsf(l - radius);
            const V3 c = l == 0.f ? centre + V3(radius, 0.f, 0.f) : centre + v * (radius / l);
            best.offer(dd * dd, k, -1, c);
            continue;
        }
        const rtg_mesh& M = d->meshes[ob.mesh];
        if (M.node_count <= 0) continue;
        PointWalk w;
        w.nodes = d->nodes + M.node_offset;
        w.faces = d->faces + M.face_offset;
        w.X = &X;
        w.p = p;
        w.pl = (X.flags & PXF_IDENTITY) ? p : xf_point(X.inv, p);
        w.best = &best;
        w.obj = k;
        w.face_offset = M.face_offset;
        // pass 1: descend to the leaf whose boxes are nearer at every level (a tie, or a false
        // comparison, goes left), for a tight bound before the pruned walk (without it an
        // unbounded query tests faces in pre-order until it happens on a near one: DESIGN.md 5)
        int i = 0;
        while (w.nodes[i].left >= 0) {
            const rtg_bvh_node& l = w.nodes[w.nodes[i].left];
            const rtg_bvh_node& r = w.nodes[w.nodes[i].left + 1];
            i = box_d2(r.bmin, r.bmax, w.pl) < box_d2(l.bmin, l.bmax, w.pl) ? w.nodes[i].left + 1 : w.nodes[i].left;
        }
        closest_leaf(w, w.nodes[i]);
        closest_bvh(w, 0);
    }
    const bool hit = best.obj >= 0;
    out.dist = hit ? sqrtf(best.d2) : q.max_dist;
    out.object = best.obj;
    out.face = best.face;
    out.pad0 = 0;
    out.px = hit ? best.c.x : 0.f;
    out.py = hit ? best.c.y : 0.f;
    out.pz = hit ? best.c.z : 0.f;
    out.pad1 = 0.f;
}

// rtg_desc_signed_distance_points: closest_one, then cross_one from the point along dir (unbounded,
// time 0); the count into pad0, an odd one onto a hit's sign bit.  A point that is not finite
// walks nothing.
void signed_one(const rtg_scene_desc* d, const PointXf* xf, const rtg_point& q, const float* dir, rtg_nearest& out) {
    closest_one(d, xf, q, out);
    const bool finite = fabsf(q.x) < INFINITY && fabsf(q.y) < INFINITY && fabsf(q.z) < INFINITY;
    if (!finite) return;
    const rtg_ray ray = {q.x, q.y, q.z, INFINITY, dir[0], dir[1], dir[2], 0.0f};
    rtg_crossings C;
    cross_one(d, ray, C);
    out.pad0 = C.count;
    if (out.object >= 0 && (C.count & 1)) out.dist = -out.dist;
}

// fn(begin, end) over [0, n) in contiguous chunks on a few threads: rays are independent
template <typename Fn>
void chunked(int64_t n, Fn&& work) {
    const int64_t kChunk = 4096;
    const int nt = (int)std::min<int64_t>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())),
                                          (n + kChunk - 1) / kChunk);
    if (nt <= 1) {
        work(0, n);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        const int64_t b = t * per, e = std::min(n, b + per);
        if (b < e) pool.emplace_back(work, b, e);
    }
    for (auto& th : pool) th.join();
}

const char* check_desc(const rtg_scene_desc* d) {
    if (d->num_faces > 0 && d->num_nodes == 0)
        return "the description has no BVH nodes (RTG_LOAD_DEVICE_BVH): it is for rtg_scene_create only";
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        if (o.kind != RTG_OBJ_SPHERE && (o.mesh < 0 || o.mesh >= d->num_meshes)) return "object with a bad mesh index";
    }
    return nullptr;
}

}  // namespace

int host_trace_rays_multi(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags,
                          rtg_hit* hits, int32_t* counts, std::string& err) {
    if (!d) { err = "null description"; return RTG_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { err = "ray count out of range"; return RTG_ERR_INVALID; }
    if (k < 1 || k > RTG_MULTIHIT_MAX) { err = "k out of range [1, RTG_MULTIHIT_MAX]"; return RTG_ERR_INVALID; }
    if (flags & RTG_QUERY_ANY_HIT) { err = "RTG_QUERY_ANY_HIT does not apply to a multi-hit query"; return RTG_ERR_INVALID; }
    if (flags & ~(uint32_t)RTG_QUERY_COHERENT) { err = "unknown query flags"; return RTG_ERR_INVALID; }
    if (const char* e = check_desc(d)) { err = e; return RTG_ERR_INVALID; }
    if (n == 0) return RTG_OK;
    if (!rays || !hits) { err = "null buffer"; return RTG_ERR_INVALID; }
    chunked(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) multi_one(d, rays[i], k, hits + i * k, counts ? counts + i : nullptr);
    });
    return RTG_OK;
}

int closest_unsupported(const PointXf* xf, int num_objects, std::string& err) {
    for (int i = 0; i < num_objects; ++i)
        if (!(xf[i].flags & PXF_SPHERE_OK)) {
            err = "object " + std::to_string(i) + ": a sphere under a transform that is not a similarity is an "
                  "ellipsoid, which closest-point queries do not handle";
            return RTG_ERR_UNSUPPORTED;
        }
    return RTG_OK;
}

int host_closest_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, uint32_t flags, rtg_nearest* out,
                        std::string& err) {
    if (!d) { err = "null description"; return RTG_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { err = "point count out of range"; return RTG_ERR_INVALID; }
    if (flags) { err = "unknown query flags"; return RTG_ERR_INVALID; }
    if (const char* e = check_desc(d)) { err = e; return RTG_ERR_INVALID; }
    if (n > 0 && (!points || !out)) { err = "null buffer"; return RTG_ERR_INVALID; }
    std::vector<PointXf> xf((size_t)d->num_objects);
    for (int i = 0; i < d->num_objects; ++i) point_xf_record(d->objects[i], xf[i]);
    if (int rc = closest_unsupported(xf.data(), d->num_objects, err)) return rc;
    chunked(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) closest_one(d, xf.data(), points[i], out[i]);
    });
    return RTG_OK;
}

int host_count_crossings(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_crossings* out,
                         std::string& err) {
    if (!d) { err = "null description"; return RTG_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { err = "ray count out of range"; return RTG_ERR_INVALID; }
    if (flags & RTG_QUERY_ANY_HIT) { err = "RTG_QUERY_ANY_HIT does not apply to a crossing count"; return RTG_ERR_INVALID; }
    if (flags & ~(uint32_t)RTG_QUERY_COHERENT) { err = "unknown query flags"; return RTG_ERR_INVALID; }
    if (const char* e = check_desc(d)) { err = e; return RTG_ERR_INVALID; }
    if (n == 0) return RTG_OK;
    if (!rays || !out) { err = "null buffer"; return RTG_ERR_INVALID; }
    chunked(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) cross_one(d, rays[i], out[i]);
    });
    return RTG_OK;
}

const char* signed_distance_dir(const float* dir, float out[3]) {
    static const float kDefault[3] = {0.8213f, 0.4402f, 0.3628f};
    const float* v = dir ? dir : kDefault;
    for (int j = 0; j < 3; ++j) {
        if (!(fabsf(v[j]) < INFINITY)) return "dir is not finite";
        out[j] = v[j];
    }
    if (v[0] == 0.f && v[1] == 0.f && v[2] == 0.f) return "dir is all zero";
    return nullptr;
}

int host_signed_distance_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, const float* dir,
                                uint32_t flags, rtg_nearest* out, std::string& err) {
    if (!d) { err = "null description"; return RTG_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { err = "point count out of range"; return RTG_ERR_INVALID; }
    if (flags) { err = "unknown query flags"; return RTG_ERR_INVALID; }
    if (const char* e = check_desc(d)) { err = e; return RTG_ERR_INVALID; }
    if (n > 0 && (!points || !out)) { err = "null buffer"; return RTG_ERR_INVALID; }
    float v[3];
    if (const char* e = signed_distance_dir(dir, v)) { err = e; return RTG_ERR_INVALID; }
    std::vector<PointXf> xf((size_t)d->num_objects);
    for (int i = 0; i < d->num_objects; ++i) point_xf_record(d->objects[i], xf[i]);
    if (int rc = closest_unsupported(xf.data(), d->num_objects, err)) return rc;
    chunked(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) signed_one(d, xf.data(), points[i], v, out[i]);
    });
    return RTG_OK;
}

int host_trace_rays(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_hit* hits,
                    float* normals, std::string& err) {
    if (!d) { err = "null description"; return RTG_ERR_INVALID; }
    if (n < 0 || n > INT32_MAX) { err = "ray count out of range"; return RTG_ERR_INVALID; }
    if (flags & ~(uint32_t)(RTG_QUERY_ANY_HIT | RTG_QUERY_COHERENT)) { err = "unknown query flags"; return RTG_ERR_INVALID; }
    if (d->num_faces > 0 && d->num_nodes == 0) {
        err = "the description has no BVH nodes (RTG_LOAD_DEVICE_BVH): it is for rtg_scene_create only";
        return RTG_ERR_INVALID;
    }
    if (n == 0) return RTG_OK;
    if (!rays || !hits) { err = "null buffer"; return RTG_ERR_INVALID; }
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        if (o.kind != RTG_OBJ_SPHERE && (o.mesh < 0 || o.mesh >= d->num_meshes)) {
            err = "object with a bad mesh index";
            return RTG_ERR_INVALID;
        }
    }
    const bool any = (flags & RTG_QUERY_ANY_HIT) != 0;
    chunked(n, [&](int64_t b, int64_t e) {
        for (int64_t i = b; i < e; ++i) trace_one(d, rays[i], any, hits[i], normals ? normals + 4 * i : nullptr);
    });
    return RTG_OK;
}

}  // namespace rtg
