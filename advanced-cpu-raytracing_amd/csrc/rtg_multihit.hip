// Multi-hit ray queries (rtgpu.h rtg_trace_rays_multi*): the k nearest hits along caller rays,
// one ray per lane.
//
//   k_multihit<FEAT, KMAX>   IntersectObjects (raytracer.cpp:625-643) whose ray keeps the k smallest
//                            accepted distances instead of one: minT is the k-th of them (tmax while
//                            fewer are held), used wherever the reference uses minT -- box tests, group
//                            and instance world boxes, the moved-origin rule, t > 0 && t < minT at
//                            faces and spheres.  With k = 1 it is IntersectObjects.
//
// The object loop is trace<>'s per-lane path and the mesh walk walk_bvh_seq's stackless pre-order
// loop, with the same exact-decision tests (box_hit_fast, tri_test_sel, sphere_t's arithmetic), so
// the device decides as the host walk (host_query.cpp multi_one) does.  Leaves are always tested
// in order by their own lane, large ones (LEAF_EXT) too: the cooperative leaf reduction of
// walk_bvh keeps one survivor per leaf, and a hit list needs every accepted face in leaf order.
#include "rtg_walk.hpp"
#include "rtg_kernels.hpp"

namespace rtg {

static_assert(sizeof(rtg_ray) == 32 && sizeof(rtg_hit) == 16, "two 16-byte loads per ray, one 16-byte store per slot");
static_assert(RTG_MULTIHIT_MAX == 8, "multi_kmax's list ends at 8");

// The k nearest hits in ascending t, KMAX >= k slots per field.  Every index below is a constant
// once the loops are unrolled, so the fields are KMAX registers each, not a private array (a
// runtime-indexed one would live in scratch).  Slots >= k are never written.  Empty slots hold
// the miss record (tmax, -1, -1): an accepted hit has t < minT <= tmax, so it sorts before them.
template <int KMAX>
struct HitList {
    float t[KMAX];
    int obj[KMAX], face[KMAX];
};
template <int KMAX>
DEV void list_init(HitList<KMAX>& L, float tmax) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        L.t[j] = tmax;
        L.obj[j] = -1;
        L.face[j] = -1;
    }
}
// A compare-and-carry chain from slot 0 up: the new hit takes the first slot whose t it is
// strictly below, so it lands after every held hit of equal t (ties stable: first object, first
// face of the walk), and from there on every slot's hit moves up by one, whatever its t: a
// carried hit that ties with the next slot was found before it and stays before it (compared
// again, it would stay behind and be dropped in place of the later one).  What leaves slot
// k - 1 is dropped.  Returns the new minT, slot k - 1 (k is wave-uniform: scalar compares).
template <int KMAX>
DEV float list_insert(HitList<KMAX>& L, const int k, float t, int obj, int face) {
    float minT = L.t[0];
    bool placed = false;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
            const bool lt = placed | (t < L.t[j]);
            placed = lt;
            const float ct = L.t[j];
            const int co = L.obj[j], cf = L.face[j];
            L.t[j] = lt ? t : ct;
            L.obj[j] = lt ? obj : co;
            L.face[j] = lt ? face : cf;
            t = lt ? ct : t;
            obj = lt ? co : obj;
            face = lt ? cf : face;
            minT = L.t[j];
        }
    }
    return minT;
}

// walk_bvh_seq<false> (its select form, SEL) with the list in place of the single survivor
template <int KMAX>
DEV void walk_bvh_multi(const DevScene& S, int i, const int end, const Ray& r, HitList<KMAX>& L, const int k,
                        float& minT, const int obj) {
    const RayRcp q = ray_rcp(r);
    while (i < end) {
        const float4 a = S.nodes[2 * i];
        const float4 b = S.nodes[2 * i + 1];
        const int skip = __float_as_int(b.z);
        if (box_hit_fast<true>(a.x, a.y, a.z, a.w, b.x, b.y, r, q, minT)) {
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
                    if (tri_test_sel(S.tris + 3 * f, r, minT, t)) minT = list_insert(L, k, t, obj, f);
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

// Sphere::Intersect (sphere.cpp:13-70) with both roots: sphere_t's arithmetic and root selection;
// `sel` is the root the reference reports, `other` the one it leaves.  False: no real root.
DEV bool sphere_roots(const DevObject& ob, const Ray& lr, float& sel, float& other) {
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
    bool first = false;                      // the selected root is t1
    if (t1 < t2) first = t1 > 0.0f;
    else if (t2 < t1) first = !(t2 > 0.0f);
    sel = first ? t1 : t2;
    other = first ? t2 : t1;
    return true;
}

// Waves per SIMD (the register budget is 512 / waves), from the compiler's resource report
// (profiles/r13_multihit_resource_lines.txt): for the plain-mesh (FEAT 0) and FEAT_SPHERE variants
// the highest count without scratch --
//     KMAX       2            4            8
//     FEAT 0     7 (72 VGPRs) 6 (78)       4 (112)      one more: 16 / 24 / 76 B of scratch per lane
//     SPHERE     5 (92)       4 (116)      3 (164)      one more:  8 / 40 / 104 B
// (the list is 3 KMAX registers, and the sphere variants keep about as many again across the
// transform's double arithmetic).  The large-leaf, instance and transform variants keep their
// natural allocation, as RTG_TRACE_WAVES gives the closest-hit walk's: 72-164 VGPRs, nothing spilled.
constexpr int multi_waves(int feat, int kmax) {
    if (feat & ~FEAT_SPHERE) return 1;
    if (feat & FEAT_SPHERE) return kmax <= 2 ? 5 : kmax == 4 ? 4 : 3;
    return kmax <= 2 ? 7 : kmax == 4 ? 6 : 4;
}

template <int FEAT, int KMAX>
__global__ __launch_bounds__(256, multi_waves(FEAT, KMAX)) void k_multihit(
    const DevScene S, const float4* __restrict__ rays, const int n, const int k, int4* __restrict__ hits,
    int* __restrict__ counts) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 ra = rays[2 * (size_t)i], rb = rays[2 * (size_t)i + 1];
    Ray r;
    r.o = mk(ra.x, ra.y, ra.z);
    r.d = mk(rb.x, rb.y, rb.z);
    const float mbTime = rb.w;
    HitList<KMAX> L;
    list_init(L, ra.w);
    float minT = ra.w;
    // trace<>'s per-lane object loop (the comments there)
    const RayRcp rq = (FEAT & FEAT_INSTANCE) ? ray_rcp(r) : RayRcp{};
    for (int o = 0; o < S.num_objects; ++o) {
        const DevObject& ob = S.objects[o];
        if ((FEAT & FEAT_INSTANCE) && ob.group_end > o) {
            const float4 ga = S.group_box[2 * o], gb = S.group_box[2 * o + 1];
            if (!box_hit_fast(ga.x, ga.y, ga.z, gb.x, gb.y, gb.z, r, rq, minT)) {
                o = ob.group_end - 1;
                continue;
            }
        }
        if ((FEAT & FEAT_SPHERE) && ob.kind == OBJ_SPHERE) {
            const Ray lr = trav_ray(ob, r, mbTime);
            float t, u;
            if (sphere_roots(ob, lr, t, u)) {
                // the reference's root first (face -1), then the other if it differs (face -2),
                // each under t > 0 && t < minT
                if (t < minT && t > 0.0f) minT = list_insert(L, k, t, o, -1);
                if (u != t && u < minT && u > 0.0f) minT = list_insert(L, k, u, o, -2);
            }
            continue;
        }
        if ((FEAT & FEAT_INSTANCE) && ob.kind == OBJ_INSTANCE) {
            Ray wr = r;
            if (ob.flags & OBJF_MOTION_BLUR) wr.o = add(wr.o, muls(ld3(ob.mbv), mbTime));
            if (!box_hit_fast(ob.bmin[0], ob.bmin[1], ob.bmin[2], ob.bmax[0], ob.bmax[1], ob.bmax[2], wr, rq, minT)) {
                r.o = wr.o;
                continue;
            }
        }
        const Ray lr = (FEAT & FEAT_XFORM) ? trav_ray(ob, r, mbTime) : ident_ray(r);
        walk_bvh_multi(S, ob.node_begin, ob.node_end, lr, L, k, minT, o);
    }
    // ray-major, one 16-byte store per slot; slots >= k are the miss record and stay unwritten
    int cnt = 0;
    int4* out = hits + (size_t)i * (size_t)k;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
            out[j] = make_int4(__float_as_int(L.t[j]), L.obj[j], L.face[j], 0);
            cnt += L.obj[j] >= 0;
        }
    }
    if (counts) counts[i] = cnt;
}

hipError_t launch_multihit(const DevScene& S, int feat, const rtg_ray* rays, int n, int k, rtg_hit* hits, int* counts,
                           hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    return with_trav_feat(feat, [&](auto F) {
        return with_value<2, 4, 8>(multi_kmax(k), [&](auto K) {
            hipLaunchKernelGGL((k_multihit<decltype(F)::value, decltype(K)::value>), grid, block, 0, stream, S,
                               reinterpret_cast<const float4*>(rays), n, k, reinterpret_cast<int4*>(hits), counts);
            return hipGetLastError();
        });
    });
}

}  // namespace rtg
