// Description -> kernel tables (scene_tables.hpp): host arithmetic only.
#include "scene_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "rtg_variants.hpp"   // max_supported_depth

namespace rtg {
namespace {

int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// Ken Perlin's reference permutation ("Improving Noise", SIGGRAPH 2002), duplicated to
// 512 entries, and the 12 cube-edge gradients -- the tables perlinTexture.cpp:5-37 uses.
const int kPerm256[256] = {
    151, 160, 137, 91,  90,  15,  131, 13,  201, 95,  96,  53,  194, 233, 7,   225, 140, 36,  103, 30,  69,  142,
    8,   99,  37,  240, 21,  10,  23,  190, 6,   148, 247, 120, 234, 75,  0,   26,  197, 62,  94,  252, 219, 203,
    117, 35,  11,  32,  57,  177, 33,  88,  237, 149, 56,  87,  174, 20,  125, 136, 171, 168, 68,  175, 74,  165,
    71,  134, 139, 48,  27,  166, 77,  146, 158, 231, 83,  111, 229, 122, 60,  211, 133, 230, 220, 105, 92,  41,
    55,  46,  245, 40,  244, 102, 143, 54,  65,  25,  63,  161, 1,   216, 80,  73,  209, 76,  132, 187, 208, 89,
    18,  169, 200, 196, 135, 130, 116, 188, 159, 86,  164, 100, 109, 198, 173, 186, 3,   64,  52,  217, 226, 250,
    124, 123, 5,   202, 38,  147, 118, 126, 255, 82,  85,  212, 207, 206, 59,  227, 47,  16,  58,  17,  182, 189,
    28,  42,  223, 183, 170, 213, 119, 248, 152, 2,   44,  154, 163, 70,  221, 153, 101, 155, 167, 43,  172, 9,
    129, 22,  39,  253, 19,  98,  108, 110, 79,  113, 224, 232, 178, 185, 112, 104, 218, 246, 97,  228, 251, 34,
    242, 193, 238, 210, 144, 12,  191, 179, 162, 241, 81,  51,  145, 235, 249, 14,  239, 107, 49,  192, 214, 31,
    181, 199, 106, 157, 184, 84,  204, 176, 115, 121, 50,  45,  127, 4,   150, 254, 138, 236, 205, 93,  222, 114,
    67,  29,  24,  72,  243, 141, 128, 195, 78,  66,  215, 61,  156, 180};
const float kGrad[36] = {1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1, 0, 1, 0, 1, -1, 0, 1,
                         1, 0, -1, -1, 0, -1, 0, 1, 1, 0, -1, 1, 0, 1, -1, 0, -1, -1};

void f4(float* dst, const rtg_float3& v, float w = 0.f) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = w; }

// Pre-order (left subtree first) of one mesh's BVH as the description carries it; false when a
// child index leaves the mesh's nodes or the links do not form a tree.
bool mesh_preorder(const rtg_mesh& M, const rtg_bvh_node* N, std::vector<int>& order) {
    order.clear();
    order.reserve(M.node_count);
    std::vector<int> stack{0};
    while (!stack.empty()) {
        int k = stack.back();
        stack.pop_back();
        if (k < 0 || k >= M.node_count || (int)order.size() >= M.node_count) return false;
        order.push_back(k);
        if (N[k].left >= 0) { stack.push_back(N[k].left + 1); stack.push_back(N[k].left); }
    }
    return true;
}

// The reference's BVH (mesh.cpp:23-156, as the description carries it) re-laid in pre-order
// with skip links (rtg_device.hpp): a stackless walk "hit -> i+1, miss or leaf done -> skip"
// visits boxes and faces in the order of BVH::IntersectBVH's recursion (bvh.cpp:5-30).
int reference_preorder(const rtg_scene_desc* d, std::vector<float4>& nodes, std::vector<int2>& next,
                       std::vector<int>& meshBegin, std::vector<int>& meshEnd, bool& bigleaf, std::string& err) {
    nodes.reserve(2 * d->num_nodes + 2); next.reserve(d->num_nodes);
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        const rtg_bvh_node* N = d->nodes + M.node_offset;
        const int base = (int)(nodes.size() / 2);
        meshBegin[m] = base;
        // pre-order, recording each node's subtree end for the skip link
        std::vector<int> order;
        if (!mesh_preorder(M, N, order)) return fail(err, RTG_ERR_INVALID, "mesh %d: corrupt BVH", m);
        std::vector<int> pos(M.node_count, -1);
        for (size_t i = 0; i < order.size(); ++i) pos[order[i]] = (int)i;
        std::vector<int> size(M.node_count, 1);
        for (int i = (int)order.size() - 1; i >= 0; --i) {
            int k = order[i];
            if (N[k].left >= 0) size[k] = 1 + size[N[k].left] + size[N[k].left + 1];
        }
        for (int k : order) {
            const rtg_bvh_node& n = N[k];
            int skip = base + pos[k] + size[k];
            const int first = M.face_offset + n.first;
            int leaf = -1;
            if (n.left < 0) leaf = (first < (1 << 23) && n.count < 255) ? (first << 8) | n.count : LEAF_EXT;
            if (n.left < 0 && n.count > kBigLeaf) bigleaf = true;
            float4 a, b;
            a.x = n.bmin[0]; a.y = n.bmin[1]; a.z = n.bmin[2]; a.w = n.bmax[0];
            b.x = n.bmax[1]; b.y = n.bmax[2];
            std::memcpy(&b.z, &skip, 4);
            std::memcpy(&b.w, &leaf, 4);
            nodes.push_back(a); nodes.push_back(b);
            next.push_back(make_int2(n.left < 0 ? first : -1, n.left < 0 ? n.count : 0));
        }
        meshEnd[m] = (int)(nodes.size() / 2);
    }
    return RTG_OK;
}

// Any-hit trees of every mesh (rtg_ahb.cpp).  `reach` bounds |A - o| in the mesh's local space
// for every shadow ray: origins are surface points and ends light points (a directional
// light's ray matters only inside the scene), so the world box of every object and light,
// mapped into each object's local space, bounds both.  False (and no trees) when a leaf
// entry range does not fit its encoding: shadow rays then take the reference walk.
bool anyhit_trees(const rtg_scene_desc* d, const std::vector<float4>& nd, const std::vector<int2>& nx,
                  const std::vector<int>& meshBegin, const std::vector<int>& meshEnd, const float4* htp, int mode,
                  std::vector<WNode>& anodes, std::vector<float4>& ahtris, std::vector<int>& aroot, AhbStats& ast) {
    double wlo[3] = {INFINITY, INFINITY, INFINITY}, whi[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto addp = [&](double x, double y, double z) {
        const double p[3] = {x, y, z};
        for (int k = 0; k < 3; ++k) { wlo[k] = std::min(wlo[k], p[k]); whi[k] = std::max(whi[k], p[k]); }
    };
    auto xf = [](const double* m, const double* p, double* o) {
        for (int r = 0; r < 3; ++r) o[r] = m[4 * r] * p[0] + m[4 * r + 1] * p[1] + m[4 * r + 2] * p[2] + m[4 * r + 3];
    };
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        double lo[3], hi[3];
        if (o.kind == RTG_OBJ_SPHERE) {
            for (int k = 0; k < 3; ++k) {
                lo[k] = (&o.center.x)[k] - std::fabs((double)o.radius);
                hi[k] = (&o.center.x)[k] + std::fabs((double)o.radius);
            }
        } else {
            for (int k = 0; k < 3; ++k) { lo[k] = o.bbox_min[k]; hi[k] = o.bbox_max[k]; }
        }
        for (int c = 0; c < 8; ++c) {
            const double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
            if (o.kind == RTG_OBJ_INSTANCE) { addp(p[0], p[1], p[2]); continue; }   // world box already
            double w[3];
            xf(o.transform, p, w);
            addp(w[0], w[1], w[2]);
        }
    }
    for (int i = 0; i < d->num_point_lights; ++i)
        addp(d->point_lights[i].position.x, d->point_lights[i].position.y, d->point_lights[i].position.z);
    for (int i = 0; i < d->num_spot_lights; ++i)
        addp(d->spot_lights[i].position.x, d->spot_lights[i].position.y, d->spot_lights[i].position.z);
    for (int i = 0; i < d->num_area_lights; ++i) {
        const rtg_area_light& L = d->area_lights[i];
        for (int c = 0; c < 4; ++c) {
            const double su = (c & 1) ? 0.5 : -0.5, sv = (c & 2) ? 0.5 : -0.5;
            addp(L.position.x + (L.u.x * su + L.v.x * sv) * L.extent, L.position.y + (L.u.y * su + L.v.y * sv) * L.extent,
                 L.position.z + (L.u.z * su + L.v.z * sv) * L.extent);
        }
    }
    // reach = the diagonal of the local-space box holding the mesh and every world point (the
    // distance |A - o| between a face and a shadow ray's origin is below it)
    std::vector<double> reach(d->num_meshes, 0.0);
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        if (o.kind == RTG_OBJ_SPHERE) continue;
        double lo[3], hi[3];
        for (int k = 0; k < 3; ++k) { lo[k] = o.bbox_min[k]; hi[k] = o.bbox_max[k]; }
        for (int c = 0; c < 8 && std::isfinite(wlo[0]); ++c) {
            const double p[3] = {(c & 1) ? whi[0] : wlo[0], (c & 2) ? whi[1] : wlo[1], (c & 4) ? whi[2] : wlo[2]};
            double l[3];
            xf(o.inv_transform, p, l);
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], l[k]); hi[k] = std::max(hi[k], l[k]); }
        }
        const double diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) +
                                      (hi[2] - lo[2]) * (hi[2] - lo[2]));
        reach[o.mesh] = std::max(reach[o.mesh], diag);
    }
    auto build_all = [&](AhbMode md, std::vector<WNode>& wn, std::vector<float4>& we, std::vector<int>& roots,
                         AhbStats& st) {
        roots.assign(d->num_meshes, -1);
        for (int m = 0; m < d->num_meshes; ++m) {
            if (meshEnd[m] <= meshBegin[m]) continue;
            roots[m] = build_ahb(nd, nx, meshBegin[m], meshEnd[m], htp, reach[m], md, wn, we, &st);
            if (roots[m] == -2) return false;   // leaf encoding exceeded: shadow rays take the reference walk
        }
        return true;
    };
    const bool fresh = anodes.empty() && ahtris.empty();
    const AhbStats ast0 = ast;
    bool ahbOk = build_all((AhbMode)mode, anodes, ahtris, aroot, ast);
    // The binned SAH is a heuristic: on some scenes (long runs of equal boxes, one outlier that
    // stretches the bins) its trees have more wide nodes than the reference's own topology
    // collapsed.  The default trees are never the larger set: a scene on which the SAH loses
    // takes the reference's topology over the same primitives and cull boxes, so the walk's
    // decisions are what they were.  (The split tree has other primitives and keeps the SAH.)
    if (ahbOk && fresh && mode == AHB_EXACT) {
        std::vector<WNode> rn;
        std::vector<float4> re;
        std::vector<int> rr;
        AhbStats rs = ast0;
        if (build_all(AHB_REF, rn, re, rr, rs) && rs.nodes < ast.nodes) {
            anodes.swap(rn);
            ahtris.swap(re);
            aroot.swap(rr);
            ast = rs;
        }
    }
    if (!ahbOk) { anodes.clear(); ahtris.clear(); aroot.assign(d->num_meshes, -1); }
    return ahbOk;
}

// The face tables of the description's own (already BVH-permuted) face order.
void face_tables(const rtg_scene_desc* d, SceneTables& T) {
    const size_t F = (size_t)d->num_faces;
    const bool uv = any_uv(d), mapped = any_mapped(d);
    T.tris.resize(3 * F);
    T.face_n.resize(F);
    T.face_uv.resize(uv ? 3 * F : 0);
    T.face_v12.resize(mapped ? 2 * F : 0);
    for (size_t f = 0; f < F; ++f) {
        const rtg_face& A = d->faces[f];
        // the walk's record {v0}, {v0 - v1}, {v0 - v2} (matrixA columns of mesh.cpp:208-210)
        T.tris[3 * f] = make_float4(A.v0.x, A.v0.y, A.v0.z, 0.f);
        T.tris[3 * f + 1] = make_float4(A.v0.x - A.v1.x, A.v0.y - A.v1.y, A.v0.z - A.v1.z, 0.f);
        T.tris[3 * f + 2] = make_float4(A.v0.x - A.v2.x, A.v0.y - A.v2.y, A.v0.z - A.v2.z, 0.f);
        T.face_n[f] = make_float4(A.n.x, A.n.y, A.n.z, 0.f);
        if (uv) {
            T.face_uv[3 * f] = make_float2(A.uv0[0], A.uv0[1]);
            T.face_uv[3 * f + 1] = make_float2(A.uv1[0], A.uv1[1]);
            T.face_uv[3 * f + 2] = make_float2(A.uv2[0], A.uv2[1]);
        }
        if (mapped) {
            T.face_v12[2 * f] = make_float4(A.v1.x, A.v1.y, A.v1.z, 0.f);
            T.face_v12[2 * f + 1] = make_float4(A.v2.x, A.v2.y, A.v2.z, 0.f);
        }
    }
}

// Objects with their feature bits; returns the scene's FEAT_SPHERE / INSTANCE / XFORM bits.
int object_table(const rtg_scene_desc* d, SceneTables& T) {
    T.objects.resize(d->num_objects);
    int feat = 0;
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        DevObject& D = T.objects[i];
        std::memset(&D, 0, sizeof(D));
        D.kind = o.kind;
        D.material = o.material;
        D.flags = o.flags;
        D.aroot = -1;
        if (o.kind != RTG_OBJ_SPHERE) {
            D.node_begin = T.mesh_begin[o.mesh];
            D.node_end = T.mesh_end[o.mesh];
            if (d->meshes[o.mesh].has_uv) D.flags |= OBJF_HAS_UV;
        }
        D.tex_diffuse = o.tex_diffuse;
        D.tex_specular = o.tex_specular;
        D.tex_replace_all = o.tex_replace_all;
        // maps only act where the reference reads them: mesh faces with UVs (mesh.cpp:245-358)
        // and sphere bump maps (sphere.cpp:116-170)
        const bool uvmesh = o.kind != RTG_OBJ_SPHERE && d->meshes[o.mesh].has_uv;
        D.tex_normal = uvmesh ? o.tex_normal : -1;
        D.tex_bump = (uvmesh && o.tex_normal < 0) || o.kind == RTG_OBJ_SPHERE ? o.tex_bump : -1;
        if (D.tex_normal >= 0 || D.tex_bump >= 0) D.flags |= OBJF_MAPPED;
        for (int k = 0; k < 3; ++k) { D.bmin[k] = o.bbox_min[k]; D.bmax[k] = o.bbox_max[k]; }
        f4(D.mbv, o.motion_blur);
        f4(D.center, o.center, o.radius);
        bool ident = true;
        for (int k = 0; k < 12; ++k) {
            D.inv[k] = o.inv_transform[k];
            D.invT[k] = o.inv_transpose[k];
            D.baseInvT[k] = o.base_inv_transpose[k];
            ident &= o.inv_transform[k] == ((k % 5 == 0) ? 1.0 : 0.0);
        }
        if (ident) D.flags |= OBJF_IDENTITY;
        D.id = o.kind == RTG_OBJ_SPHERE ? INT32_MIN : o.id;   // spheres never carry a light's id
        if (o.kind == RTG_OBJ_SPHERE) feat |= FEAT_SPHERE;
        else if (o.kind == RTG_OBJ_INSTANCE) feat |= FEAT_INSTANCE;
        else if (!ident || (o.flags & RTG_OBJF_MOTION_BLUR)) feat |= FEAT_XFORM;
    }
    return feat;
}

// Shadow-ray acceleration (rtg_anyhit.hpp): the any-hit wide BVH (trace_any_wide) and
// face -> reference leaf (its exact leaf-box decisions, the deferred leaves' checks), from the
// walk records nd / nx and the face records tris.
void shadow_tables(const rtg_scene_desc* d, const TableOptions& opt, const std::vector<float4>& nd,
                   const std::vector<int2>& nx, const float4* tris, SceneTables& T) {
    auto leafv = [&](int i) { int l; std::memcpy(&l, &nd[2 * i + 1].w, 4); return l; };
    T.face_leaf.assign((size_t)d->num_faces, -1);
    for (int m = 0; m < d->num_meshes; ++m)
        for (int p = T.mesh_begin[m]; p < T.mesh_end[m]; ++p) {
            const int l = leafv(p);
            if (l < 0) continue;
            int first = l >> 8, cnt = l & 255;
            if (l == LEAF_EXT) { first = nx[p].x; cnt = nx[p].y; }
            for (int f = first; f < first + cnt; ++f) T.face_leaf[f] = p;
        }
    T.ahb_mode = opt.ahb_mode;
    T.ahb_ok = anyhit_trees(d, nd, nx, T.mesh_begin, T.mesh_end, tris, opt.ahb_mode, T.anodes, T.ahtris, T.aroot, T.ahb);
    for (int i = 0; i < d->num_objects; ++i)
        T.objects[i].aroot = d->objects[i].kind != RTG_OBJ_SPHERE ? T.aroot[d->objects[i].mesh] : -1;
    if (opt.verbose)
        std::fprintf(stderr, "rtgpu any-hit tree (mode %d): %lld nodes, %lld entries, depth %d, %lld leaf prims, "
                             "%lld face prims (%lld on their leaf box)\n",
                     T.ahb_mode, T.ahb.nodes, T.ahb.entries, T.ahb.max_depth, T.ahb.leaf_prims, T.ahb.face_prims,
                     T.ahb.exact_faces);
}

// Instance groups: runs of consecutive instances without motion blur, chunked by ~sqrt of
// the run length, with the exact (min/max) union of the members' world boxes.
void instance_groups(SceneTables& T) {
    std::vector<DevObject>& objs = T.objects;
    const int n = (int)objs.size();
    T.group_box.assign(2 * (size_t)n, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int k = 0; k < n;) {
        auto eligible = [&](int i) { return objs[i].kind == OBJ_INSTANCE && !(objs[i].flags & OBJF_MOTION_BLUR); };
        if (!eligible(k)) { ++k; continue; }
        int e = k;
        while (e < n && eligible(e)) ++e;
        const int run = e - k;
        const int gsz = std::max(4, (int)std::lround(std::sqrt((double)run)));
        for (int g = k; g < e; g += gsz) {
            const int ge = std::min(e, g + gsz);
            if (ge - g < 2) continue;
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = g; i < ge; ++i)
                for (int c = 0; c < 3; ++c) {
                    mn[c] = std::min(mn[c], objs[i].bmin[c]);
                    mx[c] = std::max(mx[c], objs[i].bmax[c]);
                }
            objs[g].group_end = ge;
            T.group_box[2 * g] = make_float4(mn[0], mn[1], mn[2], 0.f);
            T.group_box[2 * g + 1] = make_float4(mx[0], mx[1], mx[2], 0.f);
        }
        k = e;
    }
}

// feat, shade_sk, num_slots and the pipelines the scene may take.
void scene_scalars(const rtg_scene_desc* d, const TableOptions& opt, int feat, bool bigleaf, SceneTables& T) {
    // wavefront eligibility: no ray-tree children and no motion blur
    bool branching = false, blur = false;
    for (int i = 0; i < d->num_materials; ++i) {
        int t = d->materials[i].type;
        branching |= (t == RTG_MAT_MIRROR || t == RTG_MAT_DIELECTRIC || t == RTG_MAT_CONDUCTOR);
    }
    for (int i = 0; i < d->num_objects; ++i) blur |= (d->objects[i].flags & RTG_OBJF_MOTION_BLUR) != 0;
    // without coop, large leaves are tested by their own lane (the sequential walk handles any
    // leaf size; the cooperative one is only faster)
    T.feat = feat | (bigleaf && opt.coop ? FEAT_BIGLEAF : 0);
    T.tree_ok = !blur && d->max_recursion_depth > 0 && branching;
    T.wave_ok = !blur && (d->max_recursion_depth <= 0 || !branching);
    T.path_ok = !blur;
    T.num_slots = d->num_point_lights + d->num_area_lights + d->num_env_lights + d->num_dir_lights +
                  d->num_spot_lights + d->num_mesh_lights;
    // shading features: textures / maps (incl. a background texture), BRDFs, env / spot / mesh
    // lights
    int sk = 0;
    for (const DevObject& o : T.objects)
        if (o.tex_diffuse >= 0 || o.tex_specular >= 0 || o.tex_replace_all >= 0 || (o.flags & OBJF_MAPPED)) sk |= SK_TEX;
    if (d->bg_texture >= 0) sk |= SK_TEX;
    for (int i = 0; i < d->num_materials; ++i)
        if (d->materials[i].brdf >= 0) sk |= SK_BRDF;
    if (d->num_env_lights + d->num_spot_lights + d->num_mesh_lights > 0) sk |= SK_XLIGHT;
    T.shade_sk = sk;
}

// A mesh light's record (meshLight.h) over faces [face_begin, ...) of light_faces.
void mesh_light_record(const rtg_scene_desc* d, int i, int face_begin, DevMeshLight& L) {
    const rtg_object& o = d->objects[d->mesh_lights[i].object];
    const rtg_mesh& M = d->meshes[o.mesh];
    std::memset(&L, 0, sizeof(L));
    L.id = o.id;
    L.face_begin = face_begin;
    L.face_count = M.face_count;
    f4(L.radiance, d->mesh_lights[i].radiance);
    L.surface_area = M.surface_area;
    for (int k = 0; k < 12; ++k) L.xf[k] = o.transform[k];
}

// Mesh lights: their records and their faces in MeshLight::faces order (the BVH-permuted one;
// `perm`, nullable: final face position -> description face).
void mesh_light_tables(const rtg_scene_desc* d, const std::vector<int>* perm, SceneTables& T) {
    T.mesh_lights.resize(d->num_mesh_lights);
    for (int i = 0; i < d->num_mesh_lights; ++i) {
        mesh_light_record(d, i, (int)T.light_faces.size(), T.mesh_lights[i]);
        const rtg_mesh& M = d->meshes[d->objects[d->mesh_lights[i].object].mesh];
        for (int f = 0; f < M.face_count; ++f) {
            const rtg_face& F = d->faces[perm ? (*perm)[M.face_offset + f] : M.face_offset + f];
            DevLightFace lf;
            std::memset(&lf, 0, sizeof(lf));
            f4(lf.v0, F.v0); f4(lf.v1, F.v1); f4(lf.v2, F.v2);
            lf.area = F.area;
            T.light_faces.push_back(lf);
        }
    }
}

// Materials, BRDFs and textures.
void shading_records(const rtg_scene_desc* d, SceneTables& T) {
    T.materials.resize(d->num_materials);
    for (int i = 0; i < d->num_materials; ++i) {
        const rtg_material& m = d->materials[i];
        DevMaterial& D = T.materials[i];
        std::memset(&D, 0, sizeof(D));
        D.type = m.type;
        D.brdf = m.brdf;
        f4(D.ambient, m.ambient); f4(D.diffuse, m.diffuse); f4(D.specular, m.specular); f4(D.mirror, m.mirror);
        f4(D.absorption, m.absorption); f4(D.radiance, m.radiance);
        D.phong_exponent = m.phong_exponent;
        D.refractive_index = m.refractive_index;
        D.absorption_index = m.absorption_index;
        D.roughness = m.roughness;
    }
    T.brdfs.resize(d->num_brdfs);
    for (int i = 0; i < d->num_brdfs; ++i) {
        DevBrdf& B = T.brdfs[i];
        std::memset(&B, 0, sizeof(B));
        B.type = d->brdfs[i].type;
        B.energy_conserving = d->brdfs[i].energy_conserving;
        B.kd_fresnel = d->brdfs[i].kd_fresnel;
        B.exponent = d->brdfs[i].exponent;
    }
    T.textures.resize(d->num_textures);
    for (int i = 0; i < d->num_textures; ++i) {
        const rtg_texture& t = d->textures[i];
        DevTexture& X = T.textures[i];
        std::memset(&X, 0, sizeof(X));
        X.kind = t.kind;
        X.blend = t.blend;
        X.image = t.image;
        X.nearest = t.nearest;
        X.noise_scale = t.noise_scale;
        X.bump_factor = t.bump_factor;
        X.normalizer = t.normalizer;
        X.noise_abs = t.noise_abs;
    }
}

// An image's record at `offset` of the texel pool.
void image_record(const rtg_image& im, long long offset, DevImage& I) {
    std::memset(&I, 0, sizeof(I));
    I.width = im.width; I.height = im.height; I.channels = im.channels;
    I.offset = offset;
}

// The records above, the texel pool and the Perlin tables.
void shading_tables(const rtg_scene_desc* d, SceneTables& T) {
    shading_records(d, T);
    // texel pool; each image padded with one extra row + 4 floats so the reference's
    // edge reads (bilinear p+1, 1-channel RGB reads) stay inside the allocation
    T.images.resize(d->num_images);
    for (int i = 0; i < d->num_images; ++i) {
        const rtg_image& im = d->images[i];
        image_record(im, (long long)T.texels.size(), T.images[i]);
        size_t n = (size_t)im.width * im.height * im.channels;
        T.texels.insert(T.texels.end(), im.texels, im.texels + n);
        T.texels.insert(T.texels.end(), (size_t)im.width * im.channels + 4, 0.f);
    }
    T.perm.resize(512);
    for (int i = 0; i < 512; ++i) T.perm[i] = kPerm256[i & 255];
    T.grad.assign(kGrad, kGrad + 36);
}

// The four analytic light arrays, the env lights' images and env_direction's hash table.
void light_tables(const rtg_scene_desc* d, SceneTables& T) {
    T.point_lights.resize(d->num_point_lights);
    for (int i = 0; i < d->num_point_lights; ++i) {
        f4(T.point_lights[i].pos, d->point_lights[i].position);
        f4(T.point_lights[i].intensity, d->point_lights[i].intensity);
    }
    T.area_lights.resize(d->num_area_lights);
    for (int i = 0; i < d->num_area_lights; ++i) {
        const rtg_area_light& a = d->area_lights[i];
        DevAreaLight& A = T.area_lights[i];
        std::memset(&A, 0, sizeof(A));
        f4(A.pos, a.position); f4(A.normal, a.normal); f4(A.radiance, a.radiance);
        f4(A.u, a.u); f4(A.v, a.v);
        A.extent = a.extent; A.area = a.area;
    }
    T.dir_lights.resize(d->num_dir_lights);
    for (int i = 0; i < d->num_dir_lights; ++i) {
        f4(T.dir_lights[i].dir, d->dir_lights[i].dir);
        f4(T.dir_lights[i].radiance, d->dir_lights[i].radiance);
    }
    T.spot_lights.resize(d->num_spot_lights);
    for (int i = 0; i < d->num_spot_lights; ++i) {
        const rtg_spot_light& s = d->spot_lights[i];
        DevSpotLight& S = T.spot_lights[i];
        std::memset(&S, 0, sizeof(S));
        f4(S.pos, s.position); f4(S.dir, s.dir); f4(S.intensity, s.intensity);
        S.coverage_deg = s.coverage_deg; S.falloff_deg = s.falloff_deg;
        S.cos_half_coverage = s.cos_half_coverage; S.cos_half_falloff = s.cos_half_falloff;
    }
    T.env_images.resize(d->num_env_lights);
    for (int i = 0; i < d->num_env_lights; ++i) T.env_images[i] = d->env_lights[i].image;
    // env_direction's key-independent inner hashes: mix64(RP_ENV << 32 | e * 16384 + j)
    auto mix = [](uint64_t z) {
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    };
    T.env_mix.resize((size_t)d->num_env_lights * kEnvDraws);
    for (int e = 0; e < d->num_env_lights; ++e)
        for (int j = 0; j < kEnvDraws; ++j)
            T.env_mix[(size_t)e * kEnvDraws + j] = mix(((uint64_t)kRpEnv << 32) | (uint32_t)((uint32_t)e * 16384u + (uint32_t)j));
}

// The largest eigenvalue of the symmetric 3x3 matrix b (cyclic Jacobi rotations, double): a
// fixed number of sweeps, far more than 3x3 needs to converge to the last bits.
double sym3_max_eigen(double b[3][3]) {
    for (int sweep = 0; sweep < 16; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (b[p][q] == 0.0) continue;
                const double theta = (b[q][q] - b[p][p]) / (2.0 * b[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {         // columns p, q
                    const double kp = b[k][p], kq = b[k][q];
                    b[k][p] = c * kp - s * kq;
                    b[k][q] = s * kp + c * kq;
                }
                for (int k = 0; k < 3; ++k) {         // rows p, q
                    const double pk = b[p][k], qk = b[q][k];
                    b[p][k] = c * pk - s * qk;
                    b[q][k] = s * pk + c * qk;
                }
            }
    return std::max(b[0][0], std::max(b[1][1], b[2][2]));
}

void point_table(const rtg_scene_desc* d, SceneTables& T) {
    T.point_xf.resize(d->num_objects);
    for (int i = 0; i < d->num_objects; ++i) point_xf_record(d->objects[i], T.point_xf[i]);
}

}  // namespace

// rtg_pointxf.hpp.  Rows 0..2 of the 4x4 row-major matrices are their first 12 entries.
void point_xf_record(const rtg_object& o, PointXf& X) {
    std::memset(&X, 0, sizeof(X));
    bool ident = true;
    for (int k = 0; k < 12; ++k) {
        X.fwd[k] = (float)o.transform[k];
        X.inv[k] = (float)o.inv_transform[k];
        ident &= o.transform[k] == ((k % 5 == 0) ? 1.0 : 0.0);
    }
    X.lip2 = 1.0f;
    X.scale = 1.0f;
    X.flags = PXF_SPHERE_OK;
    if (ident) {
        X.flags |= PXF_IDENTITY;
        return;
    }
    // sigma_max(inv 3x3)^2: the largest eigenvalue of inv^T inv.  A NaN or an overflow ends as
    // lip2 = inf or NaN, under which no box is skipped.
    const double* A = o.inv_transform;
    double b[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) b[r][c] = A[r] * A[c] + A[4 + r] * A[4 + c] + A[8 + r] * A[8 + c];
    const double l2 = sym3_max_eigen(b) * (1.0 + 1e-5);
    X.lip2 = (float)l2;
    if ((double)X.lip2 < l2) X.lip2 = std::nextafterf(X.lip2, INFINITY);
    if (o.kind != RTG_OBJ_SPHERE) return;
    // a sphere stays one under a similarity alone: M^T M = s^2 I within 1e-6 s^2, s = cbrt(|det M|)
    const double* M = o.transform;
    const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) +
                       M[2] * (M[4] * M[9] - M[5] * M[8]);
    const double s = std::cbrt(std::fabs(det)), s2 = s * s;
    bool similar = s > 0.0 && std::isfinite(s);
    for (int r = 0; r < 3 && similar; ++r)
        for (int c = 0; c < 3; ++c) {
            const double g = M[r] * M[c] + M[4 + r] * M[4 + c] + M[8 + r] * M[8 + c];
            if (!(std::fabs(g - (r == c ? s2 : 0.0)) <= 1e-6 * s2)) similar = false;
        }
    X.scale = (float)s;
    if (!similar) X.flags &= ~PXF_SPHERE_OK;
}

bool any_uv(const rtg_scene_desc* d) {
    bool uv = false;
    for (int m = 0; m < d->num_meshes; ++m) uv |= d->meshes[m].has_uv != 0;
    return uv;
}

bool any_mapped(const rtg_scene_desc* d) {
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        const bool uvmesh = o.kind != RTG_OBJ_SPHERE && d->meshes[o.mesh].has_uv;
        if ((uvmesh && o.tex_normal >= 0) || ((uvmesh || o.kind == RTG_OBJ_SPHERE) && o.tex_bump >= 0)) return true;
    }
    return false;
}

namespace {
// validate_desc; `geometry` false: without the checks that read faces, nodes or texels
int validate(const rtg_scene_desc* d, bool geometry, std::string& err) {
    // the packet walks address records by 32-bit byte offsets (rtg_isect.hpp rec_at)
    if (geometry && d->num_faces > ((int64_t)1 << 25))
        return fail(err, RTG_ERR_INVALID, "%lld faces: at most 2^25 per scene", (long long)d->num_faces);
    for (int i = 0; i < d->num_mesh_lights; ++i) {
        const int o = d->mesh_lights ? d->mesh_lights[i].object : -1;
        if (o < 0 || o >= d->num_objects || d->objects[o].kind != RTG_OBJ_MESH ||
            d->meshes[d->objects[o].mesh].face_count <= 0)
            return fail(err, RTG_ERR_INVALID, "mesh light %d: bad object", i);
    }
    if (d->max_recursion_depth > max_supported_depth())
        return fail(err, RTG_ERR_UNSUPPORTED, "MaxRecursionDepth %d > %d", d->max_recursion_depth, max_supported_depth());
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        if (o.kind == RTG_OBJ_SPHERE && o.tex_normal >= 0)
            return fail(err, RTG_ERR_UNSUPPORTED, "sphere %d: normal map (the reference leaves the normal unset, "
                        "sphere.cpp:95-113)", i);
        if ((o.tex_normal >= d->num_textures) || (o.tex_bump >= d->num_textures))
            return fail(err, RTG_ERR_INVALID, "object %d: bad normal / bump texture", i);
        if (o.tex_normal >= 0 && d->textures[o.tex_normal].kind == RTG_TEX_IMAGE &&
            (d->textures[o.tex_normal].image < 0 || d->textures[o.tex_normal].image >= d->num_images))
            return fail(err, RTG_ERR_INVALID, "object %d: normal map without an image", i);
        if (o.tex_bump >= 0 && d->textures[o.tex_bump].kind == RTG_TEX_IMAGE &&
            (d->textures[o.tex_bump].image < 0 || d->textures[o.tex_bump].image >= d->num_images))
            return fail(err, RTG_ERR_INVALID, "object %d: bump map without an image", i);
        if (o.material < 0 || o.material >= d->num_materials) return fail(err, RTG_ERR_INVALID, "object %d: bad material", i);
        if (o.kind != RTG_OBJ_SPHERE && (o.mesh < 0 || o.mesh >= d->num_meshes))
            return fail(err, RTG_ERR_INVALID, "object %d: bad mesh", i);
    }
    for (int i = 0; i < d->num_images && geometry; ++i)
        if (d->images[i].channels < 1 || !d->images[i].texels) return fail(err, RTG_ERR_INVALID, "image %d: no texels", i);
    std::vector<int> order;
    for (int m = 0; m < d->num_meshes && d->num_nodes > 0 && geometry; ++m)
        if (!mesh_preorder(d->meshes[m], d->nodes + d->meshes[m].node_offset, order))
            return fail(err, RTG_ERR_INVALID, "mesh %d: corrupt BVH", m);
    for (int i = 0; i < d->num_env_lights; ++i)
        if (d->env_lights[i].image < 0 || d->env_lights[i].image >= d->num_images)
            return fail(err, RTG_ERR_INVALID, "env light %d: bad image", i);
    return RTG_OK;
}
}  // namespace

int validate_desc(const rtg_scene_desc* d, std::string& err) { return validate(d, true, err); }
int validate_desc_update(const rtg_scene_desc* d, std::string& err) { return validate(d, false, err); }

int build_scene_tables(const rtg_scene_desc* d, const TableOptions& opt, const BvhReadback* rb, SceneTables& T,
                       std::string& err) {
    T = SceneTables();
    if (!rb && d->num_faces > 0 && d->num_nodes == 0) return fail(err, RTG_ERR_INVALID, "description without a BVH");
    bool bigleaf = false;
    if (rb) {
        T.mesh_begin = rb->mesh_begin;
        T.mesh_end = rb->mesh_end;
        T.node_count = rb->node_count;
        bigleaf = rb->bigleaf;
    } else {
        T.mesh_begin.resize(d->num_meshes);
        T.mesh_end.resize(d->num_meshes);
        const int rc = reference_preorder(d, T.nodes, T.node_ext, T.mesh_begin, T.mesh_end, bigleaf, err);
        if (rc) return rc;
        T.nodes.push_back(make_float4(0.f, 0.f, 0.f, 0.f));     // pad node: walk_bvh prefetches i+1
        T.nodes.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
        T.node_count = (int)(T.nodes.size() / 2);
        face_tables(d, T);
    }
    const int feat = object_table(d, T);
    point_table(d, T);
    if (opt.fast_shadow && d->num_meshes > 0)
        shadow_tables(d, opt, rb ? rb->nodes : T.nodes, rb ? rb->ext : T.node_ext, rb ? rb->tris.data() : T.tris.data(), T);
    T.ahb_split = T.ahb_mode == AHB_SPLIT && !T.anodes.empty();
    T.bigleaf = bigleaf;
    instance_groups(T);
    scene_scalars(d, opt, feat, bigleaf, T);
    mesh_light_tables(d, rb ? &rb->perm : nullptr, T);
    shading_tables(d, T);
    light_tables(d, T);
    return RTG_OK;
}

void keep_tables(const rtg_scene_desc* d, const SceneTables& T, KeptTables& K) {
    K = KeptTables();
    K.mesh_begin = T.mesh_begin; K.mesh_end = T.mesh_end; K.aroot = T.aroot;
    K.bigleaf = T.bigleaf;
    K.ahb_mode = T.ahb_mode; K.ahb_ok = T.ahb_ok; K.ahb_split = T.ahb_split;
    K.has_uv = any_uv(d); K.has_v12 = any_mapped(d);
    for (int i = 0; i < d->num_mesh_lights; ++i) {
        K.light_face_begin.push_back(T.mesh_lights[i].face_begin);
        K.light_face_count.push_back(T.mesh_lights[i].face_count);
        K.light_object.push_back(d->mesh_lights[i].object);
    }
    for (const DevImage& I : T.images) K.image_offset.push_back(I.offset);
    K.num_faces = d->num_faces; K.num_nodes = d->num_nodes;
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        K.meshes.push_back({M.face_offset, M.face_count, M.node_offset, M.node_count, M.has_uv});
    }
    for (int i = 0; i < d->num_objects; ++i) K.objects.push_back(make_int2(d->objects[i].kind, d->objects[i].mesh));
    for (int i = 0; i < d->num_images; ++i)
        K.images.push_back({d->images[i].width, d->images[i].height, d->images[i].channels, d->images[i].is_hdr});
}

int same_geometry(const rtg_scene_desc* d, const KeptTables& K, std::string& err) {
    if (d->num_meshes != (int)K.meshes.size() || d->num_faces != K.num_faces || d->num_nodes != K.num_nodes ||
        d->num_objects != (int)K.objects.size())
        return fail(err, RTG_ERR_INVALID, "geometry differs: %d meshes, %lld faces, %lld nodes, %d objects against the "
                    "scene's %zu, %lld, %lld, %zu", d->num_meshes, (long long)d->num_faces, (long long)d->num_nodes,
                    d->num_objects, K.meshes.size(), K.num_faces, K.num_nodes, K.objects.size());
    if ((d->num_meshes > 0 && !d->meshes) || (d->num_objects > 0 && !d->objects) || (d->num_images > 0 && !d->images) ||
        (d->num_mesh_lights > 0 && !d->mesh_lights))
        return fail(err, RTG_ERR_INVALID, "null table in the description");
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        const KeptTables::Mesh& k = K.meshes[m];
        if (M.face_offset != k.face_offset || M.face_count != k.face_count || M.node_offset != k.node_offset ||
            M.node_count != k.node_count || M.has_uv != k.has_uv)
            return fail(err, RTG_ERR_INVALID, "mesh %d: face / node range or UVs differ from the scene's", m);
    }
    for (int i = 0; i < d->num_objects; ++i)
        if (d->objects[i].kind != K.objects[i].x || d->objects[i].mesh != K.objects[i].y)
            return fail(err, RTG_ERR_INVALID, "object %d: kind or mesh differs from the scene's", i);
    if (d->num_images != (int)K.images.size())
        return fail(err, RTG_ERR_INVALID, "%d images, the scene has %zu", d->num_images, K.images.size());
    for (int i = 0; i < d->num_images; ++i) {
        const rtg_image& im = d->images[i];
        const KeptTables::Image& k = K.images[i];
        if (im.width != k.width || im.height != k.height || im.channels != k.channels || im.is_hdr != k.is_hdr)
            return fail(err, RTG_ERR_INVALID, "image %d: size or format differs from the scene's", i);
    }
    if (d->num_mesh_lights != (int)K.light_object.size())
        return fail(err, RTG_ERR_INVALID, "%d mesh lights, the scene has %zu", d->num_mesh_lights, K.light_object.size());
    for (int i = 0; i < d->num_mesh_lights; ++i)
        if (d->mesh_lights[i].object != K.light_object[i])
            return fail(err, RTG_ERR_INVALID, "mesh light %d: object differs from the scene's", i);
    return RTG_OK;
}

int update_scene_tables(const rtg_scene_desc* d, const KeptTables& K, const TableOptions& opt, SceneTables& T,
                        std::string& err) {
    int rc = same_geometry(d, K, err);
    if (!rc) rc = validate_desc_update(d, err);
    if (rc) return rc;
    if (any_mapped(d) && !K.has_v12)
        return fail(err, RTG_ERR_UNSUPPORTED, "a normal / bump map in a scene created without one (no face_v12 table)");
    if (K.ahb_split)
        return fail(err, RTG_ERR_UNSUPPORTED, "any-hit trees built in the split mode depend on transforms and lights");
    T = SceneTables();
    T.mesh_begin = K.mesh_begin; T.mesh_end = K.mesh_end; T.aroot = K.aroot;
    T.ahb_mode = K.ahb_mode; T.ahb_ok = K.ahb_ok; T.ahb_split = K.ahb_split; T.bigleaf = K.bigleaf;
    const int feat = object_table(d, T);
    point_table(d, T);
    if (!T.aroot.empty())
        for (int i = 0; i < d->num_objects; ++i)
            T.objects[i].aroot = d->objects[i].kind != RTG_OBJ_SPHERE ? T.aroot[d->objects[i].mesh] : -1;
    instance_groups(T);
    scene_scalars(d, opt, feat, K.bigleaf, T);
    T.mesh_lights.resize(d->num_mesh_lights);
    for (int i = 0; i < d->num_mesh_lights; ++i) mesh_light_record(d, i, K.light_face_begin[i], T.mesh_lights[i]);
    shading_records(d, T);
    T.images.resize(d->num_images);
    for (int i = 0; i < d->num_images; ++i) image_record(d->images[i], K.image_offset[i], T.images[i]);
    light_tables(d, T);
    return RTG_OK;
}

}  // namespace rtg
