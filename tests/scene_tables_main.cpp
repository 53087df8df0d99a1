// Stand-alone check of the description -> kernel tables conversion (csrc/scene_tables.cpp),
// host only: links host_xml.cpp host_scene.cpp host_assets.cpp scene_tables.cpp rtg_ahb.cpp -lz,
// neither the library nor HIP (tests/test_scene_tables.py builds and runs it).
//
//   scene_tables_main [--digest] scene.xml...
//
// Loads each scene, builds its tables in the three any-hit modes and once without the
// shadow-ray acceleration, checks them against the description (below; exit 1 with a message
// on the first violation) and, with --digest, prints one JSON object
// {scene: {mode: {table: hash of its raw bytes, scalar: value}}} -- the content of
// tests/golden/scene_tables.json.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host_scene.hpp"
#include "scene_tables.hpp"

namespace {

std::string g_where;

[[noreturn]] void die(const char* fmt, ...) {
    std::fprintf(stderr, "scene_tables_main: %s: ", g_where.c_str());
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) die(__VA_ARGS__); } while (0)

// FNV-1a, 64 bit, over the byte count and then the bytes
uint64_t fnv64(const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    uint64_t h = (1469598103934665603ull ^ (uint64_t)n) * 1099511628211ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

using Digest = std::map<std::string, std::string>;   // table -> hash, scalar -> value

Digest digest(const rtg::SceneTables& T) {
    Digest D;
    auto tab = [&](const char* name, const auto& v) {
        char buf[32];
        std::snprintf(buf, sizeof(buf), "\"%016llx\"", (unsigned long long)fnv64(v.data(), v.size() * sizeof(v[0])));
        D[name] = buf;
    };
    auto num = [&](const char* name, long long v) { D[name] = std::to_string(v); };
    tab("nodes", T.nodes); tab("node_ext", T.node_ext); tab("tris", T.tris); tab("face_n", T.face_n);
    tab("face_uv", T.face_uv); tab("face_v12", T.face_v12);
    tab("objects", T.objects); tab("group_box", T.group_box); tab("materials", T.materials); tab("brdfs", T.brdfs);
    tab("textures", T.textures); tab("images", T.images); tab("texels", T.texels);
    tab("point_lights", T.point_lights); tab("area_lights", T.area_lights); tab("dir_lights", T.dir_lights);
    tab("spot_lights", T.spot_lights); tab("env_images", T.env_images); tab("env_mix", T.env_mix);
    tab("mesh_lights", T.mesh_lights); tab("light_faces", T.light_faces);
    tab("anodes", T.anodes); tab("ahtris", T.ahtris); tab("face_leaf", T.face_leaf);
    tab("perm", T.perm); tab("grad", T.grad);
    num("node_count", T.node_count); num("feat", T.feat); num("shade_sk", T.shade_sk); num("num_slots", T.num_slots);
    num("wave_ok", T.wave_ok); num("tree_ok", T.tree_ok); num("path_ok", T.path_ok);
    num("ahb_mode", T.ahb_mode); num("ahb_split", T.ahb_split);
    num("ahb_nodes", T.ahb.nodes); num("ahb_entries", T.ahb.entries); num("ahb_max_depth", T.ahb.max_depth);
    num("ahb_leaf_prims", T.ahb.leaf_prims); num("ahb_face_prims", T.ahb.face_prims);
    num("ahb_exact_faces", T.ahb.exact_faces);
    return D;
}

int as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
bool same(const float4& a, float x, float y, float z, float w) {
    const float b[4] = {x, y, z, w};
    return std::memcmp(&a, b, 16) == 0;
}

// recursive left-first descent of one mesh's BVH as the description carries it
void descend(const rtg_bvh_node* N, int k, std::vector<int>& order, std::vector<int>& size) {
    const size_t at = order.size();
    order.push_back(k);
    size.push_back(1);
    if (N[k].left >= 0) { descend(N, N[k].left, order, size); descend(N, N[k].left + 1, order, size); }
    size[at] = (int)(order.size() - at);
}

// The walk records against the description: pre-order, skip links, leaf ranges, pad node.
void check_walk(const rtg_scene_desc* d, const rtg::SceneTables& T) {
    int total = 0;
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        const rtg_bvh_node* N = d->nodes + M.node_offset;
        std::vector<int> order, size;
        descend(N, 0, order, size);
        const int begin = T.mesh_begin[m];
        CHECK(begin == total && T.mesh_end[m] == begin + (int)order.size(), "mesh %d: node range", m);
        total += (int)order.size();
        // "hit -> i+1, miss or leaf -> skip" with every box hit visits the recursion's order
        size_t seen = 0;
        for (int i = begin; i < T.mesh_end[m]; ++seen) {
            CHECK(seen < order.size() && i == begin + (int)seen, "mesh %d: walk leaves the pre-order at node %d", m, i);
            const rtg_bvh_node& n = N[order[seen]];
            const float4 a = T.nodes[2 * i], b = T.nodes[2 * i + 1];
            CHECK(a.x == n.bmin[0] && a.y == n.bmin[1] && a.z == n.bmin[2] && a.w == n.bmax[0] && b.x == n.bmax[1] &&
                  b.y == n.bmax[2], "mesh %d node %d: box", m, i);
            const int skip = as_int(b.z), leaf = as_int(b.w);
            CHECK(skip == i + size[seen], "mesh %d node %d: skip %d, subtree ends at %d", m, i, skip, i + size[seen]);
            CHECK((leaf < 0) == (n.left >= 0), "mesh %d node %d: leaf flag", m, i);
            if (leaf >= 0) {
                int first = leaf >> 8, count = leaf & 255;
                if (leaf == rtg::LEAF_EXT) { first = T.node_ext[i].x; count = T.node_ext[i].y; }
                CHECK(first == M.face_offset + n.first && count == n.count, "mesh %d node %d: leaf range", m, i);
            }
            i = leaf >= 0 ? skip : i + 1;
        }
        CHECK(seen == order.size(), "mesh %d: walk visits %zu of %zu nodes", m, seen, order.size());
    }
    CHECK(T.node_count == total + 1 && T.nodes.size() == 2 * (size_t)T.node_count, "node count");
    CHECK(same(T.nodes[2 * total], 0, 0, 0, 0) && same(T.nodes[2 * total + 1], 0, 0, 0, 0), "pad node not zero");
    for (int64_t f = 0; f < d->num_faces; ++f) {
        const rtg_face& F = d->faces[f];
        CHECK(same(T.tris[3 * f], F.v0.x, F.v0.y, F.v0.z, 0.f) &&
              same(T.tris[3 * f + 1], F.v0.x - F.v1.x, F.v0.y - F.v1.y, F.v0.z - F.v1.z, 0.f) &&
              same(T.tris[3 * f + 2], F.v0.x - F.v2.x, F.v0.y - F.v2.y, F.v0.z - F.v2.z, 0.f),
              "face record %lld", (long long)f);
    }
}

void check_objects(const rtg_scene_desc* d, const rtg::TableOptions& opt, const rtg::SceneTables& T) {
    int feat = 0;
    for (int i = 0; i < d->num_objects; ++i) {
        const rtg_object& o = d->objects[i];
        const rtg::DevObject& D = T.objects[i];
        bool ident = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) ident = ident && o.inv_transform[4 * r + c] == (r == c ? 1.0 : 0.0);
        CHECK(((D.flags & rtg::OBJF_IDENTITY) != 0) == ident, "object %d: OBJF_IDENTITY", i);
        if (o.kind == RTG_OBJ_SPHERE) feat |= rtg::FEAT_SPHERE;
        if (o.kind == RTG_OBJ_INSTANCE) feat |= rtg::FEAT_INSTANCE;
        if (!opt.fast_shadow) CHECK(D.aroot == -1, "object %d: any-hit root without trees", i);
        if (D.group_end <= 0) continue;
        CHECK(D.group_end > i + 1 && D.group_end <= d->num_objects, "object %d: group end %d", i, D.group_end);
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = i; k < D.group_end; ++k) {
            const rtg_object& g = d->objects[k];
            CHECK(g.kind == RTG_OBJ_INSTANCE && !(g.flags & RTG_OBJF_MOTION_BLUR), "object %d: group member %d", i, k);
            for (int c = 0; c < 3; ++c) {
                mn[c] = g.bbox_min[c] < mn[c] ? g.bbox_min[c] : mn[c];
                mx[c] = g.bbox_max[c] > mx[c] ? g.bbox_max[c] : mx[c];
            }
        }
        CHECK(same(T.group_box[2 * i], mn[0], mn[1], mn[2], 0.f) && same(T.group_box[2 * i + 1], mx[0], mx[1], mx[2], 0.f),
              "object %d: group box", i);
    }
    for (int m = 0; m < d->num_meshes && opt.coop; ++m)
        for (int k = 0; k < d->meshes[m].node_count; ++k) {
            const rtg_bvh_node& n = d->nodes[d->meshes[m].node_offset + k];
            if (n.left < 0 && n.count > rtg::kBigLeaf) feat |= rtg::FEAT_BIGLEAF;
        }
    const int mask = rtg::FEAT_SPHERE | rtg::FEAT_INSTANCE | rtg::FEAT_BIGLEAF;
    CHECK((T.feat & mask) == feat, "feature bits 0x%x, the description's 0x%x", T.feat & mask, feat);
}

// face -> leaf and the any-hit trees (what tests/test_ahb.py asserts through the library)
void check_shadow(const rtg_scene_desc* d, const rtg::TableOptions& opt, const rtg::SceneTables& T) {
    if (!opt.fast_shadow) {
        CHECK(T.anodes.empty() && T.ahtris.empty() && T.face_leaf.empty(), "shadow tables without fast_shadow");
        return;
    }
    if (d->num_meshes == 0) return;
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        for (int f = M.face_offset; f < M.face_offset + M.face_count; ++f) {
            const int p = T.face_leaf[f];
            CHECK(p >= T.mesh_begin[m] && p < T.mesh_end[m], "face %d: leaf %d outside its mesh", f, p);
            const int leaf = as_int(T.nodes[2 * p + 1].w);
            CHECK(leaf >= 0, "face %d: node %d is no leaf", f, p);
            int first = leaf >> 8, count = leaf & 255;
            if (leaf == rtg::LEAF_EXT) { first = T.node_ext[p].x; count = T.node_ext[p].y; }
            CHECK(f >= first && f < first + count, "face %d: not in leaf %d's range", f, p);
        }
    }
    CHECK(T.ahb_ok && T.ahb.entries == d->num_faces, "any-hit entries %lld, faces %lld", T.ahb.entries,
          (long long)d->num_faces);
    long long bad = 0;
    for (int m = 0; m < d->num_meshes; ++m)
        bad += rtg::ahb_validate(T.anodes, T.ahtris, T.aroot[m], T.nodes, T.node_ext, T.mesh_begin[m], T.mesh_end[m],
                                 T.tris.data());
    CHECK(bad == 0, "any-hit trees: %lld violations", bad);
}

// A device build that hands back the host's own records and face order must give the same
// tables, the six walk / face tables left to the device.
void check_readback(const rtg_scene_desc* d, const rtg::TableOptions& opt, const rtg::SceneTables& T, const Digest& want) {
    rtg::BvhReadback rb;
    rb.nodes = T.nodes; rb.ext = T.node_ext; rb.tris = T.tris;
    rb.perm.resize((size_t)d->num_faces);
    for (size_t f = 0; f < rb.perm.size(); ++f) rb.perm[f] = (int)f;
    rb.mesh_begin = T.mesh_begin; rb.mesh_end = T.mesh_end;
    rb.bigleaf = false;
    for (int i = 0; i < d->num_nodes; ++i) rb.bigleaf |= d->nodes[i].left < 0 && d->nodes[i].count > rtg::kBigLeaf;
    rb.node_count = T.node_count;
    rtg::SceneTables R;
    std::string err;
    CHECK(rtg::build_scene_tables(d, opt, &rb, R, err) == RTG_OK, "read-back build: %s", err.c_str());
    CHECK(R.nodes.empty() && R.node_ext.empty() && R.tris.empty() && R.face_n.empty() && R.face_uv.empty() &&
          R.face_v12.empty(), "read-back build fills a walk table");
    const Digest got = digest(R);
    for (const auto& kv : want) {
        const std::string& k = kv.first;
        if (k == "nodes" || k == "node_ext" || k == "tris" || k == "face_n" || k == "face_uv" || k == "face_v12") continue;
        CHECK(got.at(k) == kv.second, "read-back build: %s differs", k.c_str());
    }
}

}  // namespace

int main(int argc, char** argv) {
    bool print = false;
    std::vector<std::string> paths;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--digest") == 0) print = true;
        else paths.push_back(argv[i]);
    }
    if (paths.empty()) { std::fprintf(stderr, "usage: scene_tables_main [--digest] scene.xml...\n"); return 2; }
    struct Mode { const char* name; bool fast_shadow; rtg::AhbMode ahb; };
    const Mode modes[4] = {{"ref", true, rtg::AHB_REF}, {"exact", true, rtg::AHB_EXACT}, {"split", true, rtg::AHB_SPLIT},
                           {"noshadow", false, rtg::AHB_EXACT}};
    if (print) std::printf("{\n");
    for (size_t s = 0; s < paths.size(); ++s) {
        std::string name = paths[s].substr(paths[s].find_last_of('/') + 1);
        name = name.substr(0, name.rfind('.'));
        g_where = name;
        rtg::HostScene hs;
        std::string err;
        CHECK(hs.load(paths[s], err) == RTG_OK, "load: %s", err.c_str());
        const rtg_scene_desc* d = &hs.desc;
        CHECK(rtg::validate_desc(d, err) == RTG_OK, "validate_desc: %s", err.c_str());
        if (print) std::printf(" \"%s\": {\n", name.c_str());
        for (int k = 0; k < 4; ++k) {
            g_where = name + " (" + modes[k].name + ")";
            rtg::TableOptions opt;
            opt.fast_shadow = modes[k].fast_shadow;
            opt.ahb_mode = modes[k].ahb;
            rtg::SceneTables T;
            CHECK(rtg::build_scene_tables(d, opt, nullptr, T, err) == RTG_OK, "build_scene_tables: %s", err.c_str());
            check_walk(d, T);
            check_objects(d, opt, T);
            check_shadow(d, opt, T);
            const Digest D = digest(T);
            check_readback(d, opt, T, D);
            if (k == 1) {   // without the cooperative walk: FEAT_BIGLEAF cleared, nothing else moves
                rtg::TableOptions lone = opt;
                lone.coop = false;
                rtg::SceneTables L;
                CHECK(rtg::build_scene_tables(d, lone, nullptr, L, err) == RTG_OK, "build_scene_tables: %s", err.c_str());
                check_objects(d, lone, L);
                CHECK(L.feat == (T.feat & ~rtg::FEAT_BIGLEAF), "coop = false: feature bits 0x%x", L.feat);
            }
            if (!print) continue;
            std::printf("  \"%s\": {", modes[k].name);
            const char* sep = "";
            for (const auto& kv : D) { std::printf("%s\"%s\": %s", sep, kv.first.c_str(), kv.second.c_str()); sep = ", "; }
            std::printf("}%s\n", k < 3 ? "," : "");
        }
        if (print) std::printf(" }%s\n", s + 1 < paths.size() ? "," : "");
    }
    if (print) std::printf("}\n");
    return 0;
}
