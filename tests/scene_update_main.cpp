// Stand-alone check of update_scene_tables (csrc/scene_tables.cpp), host only: links host_xml.cpp
// host_scene.cpp host_assets.cpp scene_tables.cpp rtg_ahb.cpp -lz, neither the library nor HIP
// (tests/test_scene_update.py builds and runs it).
//
//   scene_update_main <command>...
//     pair NAME A.xml B.xml        B must keep A's geometry; the update of A's kept state to B must
//                                  give, byte for byte, the mutable tables and scalars of
//                                  build_scene_tables(B), in the ref, exact and no-shadow modes, and
//                                  must be refused where A's any-hit trees are split ones
//     refuse NAME A.xml B.xml CODE the update of A's kept state to B must return CODE
//     refuse-mesh NAME A.xml       ... to A with one object's mesh index changed: RTG_ERR_INVALID
//
// Exit 1 with a message on the first violation; one line per check on stdout otherwise.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_scene.hpp"
#include "scene_tables.hpp"

namespace {

std::string g_where;

[[noreturn]] void die(const char* fmt, ...) {
    std::fprintf(stderr, "scene_update_main: %s: ", g_where.c_str());
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) die(__VA_ARGS__); } while (0)

// FNV-1a, 64 bit, over the byte count and then the bytes
uint64_t fnv64(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    h = (h ^ (uint64_t)n) * 1099511628211ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

template <typename V>
bool same_bytes(const V& a, const V& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

void load(rtg::HostScene& hs, const char* path) {
    std::string err;
    CHECK(hs.load(path, err) == RTG_OK, "load %s: %s", path, err.c_str());
    CHECK(rtg::validate_desc(&hs.desc, err) == RTG_OK, "validate_desc %s: %s", path, err.c_str());
}

// `d` without what an update may not read: faces, nodes and texels are null
struct Stripped {
    rtg_scene_desc desc;
    std::vector<rtg_image> images;
    explicit Stripped(const rtg_scene_desc& d) : desc(d), images(d.images, d.images + d.num_images) {
        for (rtg_image& im : images) im.texels = nullptr;
        desc.images = images.data();
        desc.faces = nullptr;
        desc.nodes = nullptr;
    }
};

struct Mode { const char* name; bool fast_shadow; rtg::AhbMode ahb; };
const Mode kModes[4] = {{"ref", true, rtg::AHB_REF}, {"exact", true, rtg::AHB_EXACT}, {"noshadow", false, rtg::AHB_EXACT},
                        {"split", true, rtg::AHB_SPLIT}};

rtg::TableOptions options(const Mode& m) {
    rtg::TableOptions opt;
    opt.fast_shadow = m.fast_shadow;
    opt.ahb_mode = m.ahb;
    return opt;
}

void check_pair(const char* name, const char* pa, const char* pb) {
    g_where = name;
    rtg::HostScene A, B;
    load(A, pa);
    load(B, pb);
    const rtg_scene_desc *da = &A.desc, *db = &B.desc;
    // the premise: the same faces and nodes, byte for byte
    CHECK(da->num_faces == db->num_faces && da->num_nodes == db->num_nodes, "premise: %lld faces / %lld nodes against %lld / %lld",
          (long long)da->num_faces, (long long)da->num_nodes, (long long)db->num_faces, (long long)db->num_nodes);
    CHECK(da->num_faces == 0 || std::memcmp(da->faces, db->faces, (size_t)da->num_faces * sizeof(rtg_face)) == 0,
          "premise: faces differ");
    CHECK(da->num_nodes == 0 || std::memcmp(da->nodes, db->nodes, (size_t)da->num_nodes * sizeof(rtg_bvh_node)) == 0,
          "premise: nodes differ");
    const Stripped sb(*db);
    for (const Mode& m : kModes) {
        g_where = std::string(name) + " (" + m.name + ")";
        const rtg::TableOptions opt = options(m);
        rtg::SceneTables TA, TB, U;
        rtg::KeptTables K;
        std::string err;
        CHECK(rtg::build_scene_tables(da, opt, nullptr, TA, err) == RTG_OK, "build A: %s", err.c_str());
        CHECK(rtg::build_scene_tables(db, opt, nullptr, TB, err) == RTG_OK, "build B: %s", err.c_str());
        rtg::keep_tables(da, TA, K);
        CHECK(rtg::same_geometry(db, K, err) == RTG_OK, "premise: signature: %s", err.c_str());
        const int rc = rtg::update_scene_tables(&sb.desc, K, opt, U, err);
        if (TA.ahb_split) {
            CHECK(rc == RTG_ERR_UNSUPPORTED, "split any-hit trees: update returned %d", rc);
            std::printf("%s %s refused\n", name, m.name);
            continue;
        }
        CHECK(rc == RTG_OK, "update: %d %s", rc, err.c_str());
        // what stays on the device is what a fresh build of B would upload
        CHECK(same_bytes(TA.nodes, TB.nodes) && same_bytes(TA.node_ext, TB.node_ext) && same_bytes(TA.tris, TB.tris) &&
              same_bytes(TA.face_n, TB.face_n) && same_bytes(TA.face_uv, TB.face_uv) && same_bytes(TA.face_v12, TB.face_v12),
              "kept walk / face tables differ from B's");
        CHECK(same_bytes(TA.anodes, TB.anodes) && same_bytes(TA.ahtris, TB.ahtris) && same_bytes(TA.face_leaf, TB.face_leaf),
              "kept any-hit trees differ from B's");
        CHECK(same_bytes(TA.light_faces, TB.light_faces) && same_bytes(TA.texels, TB.texels) &&
              same_bytes(TA.perm, TB.perm) && same_bytes(TA.grad, TB.grad), "kept light faces / texels / noise tables differ");
        const size_t nmix = TA.env_mix.size() < TB.env_mix.size() ? TA.env_mix.size() : TB.env_mix.size();
        CHECK(nmix == 0 || std::memcmp(TA.env_mix.data(), TB.env_mix.data(), nmix * 8) == 0,
              "env_mix is no prefix of the other scene's");
        // every mutable table and scalar
        uint64_t h = 1469598103934665603ull;
#define TAB(t) do { CHECK(same_bytes(U.t, TB.t), #t " differs (%zu entries, B has %zu)", U.t.size(), TB.t.size()); \
                    h = fnv64(h, U.t.data(), U.t.size() * sizeof(U.t[0])); } while (0)
        TAB(objects); TAB(group_box); TAB(materials); TAB(brdfs); TAB(textures); TAB(images);
        TAB(point_lights); TAB(area_lights); TAB(dir_lights); TAB(spot_lights); TAB(env_images); TAB(env_mix);
        TAB(mesh_lights); TAB(mesh_begin); TAB(mesh_end); TAB(aroot);
#undef TAB
#define NUM(s) do { CHECK(U.s == TB.s, #s " %d, B has %d", (int)U.s, (int)TB.s); \
                    const int v_ = (int)U.s; h = fnv64(h, &v_, sizeof(v_)); } while (0)
        NUM(feat); NUM(shade_sk); NUM(num_slots); NUM(wave_ok); NUM(tree_ok); NUM(path_ok);
        NUM(ahb_mode); NUM(ahb_split); NUM(ahb_ok); NUM(bigleaf);
#undef NUM
        CHECK(U.nodes.empty() && U.tris.empty() && U.texels.empty() && U.anodes.empty() && U.light_faces.empty() &&
              U.face_leaf.empty(), "update fills a geometry table");
        std::printf("%s %s %016llx\n", name, m.name, (unsigned long long)h);
    }
}

// exact mode: the update of A's kept state to `d` must return `code` and leave U untouched
void check_refused(const char* name, const rtg_scene_desc* da, const rtg_scene_desc* d, int code) {
    const rtg::TableOptions opt = options(kModes[1]);
    rtg::SceneTables TA, U;
    rtg::KeptTables K;
    std::string err;
    CHECK(rtg::build_scene_tables(da, opt, nullptr, TA, err) == RTG_OK, "build A: %s", err.c_str());
    rtg::keep_tables(da, TA, K);
    U.num_slots = -7;
    const int rc = rtg::update_scene_tables(d, K, opt, U, err);
    CHECK(rc == code, "update returned %d (%s), expected %d", rc, err.c_str(), code);
    CHECK(!err.empty() && U.num_slots == -7 && U.objects.empty(), "a refused update wrote its output");
    std::printf("%s refused %d\n", name, rc);
}

}  // namespace

int main(int argc, char** argv) {
    int i = 1;
    auto arg = [&]() -> const char* {
        if (i >= argc) { std::fprintf(stderr, "scene_update_main: missing argument\n"); std::exit(2); }
        return argv[i++];
    };
    if (argc < 2) { std::fprintf(stderr, "usage: scene_update_main (pair|refuse|refuse-mesh) ...\n"); return 2; }
    while (i < argc) {
        const std::string cmd = arg();
        const char* name = arg();
        g_where = name;
        if (cmd == "pair") {
            const char* a = arg();
            const char* b = arg();
            check_pair(name, a, b);
        } else if (cmd == "refuse") {
            const char* a = arg();
            const char* b = arg();
            const int code = std::atoi(arg());
            rtg::HostScene A, B;
            load(A, a);
            load(B, b);
            check_refused(name, &A.desc, &B.desc, code);
        } else if (cmd == "refuse-mesh") {
            rtg::HostScene A;
            load(A, arg());
            CHECK(A.desc.num_meshes >= 2, "needs two meshes");
            std::vector<rtg_object> objs(A.desc.objects, A.desc.objects + A.desc.num_objects);
            size_t k = 0;
            while (k < objs.size() && objs[k].kind == RTG_OBJ_SPHERE) ++k;
            CHECK(k < objs.size(), "needs a mesh object");
            objs[k].mesh = (objs[k].mesh + 1) % A.desc.num_meshes;
            rtg_scene_desc d = A.desc;
            d.objects = objs.data();
            check_refused(name, &A.desc, &d, RTG_ERR_INVALID);
        } else {
            std::fprintf(stderr, "scene_update_main: unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
