// Which child-slot patterns the any-hit trees of a scene contain (tests/test_gpu_node_loops.py
// builds and runs it), host only: links host_xml.cpp host_scene.cpp host_assets.cpp
// scene_tables.cpp rtg_ahb.cpp -lz, neither the library nor HIP.
//
//   wide_slots_main scene.xml...
//
// Builds each scene's tables as rtg_scene_create does by default and prints one JSON object
// {scene: {"nodes": wide nodes, "depth": levels, "fanout": [nodes with 1, 2, 3, 4 children],
//          "patterns": {"LIE-": count, ...}}}: a pattern is the node's four slots in order,
// L a leaf slot, I an inner (wide-node) slot, - an empty one.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "host_scene.hpp"
#include "scene_tables.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: wide_slots_main scene.xml...\n"); return 2; }
    std::printf("{\n");
    for (int s = 1; s < argc; ++s) {
        std::string path = argv[s], name = path.substr(path.find_last_of('/') + 1);
        name = name.substr(0, name.rfind('.'));
        rtg::HostScene hs;
        std::string err;
        if (hs.load(path, err) != RTG_OK) { std::fprintf(stderr, "%s: load: %s\n", name.c_str(), err.c_str()); return 1; }
        rtg::SceneTables T;
        if (rtg::build_scene_tables(&hs.desc, rtg::TableOptions(), nullptr, T, err) != RTG_OK) {
            std::fprintf(stderr, "%s: build_scene_tables: %s\n", name.c_str(), err.c_str());
            return 1;
        }
        std::map<std::string, long long> patterns;
        long long fanout[4] = {0, 0, 0, 0};
        for (const rtg::WNode& n : T.anodes) {
            const int c[4] = {n.child.x, n.child.y, n.child.z, n.child.w};
            std::string p;
            int live = 0;
            for (int k = 0; k < 4; ++k) {
                p += c[k] == rtg::WCHILD_EMPTY ? '-' : (c[k] >= 0 ? 'I' : 'L');
                live += c[k] != rtg::WCHILD_EMPTY;
            }
            ++patterns[p];
            if (live > 0) ++fanout[live - 1];
        }
        std::printf(" \"%s\": {\"nodes\": %zu, \"depth\": %d, \"fanout\": [%lld, %lld, %lld, %lld], \"patterns\": {",
                    name.c_str(), T.anodes.size(), (int)T.ahb.max_depth, fanout[0], fanout[1], fanout[2], fanout[3]);
        bool first = true;
        for (const auto& kv : patterns) {
            std::printf("%s\"%s\": %lld", first ? "" : ", ", kv.first.c_str(), kv.second);
            first = false;
        }
        std::printf("}}%s\n", s + 1 < argc ? "," : "");
    }
    std::printf("}\n");
    return 0;
}
