// Stand-alone dump of the kernel selection (csrc/rtg_variants.hpp), host only: no library, no
// HIP beyond the vector types' header (tests/test_kernel_variants.py builds and runs it).
//
// Prints one JSON object:
//   "mega":  [sk, feat, depth, pt, rr, stats, general, MAXD, PT, SK, FEAT] for every input --
//            the constants with_general / with_special hand their callee, which must be
//            mega_variant's (exit 1 otherwise)
//   "trav":  [feat, FEAT] of with_trav_feat (== trav_feat)
//   "step":  [sk, feat, SK, FEAT] of with_step_variant (== step_variant)
//   "tree":  [sk, SK] of tree_shade_sk
//
// With arguments -- groups of seven integers sk feat depth pt rr stats general -- it prints
// {"mega": [...]} for those inputs alone, rows as above, through the same dispatchers: any depth,
// not only the six of the full table (tests/test_variant_zoo_host.py).
#include <array>
#include <cstdio>
#include <cstdlib>

#include "rtg_variants.hpp"

using namespace rtg;

namespace {

[[noreturn]] void die(const char* what, int a, int b) {
    std::fprintf(stderr, "kernel_variants_main: %s disagrees with its rule at (%d, %d)\n", what, a, b);
    std::exit(1);
}

// one "mega" row: the constants the dispatchers hand their callee for this input
void mega_row(bool first, int sk, int feat, int depth, bool pt, bool rr, bool stats, bool general) {
    const MegaVariant v = mega_variant(depth, pt, rr, sk, feat, stats, general);
    std::array<int, 4> got;
    if (v.special())
        got = with_special(v, [&](auto D, auto K, auto F) {
            return std::array<int, 4>{decltype(D)::value, v.pt, decltype(K)::value, decltype(F)::value};
        });
    else
        got = with_general(v, [](auto D, auto PT) {
            return std::array<int, 4>{decltype(D)::value, decltype(PT)::value, SK_ALL, FEAT_ALL};
        });
    if (got != std::array<int, 4>{v.maxd, v.pt, v.sk, v.feat}) die("with_general / with_special", sk, feat);
    std::printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", first ? "" : ",", sk, feat, depth, pt, rr, stats, general, got[0],
                got[1], got[2], got[3]);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) {
        if ((argc - 1) % 7 != 0) {
            std::fprintf(stderr, "usage: kernel_variants_main [sk feat depth pt rr stats general]...\n");
            return 2;
        }
        std::printf("{\"mega\": [");
        for (int i = 1; i < argc; i += 7) {
            int a[7];
            for (int k = 0; k < 7; ++k) a[k] = std::atoi(argv[i + k]);
            if (a[0] < 0 || a[0] > SK_ALL || a[1] < 0 || a[1] > FEAT_ALL) die("an argument", a[0], a[1]);
            mega_row(i == 1, a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5] != 0, a[6] != 0);
        }
        std::printf("]}\n");
        return 0;
    }
    const int depths[] = {-1, 0, 1, 8, 9, 32};
    std::printf("{\"mega\": [");
    bool first = true;
    for (int sk = 0; sk <= SK_ALL; ++sk)
        for (int feat = 0; feat <= FEAT_ALL; ++feat)
            for (int depth : depths)
                for (int bits = 0; bits < 16; ++bits) {
                    mega_row(first, sk, feat, depth, bits & 1, bits & 2, bits & 4, bits & 8);
                    first = false;
                }
    std::printf("],\n\"trav\": [");
    for (int feat = 0; feat <= FEAT_ALL; ++feat) {
        const int f = with_trav_feat(feat, [](auto F) { return (int)decltype(F)::value; });
        if (f != trav_feat(feat)) die("with_trav_feat", feat, f);
        std::printf("%s[%d,%d]", feat ? "," : "", feat, f);
    }
    std::printf("],\n\"step\": [");
    for (int sk = 0; sk <= SK_ALL; ++sk)
        for (int feat = 0; feat <= FEAT_ALL; ++feat) {
            const StepVariant v = step_variant(sk, feat);
            const std::array<int, 2> got = with_step_variant(sk, feat, [](auto K, auto F) {
                return std::array<int, 2>{decltype(K)::value, decltype(F)::value};
            });
            if (got != std::array<int, 2>{v.sk, v.feat}) die("with_step_variant", sk, feat);
            std::printf("%s[%d,%d,%d,%d]", sk || feat ? "," : "", sk, feat, got[0], got[1]);
        }
    std::printf("],\n\"tree\": [");
    for (int sk = 0; sk <= SK_ALL; ++sk) std::printf("%s[%d,%d]", sk ? "," : "", sk, tree_shade_sk(sk));
    std::printf("],\n\"max_supported_depth\": %d}\n", max_supported_depth());
    return 0;
}
