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

}  // namespace

int main() {
    const int depths[] = {-1, 0, 1, 8, 9, 32};
    std::printf("{\"mega\": [");
    bool first = true;
    for (int sk = 0; sk <= SK_ALL; ++sk)
        for (int feat = 0; feat <= FEAT_ALL; ++feat)
            for (int depth : depths)
                for (int bits = 0; bits < 16; ++bits) {
                    const bool pt = bits & 1, rr = bits & 2, stats = bits & 4, general = bits & 8;
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
                    std::printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", first ? "" : ",", sk, feat, depth, pt, rr, stats,
                                general, got[0], got[1], got[2], got[3]);
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
