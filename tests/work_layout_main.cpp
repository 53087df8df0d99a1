// Prints what csrc/work_layout.hpp computes, one JSON array per line, for tests/test_work_layout.py
// to compare with the formulas the render path used before they moved there.  Includes that
// header alone: no HIP, no library.
//   ["wave", pixels, tiles, slots, pay, col, total, off x 13, size x 13]
//   ["pair", have x 5, want x 5, covers, merged x 5]
//   ["defer", pixels, nq, cap, counts, keys, entries, states, total]
//   ["seq", id, step, pixels, nq, reused, laid-out pixels, laid-out nq, cap, counts, keys, ..., total]
#include <cstdio>
#include <vector>

#include "work_layout.hpp"

using rtg::DeferLayout;
using rtg::DeferShape;
using rtg::WaveLayout;
using rtg::WaveShape;

static void put(const WaveShape& s) {
    std::printf("%zu, %zu, %d, %d, %d", s.pixels, s.tiles, s.slots, s.pay, (int)s.col);
}

static void put(const DeferLayout& L) {
    std::printf("%zu, %zu, %zu, %zu, %zu, %zu", L.cap, L.counts, L.keys, L.entries, L.states, L.total);
}

int main() {
    const size_t pixels[] = {1, 160, 255, 256, 257, 480, 511, 512, 513, 960, 1920 * 1080, (size_t)16 << 20};
    const size_t tiles[] = {1, 7, 8, 9, 8160};
    const int slots[] = {0, 1, 2, 5};
    const int pays[] = {0, 2, 3};
    for (size_t p : pixels)
        for (size_t t : tiles)
            for (int s : slots)
                for (int pay : pays)
                    for (int col = 0; col < 2; ++col) {
                        const WaveShape sh{p, t, s, pay, col != 0};
                        const WaveLayout L = rtg::wave_layout(sh);
                        std::printf("[\"wave\", ");
                        put(sh);
                        std::printf(", %zu", L.total);
                        for (int k = 0; k < rtg::WP_COUNT; ++k) std::printf(", %zu", L.off[k]);
                        for (int k = 0; k < rtg::WP_COUNT; ++k) std::printf(", %zu", L.size[k]);
                        std::printf("]\n");
                    }

    // every ordered pair of a small subset, the default-constructed shape (no buffer yet) included
    std::vector<WaveShape> sub(1);
    for (size_t p : {(size_t)160, (size_t)256, (size_t)257})
        for (size_t t : {(size_t)1, (size_t)8})
            for (int s : {0, 1, 2, 5})
                for (int pay : pays)
                    for (int col = 0; col < 2; ++col) sub.push_back({p, t, s, pay, col != 0});
    for (const WaveShape& have : sub)
        for (const WaveShape& want : sub) {
            std::printf("[\"pair\", ");
            put(have);
            std::printf(", ");
            put(want);
            std::printf(", %d, ", (int)have.covers(want));
            put(have.merged(want));
            std::printf("]\n");
        }

    const size_t nqs[] = {0, 256, (size_t)256 * 5 * 8160};
    for (size_t p : pixels)
        for (size_t nq : nqs) {
            std::printf("[\"defer\", %zu, %zu, ", p, nq);
            put(rtg::defer_layout(p, nq));
            std::printf("]\n");
        }

    // a buffer's life over a sequence of requests, as ensure_defer drives it
    const std::vector<std::vector<size_t>> seqs = {{160, 480, 960}, {511, 512, 513}, {513, 512, 511}, {960, 160, 480},
                                                   {1, 512, 160, 513}};
    for (size_t id = 0; id < seqs.size(); ++id)
        for (size_t nq : {(size_t)256, (size_t)2560}) {
            DeferShape have;
            bool allocated = false;
            for (size_t k = 0; k < seqs[id].size(); ++k) {
                // (the shadow-queue entries grow with the request and once shrink, as a scene's would)
                const DeferShape want{seqs[id][k], k == 2 ? nq / 2 : nq * (k + 1)};
                const bool reused = allocated && have.covers(want);
                if (!reused) have = have.merged(want);
                allocated = true;
                std::printf("[\"seq\", %zu, %zu, %zu, %zu, %d, %zu, %zu, ", id * 2 + (nq != 256), k, want.pixels, want.nq,
                            (int)reused, have.pixels, have.nq);
                put(rtg::defer_layout(have.pixels, have.nq));
                std::printf("]\n");
            }
        }
    return 0;
}
