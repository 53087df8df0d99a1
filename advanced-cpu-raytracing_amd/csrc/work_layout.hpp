// The two carved work buffers of the wavefront pipeline (rtg_api.cpp ensure_wave / ensure_defer)
// as pure functions of their shapes: what a buffer was laid out for, when it can be reused, how
// it grows, and the byte offset of every piece.  std only: no HIP call, no HIP type.
#pragma once
#include <algorithm>
#include <cstddef>

namespace rtg {

// What the wavefront buffers are sized for: `pixels` pixel entries x `slots` light slots, `tiles`
// shade blocks (queue segments of 256 * slots entries), `pay` one-layout payload float4s per
// queue entry, `col`: with the colour buffer of multi-sample passes (one float4 per entry).
struct WaveShape {
    size_t pixels = 0, tiles = 0;
    int slots = 0;
    int pay = 0;
    bool col = false;
    // buffers of this shape serve a render that wants `w`
    bool covers(const WaveShape& w) const {
        return pixels >= w.pixels && slots >= w.slots && tiles >= w.tiles && pay >= w.pay && (col || !w.col);
    }
    // the shape to grow to for `w`: nothing but the slots (the scene's as it is now) shrinks
    WaveShape merged(const WaveShape& w) const {
        return {std::max(pixels, w.pixels), std::max(tiles, w.tiles), w.slots, std::max(pay, w.pay), col || w.col};
    }
};

enum WavePiece {
    WP_HIT_T, WP_HIT_OBJ, WP_HIT_FACE, WP_BASE, WP_TERM, WP_OCC, WP_Q_O, WP_Q_D, WP_Q_SLOT, WP_Q_COUNT, WP_ACCUM,
    WP_Q_PAY, WP_COL, WP_COUNT
};
struct WaveLayout {
    size_t off[WP_COUNT], size[WP_COUNT];   // bytes; every offset a multiple of 256
    size_t total;
};

inline WaveLayout wave_layout(const WaveShape& s) {
    const size_t slots = (size_t)std::max(s.slots, 1);
    const size_t ns = s.pixels * slots;            // (pixel, light slot) entries
    const size_t nq = s.tiles * 256 * slots;       // shadow-ray queue entries
    WaveLayout L{};
    L.size[WP_HIT_T] = s.pixels * 4;
    L.size[WP_HIT_OBJ] = s.pixels * 4;
    L.size[WP_HIT_FACE] = s.pixels * 4;
    L.size[WP_BASE] = s.pixels * 16;
    L.size[WP_TERM] = ns * 16;
    L.size[WP_OCC] = ns;
    L.size[WP_Q_O] = nq * 16;
    L.size[WP_Q_D] = nq * 16;
    L.size[WP_Q_SLOT] = nq * 4;
    L.size[WP_Q_COUNT] = s.tiles * 4;
    L.size[WP_ACCUM] = s.pixels * 16;
    L.size[WP_Q_PAY] = s.tiles * 256 * 16 * (size_t)s.pay;
    L.size[WP_COL] = s.col ? s.pixels * 16 : 0;
    for (int k = 0; k < WP_COUNT; ++k) {
        L.off[k] = L.total;
        L.total += (L.size[k] + 255) & ~(size_t)255;
    }
    return L;
}

// The deferred-leaf queue of a large-leaf scene's camera walk (WaveBufs dq_*, hit_key): two
// entries per pixel of capacity, 1 024 at least (an entry that does not fit is tested in the walk).
// Layout [256 B counts | pixels x 8 B keys | cap x 48 B entries | nq x 4 B states]: the entry
// and state offsets depend on the pixel count, so a buffer laid out for fewer pixels is never
// reused (the 1 024-entry floor on cap alone would let keys overrun the entries).
struct DeferShape {
    size_t pixels = 0, nq = 0;
    bool covers(const DeferShape& w) const { return pixels >= w.pixels && nq >= w.nq; }
    DeferShape merged(const DeferShape& w) const { return {std::max(pixels, w.pixels), std::max(nq, w.nq)}; }
};
struct DeferLayout {
    size_t cap;                                    // queue entries
    size_t counts, keys, entries, states, total;   // bytes
};

inline DeferLayout defer_layout(size_t pixels, size_t nq) {
    DeferLayout L{};
    L.cap = std::max<size_t>(2 * pixels, 1024);
    L.counts = 0;
    L.keys = 256;
    L.entries = L.keys + pixels * 8;
    L.states = L.entries + L.cap * 48;
    L.total = L.states + nq * 4;
    return L;
}

}  // namespace rtg
