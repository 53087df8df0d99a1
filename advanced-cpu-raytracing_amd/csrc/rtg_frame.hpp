// The frame around the ray trees: camera rays, the miss colour, sample weights and accumulation,
// pixel / tile / work-buffer indexing and the counters' flush.
#pragma once
#include "rtg_shade.hpp"

namespace rtg {

// GenerateRay (raytracer.cpp:661-699) + Camera::GetImagePlanePosition (camera.cpp:74-80)
// MOTION = false (k_shade: the wavefront pipeline never renders a scene with motion blur): the
// motion-blur time is not drawn, mbTime = 0
template <bool MOTION = true>
DEV Ray camera_ray(const DevCamera& C, int px, int py, uint64_t key, float& mbTime) {
    const f3 q = ld3(C.q), right = ld3(C.right), up = ld3(C.up), cpos = ld3(C.pos);
    float su = (float)((px + 0.5) * (double)(C.right_ext - C.left) / C.width);
    float sv = (float)((py + 0.5) * (double)(C.top - C.bottom) / C.height);
    f3 ipp = add(add(q, muls(right, su)), muls(up, -sv));
    Ray ray;
    ray.o = cpos;
    if (C.aperture > 0.0001) {
        f3 aps = ray.o;
        float first01 = 2.0f * rnd(key, RP_DOF, 0) - 1.0f;
        aps = add(aps, muls(up, first01 * C.aperture * 0.5f));
        float second01 = 2.0f * rnd(key, RP_DOF, 1) - 1.0f;
        aps = add(aps, muls(right, second01 * C.aperture * 0.5f));
        f3 dir = makeUnit(sub(ray.o, ipp));
        float tFd = C.focus_distance / dot(dir, ld3(C.gaze));
        f3 bent = add(ray.o, muls(dir, tFd));
        ray.d = makeUnit(sub(bent, aps));
        ray.o = aps;
    } else {
        ray.d = makeUnit(sub(ipp, ray.o));
    }
    mbTime = MOTION ? rnd(key, RP_MOTION, 0) : 0.f;
    return ray;
}

// PerPixel miss branch (raytracer.cpp:49-62)
template <int SK = SK_ALL>
DEV f3 miss_color(const DevScene& S, const DevCamera& C, int px, int py, f3 dir) {
    if ((SK & SK_TEX) && S.bg_texture >= 0) {
        float u = px / (float)C.width, v = py / (float)C.height;
        return tex_rgb(S, S.textures[S.bg_texture], u, v);
    }
    if ((SK & SK_XLIGHT) && S.num_env > 0) return env_sample(S, 0, dir);
    return mk((float)S.background[0], (float)S.background[1], (float)S.background[2]);
}

// Gaussian2D (gaussian.h:3-21) with sigma = 1/6 pixel
DEV float gauss_weight(float x, float y) {
    const float sigma = 1.0f / 6.0f;
    const float sigmaSqr = sigma * sigma;
    const float c1 = (float)(1.0f / (2.0f * RT_PI * sigmaSqr));
    float exponent = (float)(-0.5 * ((x * x + y * y) / sigmaSqr));
    return c1 * expf(exponent);
}

// renderThreadMain's stratified jitter (main.cpp:66-76) feeds only the Gaussian weight;
// samples beyond nRows*nCols keep (0,0) (the reused `samples` vector, main.cpp:47).
DEV float sample_weight(int spp, int s, uint64_t key) {
    const int nRows = (int)sqrt((double)spp);
    const int nCols = nRows;
    float sx = 0.f, sy = 0.f;
    if (s < nRows * nCols) {
        const int row = s / nCols, col = s % nCols;
        float psi1 = rnd(key, RP_JITTER, 0), psi2 = rnd(key, RP_JITTER, 1);
        sx = (col + psi1) / nCols;
        sy = (row + psi2) / nRows;
    }
    return gauss_weight(sx - 0.5f, sy - 0.5f);
}

// x86 cvttss2si + clamp (helperMath.cpp:140-152): out-of-range and NaN give INT_MIN -> 0
DEV unsigned char ldr(float c) {
    int i = (c > -2147483904.0f && c < 2147483648.0f) ? (int)c : (int)0x80000000;
    return (unsigned char)(i < 0 ? 0 : (i > 255 ? 255 : i));
}

// The end of a multi-sample pass for one pixel (RenderParams::slabs): its colours of samples
// sample0, sample0 + 1, ... (col[j * stride]) added to the accumulator one after the other with
// the Gaussian sample weights -- the operations, in the order, of one-sample passes
// (renderThreadMain's spp loop, main.cpp:80-121) -- and after the frame's last sample the pixel
// itself.  first: the pass starts the render's accumulation.
DEV void accum_samples(const DevCamera& C, const RenderParams& P, int sample0, int nslab, bool first, bool last,
                       int pixel, const float4* __restrict__ col, size_t stride, float4* __restrict__ accum,
                       float* __restrict__ hdr, unsigned char* __restrict__ ldrOut) {
    float4 a = first ? make_float4(0.f, 0.f, 0.f, 0.f) : accum[pixel];
    for (int j = 0; j < nslab; ++j) {
        const float4 c = col[j * stride];
        const int s = sample0 + j;
        const float gw = sample_weight(C.spp, s, root_key(P.seed, pixel, s));
        a.x += c.x * gw;
        a.y += c.y * gw;
        a.z += c.z * gw;
        a.w += gw;
    }
    accum[pixel] = a;
    if (last && !P.accum_only) {
        const size_t idx = 3 * (size_t)pixel;
        const float r = a.x / a.w, g = a.y / a.w, b = a.z / a.w;
        if (hdr) { hdr[idx] = r; hdr[idx + 1] = g; hdr[idx + 2] = b; }
        if (ldrOut) { ldrOut[idx] = ldr(r); ldrOut[idx + 1] = ldr(g); ldrOut[idx + 2] = ldr(b); }
    }
}

// 16x16-pixel tile per 256-thread block, 8x8 per wave; tiles dealt so that consecutive
// tiles share an XCD (blocks b and b+8 share one under round-robin dispatch).
// Image row of compact row `crow` of this render's part (RenderParams): compact rows are
// the part's 8-row bands in order.
// Band kb of part p of N is band kb * N + ((p - kb) mod N) of the row range (rtgpu.h
// RTG_PART_BAND_ROWS: round-robin, rotated by one slot per round).
DEV int part_row(const RenderParams& P, int crow) {
    const int kb = crow >> 3;
    int slot = (P.part_index - kb) % P.part_count;
    if (slot < 0) slot += P.part_count;
    return P.row_begin + ((kb * P.part_count + slot) << 3) + (crow & 7);
}
// Image pixel of compact pixel index i (= crow * width + x).
DEV int part_pixel(const RenderParams& P, int width, int i) {
    const int crow = i / width;
    return part_row(P, crow) * width + (i - crow * width);
}

// The ray trees' level-0 order (rtg_tree.hip): compact index i -> image pixel in 8x8 tiles
// (8-row bands of the part, each band's 8-column chunks in order; a band of fewer rows or a
// last chunk of fewer columns keeps its pixels in row-major order), so a wave's 64 camera rays
// -- and, through the per-block ordered child appends, their reflected and refracted rays --
// come from one 8x8 block of the image instead of a 64-pixel strip of a row.  A bijection of
// [0, width * part_rows) onto the part's pixels.  RTG_TREE_TILES=0: row-major (part_pixel).
DEV int tree_pixel(const RenderParams& P, int width, int i) {
    const int band = i / (8 * width), j = i - band * 8 * width;
    const int rb = min(8, P.part_rows - 8 * band);        // rows of this band
    const int fc = width >> 3, full = fc * 8 * rb;         // pixels in whole 8-column chunks
    int x, y;
    if (j < full) {
        const int c = j / (8 * rb), k = j - c * 8 * rb;
        x = 8 * c + (k & 7);
        y = k >> 3;
    } else {
        const int rw = width & 7, k = j - full;
        x = 8 * fc + k % rw;
        y = k / rw;
    }
    return part_row(P, 8 * band + y) * width + x;
}

// tile_pixel also returns the compact row and the block's sample slab (multi-sample passes,
// RenderParams::slabs): the pixel's work-buffer entry is slab * slab_px + crow * width + px
// (work_index).  A padding block of a slab (its index past num_tiles) holds no pixel: px is
// past every image width.
DEV void tile_pixel(const RenderParams& P, int& px, int& py, int& crow, int& slab) {
    slab = (int)(blockIdx.x / (unsigned)P.slab_tiles);
    const int b = (int)blockIdx.x - slab * P.slab_tiles;
    if (b >= P.num_tiles) {
        px = 1 << 24;
        crow = 0;
        py = P.row_end;
        return;
    }
    const int tile = P.tile_map[b];
    const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    px = tx * 16 + (w & 1) * 8 + (l & 7);
    crow = ty * 16 + (w >> 1) * 8 + (l >> 3);
    py = part_row(P, crow);
}
DEV void tile_pixel(const RenderParams& P, int& px, int& py) {
    int crow, slab;
    tile_pixel(P, px, py, crow, slab);
}
DEV int work_index(const RenderParams& P, int width, int slab, int crow, int px) {
    return slab * P.slab_px + crow * width + px;
}
// The image pixel of work-buffer entry i of sample slab `slab` (inverse of work_index).
DEV int work_pixel(const RenderParams& P, int width, int slab, int i) {
    const int r = i - slab * P.slab_px, crow = r / width;
    return part_row(P, crow) * width + (r - crow * width);
}

template <bool STATS>
DEV void flush_counters(Cnt<STATS>& cn, DevCounters* counters) {
    if constexpr (STATS) {
        unsigned long long v[13] = {cn.cams, cn.secs, cn.shds, cn.nodes, cn.tris, cn.sphs, cn.objs, cn.snodes, cn.stris,
                                    cn.wnodes, cn.fallbacks, cn.ewnodes, cn.efallbacks};
        for (int k = 0; k < 13; ++k) {
            unsigned long long x = v[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
            if ((threadIdx.x & 63) == 0 && x) atomicAdd(&((unsigned long long*)counters)[k], x);
        }
    }
}

}  // namespace rtg
