// The fused kernel's device code and its launchers (rtg_mega.hip, rtg_mega_pt.hip,
// rtg_mega_wh.hip; the ray tree also rtg_radiance.hip's): one thread per pixel walks
// the pixel's whole ray tree -- PerformShading (raytracer.cpp:65-134) with the recursion of
// ComputeMirrorReflection / ...Dielectric... / ...Conductor... and, for path-tracing cameras,
// ComputeGlobalIllumination (raytracer.cpp:135-191) unrolled onto an explicit per-thread stack.
#pragma once

#include "rtg_common.hpp"
#include "rtg_node.hpp"
#include "rtg_variants.hpp"

namespace rtg {

// ---------------------------------------------------------------------------
// Whole ray tree of one pixel sample; returns RenderPixel's colour
// (raytracer.cpp:38-63).  A single trace call site: the loop holds one pending ray
// (camera ray, a frame's first child, a dielectric frame's refracted child, or a path
// tracing node's GI ray).  The node steps (shade_node, resume_frame) are rtg_node.hpp's,
// shared with the wavefront path-tracing pipeline.
// SK / FEAT: the scene's shading and traversal features (a superset; the path-tracing
// and ray-tree variants of rtg_variants.hpp mega_variant), everything by default.
// SRC: where the primary ray comes from.  CameraRay (a render): GenerateRay's ray of the pixel,
// unbounded, its primary hit seen from the camera's position (also for depth-of-field rays).
// GivenRay (radiance queries, render_ray below): a caller's ray -- `tmax` bounds the primary ray
// only (the walk's initial minT), `eye` is the viewer of the primary hit, *tprim receives the
// primary ray's accepted distance (tmax on a miss); of C the tree then reads the renderer flags
// and, in miss_color, width / height, (px, py) being the pixel of the background-texture lookup.
// The split is compile-time so that k_render compiles to what it was without it
// (profiles/r08_render_resources.txt).
struct CameraRay { static constexpr bool given = false; };
struct GivenRay {
    static constexpr bool given = true;
    Ray ray;
    float mbTime, tmax;
    f3 eye;
    float* tprim;
};

template <int MAXD, bool STATS, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL, class SRC = CameraRay>
DEV f3 render_sample(const DevScene& S, const DevCamera& C, int px, int py, uint64_t key, Cnt<STATS>& cn,
                     const SRC src = SRC()) {
    float mbTime;
    Pending p;
    f3 cpos;
    if constexpr (SRC::given) {
        p.R = src.ray;
        mbTime = src.mbTime;
        cpos = src.eye;
    } else {
        p.R = camera_ray(C, px, py, key, mbTime);
        cpos = ld3(C.pos);
        cn.cam();
    }
    p.medium = 1.0f;
    p.depth = S.max_depth;
    p.key = key;
    p.tp = mk(1.0f, 1.0f, 1.0f);
    p.pend = 0;

    FrameT<PT> stack[MAXD > 0 ? MAXD : 1];
    int sp = 0;
    ChildVal v;
    v.t = 0.f;
    v.medium = 1.f;
    for (;;) {
        Node cur;
        float minT = INFINITY;
        if constexpr (SRC::given) minT = p.pend == 0 ? src.tmax : INFINITY;
        const bool hit = trace<false, STATS, FEAT>(S, p.R, mbTime, minT, INFINITY, cur.h, cn);
        if constexpr (SRC::given) {
            if (p.pend == 0) *src.tprim = cur.h.t;
        }
        if (p.pend == 0 && !hit) return miss_color<SK>(S, C, px, py, p.R.d);
        if constexpr (PT) {
            if (p.pend == 3) stack[GIDX(S, sp - 1, MAXD, 9)].skip = emissive_hit_id(S, cur.h, hit);
        }
        if (hit) {
            cur.r = p.R;
            cur.eye = p.pend == 0 ? cpos : p.R.o;
            cur.medium = p.medium;
            cur.mbTime = mbTime;
            cur.depth = p.depth;
            cur.key = p.key;
            cur.tp = p.tp;
            // ---- shade; a node with children pushes a frame and continues with its first child
            Child ch;
            const bool spawn = shade_node<MAXD, STATS, PT, SK, FEAT>(S, C, cur, sp, v.value,
                                                           stack[MAXD > 0 ? GIDX(S, sp, MAXD, 10) : 0], ch, cn);
            if (MAXD > 0 && spawn) {
                spawn_child<STATS, PT>(stack[GIDX(S, sp, MAXD, 11)], ch, p, cn);
                ++sp;
                continue;
            }
            v.hit = true;
            v.t = cur.h.t;
            v.medium = cur.medium;
        } else {
            v.value = miss_value<PT, SK>(S, stack[MAXD > 0 ? GIDX(S, sp - 1, MAXD, 12) : 0], p.R.d);
            v.hit = false;
        }
        // ---- propagate finished values up the stack
        bool descended = false;
        while (MAXD > 0 && sp > 0) {
            if (resume_frame<STATS, PT, SK, FEAT>(S, C, stack[GIDX(S, sp - 1, MAXD, 13)], v, p, cn)) {
                descended = true;
                break;
            }
            --sp;
        }
        if (!descended) return v.value;
    }
}

// The ray tree below a given primary ray (k_radiance): render_sample from the loop on.
template <int MAXD, bool STATS, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL>
DEV f3 render_ray(const DevScene& S, const DevCamera& C, const Ray& ray, float mbTime, float tmax, f3 eye, int px, int py,
                  uint64_t key, Cnt<STATS>& cn, float& tprim) {
    return render_sample<MAXD, STATS, PT, SK, FEAT, GivenRay>(S, C, px, py, key, cn, GivenRay{ray, mbTime, tmax, eye, &tprim});
}

template <int MAXD, bool STATS, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL>
__global__ __launch_bounds__(256, RTG_MEGA_WAVES) void k_render(DevScene S, DevCamera C, RenderParams P, float* __restrict__ hdr,
                                                unsigned char* __restrict__ ldrOut, float* __restrict__ accum,
                                                DevCounters* __restrict__ counters) {
    int px, py;
    tile_pixel(P, px, py);
    Cnt<STATS> cn;
    if (px < C.width && py < P.row_end) {
        const int pixel = px + py * C.width;
        f3 color;
        if (C.spp <= 1 && !P.accum_only) {
            color = render_sample<MAXD, STATS, PT, SK, FEAT>(S, C, px, py, root_key(P.seed, pixel, 0), cn);
        } else {
            // renderThreadMain multisampling (main.cpp:60-101): stratified jitter only
            // feeds the Gaussian weights; every sample traces the pixel centre.
            f3 acc = mk(0, 0, 0);
            float sumW = 0.0f;
            for (int s = P.sample_begin; s < P.sample_begin + P.sample_count; ++s) {
                const uint64_t key = root_key(P.seed, pixel, s);
                const float gw = sample_weight(C.spp, s, key);
                f3 col = render_sample<MAXD, STATS, PT, SK, FEAT>(S, C, px, py, key, cn);
                acc.x += col.x * gw;
                acc.y += col.y * gw;
                acc.z += col.z * gw;
                sumW += gw;
            }
            if (P.accum_only) {
                float4* a4 = reinterpret_cast<float4*>(accum);
                a4[pixel] = make_float4(acc.x, acc.y, acc.z, sumW);
                color = mk(0, 0, 0);
            } else {
                color = mk(acc.x / sumW, acc.y / sumW, acc.z / sumW);
            }
        }
        if (!P.accum_only) {
            const size_t idx = 3 * (size_t)pixel;
            if (hdr) { hdr[idx] = color.x; hdr[idx + 1] = color.y; hdr[idx + 2] = color.z; }
            if (ldrOut) { ldrOut[idx] = ldr(color.x); ldrOut[idx + 1] = ldr(color.y); ldrOut[idx + 2] = ldr(color.z); }
        }
    }
    flush_counters<STATS>(cn, counters);
}

// ---------------------------------------------------------------------------
// Host-side launch helpers
// ---------------------------------------------------------------------------
template <int MAXD, bool STATS, bool PT, int SK = SK_ALL, int FEAT = FEAT_ALL>
hipError_t launch_render(const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr, unsigned char* l,
                         float* accum, DevCounters* cnt, hipStream_t stream) {
    hipLaunchKernelGGL((k_render<MAXD, STATS, PT, SK, FEAT>), dim3(P.num_tiles), dim3(256), 0, stream, S, C, P, hdr, l,
                       accum, cnt);
    return hipGetLastError();
}

// The feature-specialised sets of one renderer (rtg_mega_pt.hip: PT, rtg_mega_wh.hip: ray trees;
// heavy to compile, so one translation unit each)
template <bool PT>
hipError_t launch_special(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr,
                          unsigned char* l, float* accum, DevCounters* cnt, hipStream_t stream) {
    return with_special(v, [&](auto D, auto K, auto F) {
        return launch_render<decltype(D)::value, false, PT, decltype(K)::value, decltype(F)::value>(S, C, P, hdr, l, accum,
                                                                                                     cnt, stream);
    });
}

}  // namespace rtg
