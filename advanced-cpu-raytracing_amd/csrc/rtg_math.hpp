// Device maths shared by every kernel: the force-inline qualifier and the guarded table index,
// the reference's vector helpers (helperMath.cpp), the counter-based RNG and the stats counters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtg_device.hpp"

namespace rtg {

#define DEV __device__ __forceinline__

// RTG_GUARD=1 (fault-hunting builds only): every table index taken from a hit record or an
// object, and the fused kernel's frame-stack index, is range-checked; a bad one sets bit
// `code` of S.guard[0] (printed by rtg_scene_destroy) and is clamped so the run goes on.
#ifndef RTG_GUARD
#define RTG_GUARD 0
#endif
#if RTG_GUARD
#define GIDX(S, i, n, code) \
    ([&]() -> int { const int i_ = (i); if (i_ < 0 || i_ >= (n)) { atomicOr((S).guard, 1 << (code)); return 0; } return i_; }())
#else
#define GIDX(S, i, n, code) (i)
#endif

// ---------------------------------------------------------------------------
// helperMath.cpp
// ---------------------------------------------------------------------------
struct f3 { float x, y, z; };
DEV f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
DEV f3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }
DEV f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEV f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEV f3 mulv(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
DEV f3 muls(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
DEV f3 divs(f3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
DEV f3 neg(f3 a) { return mk(a.x * -1.0f, a.y * -1.0f, a.z * -1.0f); }
DEV float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DEV f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
DEV float len(f3 a) { return sqrtf((a.x * a.x) + (a.y * a.y) + (a.z * a.z)); }
DEV f3 makeUnit(f3 a) { float l = len(a); return mk(a.x / l, a.y / l, a.z / l); }
DEV float fmax0(float v) { return (0.0f < v) ? v : 0.0f; }          // std::max(0.0f, v)

DEV void onb(f3 r, f3& u, f3& v) {                                     // helperMath.cpp:59-85
    float ax = fabsf(r.x), ay = fabsf(r.y), az = fabsf(r.z);
    f3 rp = r;
    if (ax < ay) { if (ax < az) rp.x = 1.0f; else rp.z = 1.0f; }
    else { if (ay < az) rp.y = 1.0f; else rp.z = 1.0f; }
    u = makeUnit(cross(rp, r));
    v = makeUnit(cross(r, u));
}

#define RT_PI 3.14159265358979323846
DEV double angleBetween(f3 a, f3 b) {                                  // helperMath.cpp:154-157
    float d = dot(a, b);
    float c = (-1.0f < d) ? d : -1.0f;      // std::max(-1.0f, d)
    c = (c < 1.0f) ? c : 1.0f;              // std::min(1.0f, c)
    return (double)acosf(c) * (double)(180.0f / RT_PI);
}
DEV double cosDeg(double a) { return cos(a * (RT_PI / 180.0f)); }      // helperMath.cpp:158-161

// matrix.hpp:56-81 (double accumulation, w column included)
DEV f3 xform(const double* m, f3 v, float w) {
    return mk((float)(m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3] * w),
              (float)(m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7] * w),
              (float)(m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11] * w));
}

// counter-based RNG (replaces the shared mt19937 streams; keyed by pixel, sample and
// ray-tree node so results do not depend on thread / GPU count)
DEV uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
DEV float rnd(uint64_t key, uint32_t purpose, uint32_t idx) {
    uint64_t h = mix64(key ^ mix64(((uint64_t)purpose << 32) | idx));
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}
DEV uint64_t child_key(uint64_t key, int slot) { return mix64(key + 0x632BE59BD9B4E019ULL * (uint64_t)(slot + 1)); }
DEV uint64_t root_key(uint64_t seed, int pixel, int sample) {
    return mix64(mix64(seed ^ 0xD1B54A32D192ED03ULL) ^ ((uint64_t)(uint32_t)pixel * 0x9E3779B97F4A7C15ULL) ^
                 ((uint64_t)(uint32_t)sample << 1));
}
// double draw (std::uniform_real_distribution<> of MeshLight::getSample, meshLight.h:31-36)
DEV double rndd(uint64_t key, uint32_t purpose, uint32_t idx) {
    uint64_t h = mix64(key ^ mix64(((uint64_t)purpose << 32) | idx));
    return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}
enum { RP_MOTION = 1, RP_DOF = 2, RP_JITTER = 3, RP_AREA = 4, RP_ENV = 5, RP_ROUGH_REFL = 6, RP_ROUGH_REFR = 7,
       RP_GI = 8, RP_MESHLIGHT = 9 };

// ---------------------------------------------------------------------------
// Counters
// ---------------------------------------------------------------------------
template <bool STATS> struct Cnt {
    template <bool ANY> DEV void node() {}
    template <bool ANY> DEV void tri() {}
    template <bool ANY> DEV void tri_n(uint32_t) {}
    DEV void sph() {} DEV void obj() {}
    DEV void cam() {} DEV void sec() {} DEV void shd() {}
    DEV void wnode() {}
    DEV void fallback() {}
    DEV void ewnode() {}
    DEV void efallback() {}
};
template <> struct Cnt<true> {
    uint32_t nodes = 0, tris = 0, sphs = 0, objs = 0, cams = 0, secs = 0, shds = 0, snodes = 0, stris = 0, wnodes = 0,
             fallbacks = 0, ewnodes = 0, efallbacks = 0;
    DEV void wnode() { ++wnodes; }
    DEV void ewnode() { ++ewnodes; }
    DEV void efallback() { ++efallbacks; }
    DEV void fallback() { ++fallbacks; }
    template <bool ANY> DEV void node() { if (ANY) ++snodes; else ++nodes; }
    template <bool ANY> DEV void tri() { if (ANY) ++stris; else ++tris; }
    template <bool ANY> DEV void tri_n(uint32_t n) { if (ANY) stris += n; else tris += n; }
    DEV void sph() { ++sphs; } DEV void obj() { ++objs; }
    DEV void cam() { ++cams; } DEV void sec() { ++secs; } DEV void shd() { ++shds; }
};

}  // namespace rtg
