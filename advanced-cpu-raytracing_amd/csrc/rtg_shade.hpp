// From a hit to a colour: surface reconstruction, textures, normal and bump maps, environment
// sampling, the BRDFs, Shade, light sampling and direct lighting with its shadow rays.
#pragma once
#include "rtg_walk.hpp"

namespace rtg {

// ---------------------------------------------------------------------------
// Hit reconstruction: normal / uv of the winning primitive
// ---------------------------------------------------------------------------
DEV float tiledUV(float x) {                                           // mesh.cpp:382-389
    if (x > 1.0001f) {
        x = x - floorf(x);
        if (x < 0.0001) x = 1.0f;
    }
    return x;
}

struct Surf {
    f3 p, n;
    float u, v;
};

// ---------------------------------------------------------------------------
// Textures (imageTexture.h, perlinTexture.h) and environment light
// ---------------------------------------------------------------------------
DEV f3 texel(const DevScene& S, const DevImage& im, int i, int j) {     // LDRImage.h:16-26
    const long long idx = (long long)im.channels * ((long long)i + (long long)j * im.width);
    const long long n = (long long)im.width * im.height * im.channels;
    const float* t = S.texels + im.offset;
    // linear indexing as in the reference (an x+1 read at the last column takes the next
    // row's first texel); reads outside the image, undefined in the reference, give 0
    return mk((idx >= 0 && idx < n) ? t[idx] : 0.f, (idx + 1 >= 0 && idx + 1 < n) ? t[idx + 1] : 0.f,
              (idx + 2 >= 0 && idx + 2 < n) ? t[idx + 2] : 0.f);
}

DEV f3 image_rgb(const DevScene& S, const DevTexture& tx, float u, float v) {   // imageTexture.h:60-73,111-133
    const DevImage im = S.images[GIDX(S, tx.image, S.num_images, 1)];
    if (tx.nearest) {
        int i = (int)(u * im.width);
        int j = (int)(v * im.height);
        i = (im.width - 1 < i) ? im.width - 1 : i;
        j = (im.height - 1 < j) ? im.height - 1 : j;
        return texel(S, im, i, j);
    }
    float fi = u * im.width, fj = v * im.height;
    float hiw = (float)(im.width - 1), hih = (float)(im.height - 1);
    fi = (hiw < fi) ? hiw : fi; fi = (fi < 0.0f) ? 0.0f : fi;          // std::max(lower, std::min(n, upper))
    fj = (hih < fj) ? hih : fj; fj = (fj < 0.0f) ? 0.0f : fj;
    float p = floorf(fi), q = floorf(fj);
    float dx = fi - p, dy = fj - q;
    float w1 = (1 - dx) * (1 - dy), w2 = dx * (1 - dy), w3 = (1 - dx) * dy, w4 = dx * dy;
    int ip = (int)p, iq = (int)q;
    return add(add(add(muls(texel(S, im, ip, iq), w1), muls(texel(S, im, ip + 1, iq), w2)),
                   muls(texel(S, im, ip, iq + 1), w3)), muls(texel(S, im, ip + 1, iq + 1), w4));
}


DEV double perlin_f(float x) {                                          // perlinTexture.h:153-160
    x = fabsf(x);
    if (x > 1) return 0;
    float xSqr = x * x;
    float xCube = xSqr * x;
    return (-6 * xCube * xSqr) + 15 * xCube * x - 10 * xCube + 1;
}
DEV float gdot(const float* grad, int g, float x, float y, float z) {
    return grad[3 * g] * x + grad[3 * g + 1] * y + grad[3 * g + 2] * z;
}
DEV float perlin(const DevScene& S, const DevTexture& tx, float x, float y, float z) {   // perlinTexture.h:57-123
    x *= tx.noise_scale; y *= tx.noise_scale; z *= tx.noise_scale;
    int X = (int)floorf(x), Y = (int)floorf(y), Z = (int)floorf(z);
    float dx = x - X, dy = y - Y, dz = z - Z;
    X = X & 255; Y = Y & 255; Z = Z & 255;
    const int* p = S.perm;
    const float* gr = S.grad;
    int ind0 = p[X + p[Y + p[Z]]] % 12;
    int ind1 = p[X + p[Y + p[Z + 1]]] % 12;
    int ind2 = p[X + p[Y + 1 + p[Z]]] % 12;
    int ind3 = p[X + p[Y + 1 + p[Z + 1]]] % 12;
    int ind4 = p[X + 1 + p[Y + p[Z]]] % 12;
    int ind5 = p[X + 1 + p[Y + p[Z + 1]]] % 12;
    int ind6 = p[X + 1 + p[Y + 1 + p[Z]]] % 12;
    int ind7 = p[X + 1 + p[Y + 1 + p[Z + 1]]] % 12;
    double c0 = gdot(gr, ind0, dx, dy, dz), c1 = gdot(gr, ind4, dx - 1, dy, dz), c2 = gdot(gr, ind2, dx, dy - 1, dz),
           c3 = gdot(gr, ind6, dx - 1, dy - 1, dz), c4 = gdot(gr, ind1, dx, dy, dz - 1), c5 = gdot(gr, ind5, dx - 1, dy, dz - 1),
           c6 = gdot(gr, ind3, dx, dy - 1, dz - 1), c7 = gdot(gr, ind7, dx - 1, dy - 1, dz - 1);
    double fdx = perlin_f(dx), fdy = perlin_f(dy), fdz = perlin_f(dz);
    double fdx1 = perlin_f(dx - 1), fdy1 = perlin_f(dy - 1), fdz1 = perlin_f(dz - 1);
    double w0 = fdx * fdy * fdz, w1 = fdx1 * fdy * fdz, w2 = fdx * fdy1 * fdz, w3 = fdx1 * fdy1 * fdz;
    double w4 = fdx * fdy * fdz1, w5 = fdx1 * fdy * fdz1, w6 = fdx * fdy1 * fdz1, w7 = fdx1 * fdy1 * fdz1;
    double total = w0 * c0 + w1 * c1 + w2 * c2 + w3 * c3 + w4 * c4 + w5 * c5 + w6 * c6 + w7 * c7;
    if (!tx.noise_abs) return (float)((total + 1) / 2.0f);
    return (float)fabs(total);
}

DEV f3 tex_rgb(const DevScene& S, const DevTexture& tx, float u, float v) {
    if (tx.kind == 1) return mk(180.f, 30.f, 180.f);                    // PerlinTexture::GetRGBSample
    return image_rgb(S, tx, u, v);
}

// ---------------------------------------------------------------------------
// Normal / bump mapping (mesh.cpp:263-358, sphere.cpp:116-193)
// ---------------------------------------------------------------------------
// GetTangentAndBitangentForTriangle (mesh.cpp:390-422)
DEV void tri_tangents(f3 vert0, f3 vert1, f3 vert2, float2 v0_uv, float2 v1_uv, float2 v2_uv, f3& tan, f3& bitan) {
    f3 e1 = makeUnit(sub(vert1, vert0));
    f3 e2 = makeUnit(sub(vert2, vert1));
    float v0u = tiledUV(v0_uv.x), v0v = tiledUV(v0_uv.y);
    float v1u = tiledUV(v1_uv.x), v1v = tiledUV(v1_uv.y);
    float v2u = tiledUV(v2_uv.x), v2v = tiledUV(v2_uv.y);
    float u1 = v1u - v0u, v1 = v1v - v0v;
    float u2 = v2u - v1u, v2 = v2v - v1v;
    float det = 1.0f / (u1 * v2 - v1 * u2);
    tan = mk(det * (v2 * e1.x - v1 * e2.x), det * (v2 * e1.y - v1 * e2.y), det * (v2 * e1.z - v1 * e2.z));
    const float nd = -det;
    bitan = mk(nd * u2 * e1.x + det * u1 * e2.x, nd * u2 * e1.y + det * u1 * e2.y, nd * u2 * e1.z + det * u1 * e2.z);
    tan = makeUnit(tan);
    bitan = makeUnit(bitan);
}
// GetTransformedNormal (helperMath.cpp:86-109): 3x3 double Matrix product, row by row
DEV f3 tbn_normal(f3 tan, f3 bitan, f3 normal, f3 sn) {
    double r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
    r0 += (double)tan.x * (double)sn.x; r0 += (double)bitan.x * (double)sn.y; r0 += (double)normal.x * (double)sn.z;
    r1 += (double)tan.y * (double)sn.x; r1 += (double)bitan.y * (double)sn.y; r1 += (double)normal.y * (double)sn.z;
    r2 += (double)tan.z * (double)sn.x; r2 += (double)bitan.z * (double)sn.y; r2 += (double)normal.z * (double)sn.z;
    return makeUnit(mk((float)r0, (float)r1, (float)r2));
}
// perlin bump: N minus the surface part of the height gradient (mesh.cpp:290-309, sphere.cpp:123-138)
DEV f3 perlin_bump(const DevScene& S, const DevTexture& bm, f3 N, f3 p, float bf, bool scaled) {
    const float eps = 0.001;
    float h0 = perlin(S, bm, p.x, p.y, p.z);
    float hxyz = scaled ? h0 * bf : h0;
    float gx = perlin(S, bm, p.x + eps, p.y, p.z), gy = perlin(S, bm, p.x, p.y + eps, p.z),
          gz = perlin(S, bm, p.x, p.y, p.z + eps);
    if (scaled) { gx = gx * bf; gy = gy * bf; gz = gz * bf; }
    f3 gradient = mk((gx - hxyz) / eps, (gy - hxyz) / eps, (gz - hxyz) / eps);
    f3 gParallel = muls(N, dot(gradient, N));
    f3 surfaceGradient = sub(gradient, gParallel);
    return makeUnit(sub(N, surfaceGradient));
}
// Normal of a mapped mesh face in the base mesh's object space, before its transform.
DEV f3 mesh_mapped_normal(const DevScene& S, const DevObject& ob, int face, f3 lp, float u, float v) {
    const f3 N = ld3(&S.face_n[face].x);
    const float4 a = S.tris[3 * face], b = S.face_v12[2 * face], c = S.face_v12[2 * face + 1];
    f3 tan, bitan;
    tri_tangents(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), S.face_uv[3 * face],
                 S.face_uv[3 * face + 1], S.face_uv[3 * face + 2], tan, bitan);
    if (ob.tex_normal >= 0) {                                            // mesh.cpp:263-272
        f3 sn = tex_rgb(S, S.textures[ob.tex_normal], u, v);
        sn = sub(divs(sn, 127.5f), mk(1, 1, 1));
        sn = makeUnit(sn);
        return tbn_normal(tan, bitan, N, sn);
    }
    const DevTexture& bm = S.textures[ob.tex_bump];
    if (bm.kind == 1) return perlin_bump(S, bm, N, lp, bm.bump_factor, true);
    // image bump map, forward differences (mesh.cpp:310-352)
    const DevImage im = S.images[bm.image];
    const float width = (float)im.width, height = (float)im.height;
    int i = (int)(u * (width - 1));
    int j = (int)(v * (height - 1));
    int nextI = i + 1, nextJ = j + 1;
    if ((float)i == width - 1) nextI = i;
    if ((float)j == height - 1) nextJ = j;
    f3 t0 = texel(S, im, i, j), tu = texel(S, im, nextI, j), tv = texel(S, im, i, nextJ);
    float h_uv = (t0.x + t0.y + t0.z) / 3.0f;                            // MakeGreyscale (mesh.cpp:195-197)
    float hDeltaU = (tu.x + tu.y + tu.z) / 3.0f;
    float hDeltaV = (tv.x + tv.y + tv.z) / 3.0f;
    const float bumpFactor = bm.bump_factor;
    f3 q_u = add(tan, muls(N, (hDeltaU - h_uv) * bumpFactor));
    f3 q_v = add(bitan, muls(N, (hDeltaV - h_uv) * bumpFactor));
    f3 nn = cross(q_v, q_u);
    f3 n = makeUnit(nn);
    if (nn.x * N.x <= 0 && nn.y * N.y <= 0 && nn.z * N.z <= 0) n = muls(n, -1.0f);
    else if (fabsf(nn.y - N.y) > 0.9f || fabsf(nn.x - N.x) > 0.9f || fabsf(nn.z - N.z) > 0.9f) n = muls(n, -1.0f);
    return n;
}
// Bumped sphere normal in local space (sphere.cpp:116-170, tangents sphere.cpp:181-193).
DEV f3 sphere_bumped_normal(const DevScene& S, const DevObject& ob, f3 p, float phi, float theta, float u, float v) {
    const float radius = ob.center[3];
    f3 tan = mk((float)(2 * RT_PI * (double)p.z), 0.0f, (float)(-2 * RT_PI * (double)p.x));
    f3 bitan = mk((float)(RT_PI * (double)p.y * (double)cosf(phi)),
                  (float)((double)(-radius) * RT_PI * (double)sinf(theta)),
                  (float)(RT_PI * (double)p.y * (double)sinf(phi)));
    tan = makeUnit(tan);
    bitan = makeUnit(bitan);
    const f3 N = makeUnit(cross(bitan, tan));
    const DevTexture& bm = S.textures[ob.tex_bump];
    if (bm.kind == 1) return perlin_bump(S, bm, N, p, 1.0f, false);
    const DevImage im = S.images[bm.image];
    int i = (int)(u * (float)im.width);
    int j = (int)(v * (float)im.height);
    const float normalizer = bm.normalizer, bumpFactor = bm.bump_factor;
    f3 c1 = divs(texel(S, im, i + 1, j), normalizer), c0 = divs(texel(S, im, i, j), normalizer),
       c2 = divs(texel(S, im, i, j + 1), normalizer);
    float h1 = (c1.x + c1.y + c1.z) * bumpFactor;                        // MakeGreyscale (sphere.cpp:9-11)
    float h_uv = (c0.x + c0.y + c0.z) * bumpFactor;
    float h2 = (c2.x + c2.y + c2.z) * bumpFactor;
    f3 q_u = add(tan, muls(N, h1 - h_uv));
    f3 q_v = add(bitan, muls(N, h2 - h_uv));
    return makeUnit(cross(q_v, q_u));
}

// MAPS = false: the scene has no normal / bump maps (OBJF_MAPPED never set; k_shade variants)
// FEAT: the scene's feature bits where the caller's variant knows them (k_shade's fused layouts;
// FEAT_ALL: any scene): without FEAT_SPHERE no hit is a sphere's and that branch is compiled out.
// MOTION = false: the caller's pipeline never renders a scene with motion blur (k_shade), so
// OBJF_MOTION_BLUR is not tested and mbTime not read.
template <bool STATS, bool MAPS = true, int FEAT = FEAT_ALL, bool MOTION = true>
DEV Surf surface(const DevScene& S, const Ray& r, float mbTime, const Hit& h, Cnt<STATS>& c) {
    const DevObject& ob = S.objects[GIDX(S, h.obj, S.num_objects, 0)];
    Surf s;
    s.p = add(r.o, muls(r.d, h.t));                                    // raytracer.cpp:69
    s.u = s.v = 0.f;
    Ray hr;
    hr.o = h.o;
    hr.d = r.d;
    Ray lr = local_ray<MOTION>(ob, hr, mbTime);
    if ((FEAT & FEAT_SPHERE) && h.face < 0) {                          // sphere.cpp:71-175
        const f3 center = mk(ob.center[0], ob.center[1], ob.center[2]);
        f3 lp = add(lr.o, muls(lr.d, h.t));
        f3 p = sub(lp, center);
        float phi = atan2f(p.z, p.x);
        float theta = acosf(p.y / ob.center[3]);
        s.u = (float)((-phi + RT_PI) / (2.0f * RT_PI));
        s.v = (float)(theta / RT_PI);
        f3 n = (MAPS && (ob.flags & OBJF_MAPPED)) ? sphere_bumped_normal(S, ob, p, phi, theta, s.u, s.v)
                                        : makeUnit(sub(lp, center));
        s.n = makeUnit(xform(ob.invT, n, 0.0f));
        return s;
    }
    f3 n = ld3(&S.face_n[GIDX(S, h.face, S.num_faces, 3)].x);
    if (ob.flags & OBJF_NORMAL_TWICE) n = makeUnit(xform(ob.baseInvT, n, 0.0f));   // mesh.cpp:363
    if (ob.flags & OBJF_HAS_UV) {                                                     // mesh.cpp:245-262
        float bg[2], t;
        tri_test(S, h.face, lr, INFINITY, t, bg);
        const float2 a = S.face_uv[3 * h.face], b = S.face_uv[3 * h.face + 1], cc = S.face_uv[3 * h.face + 2];
        float u = a.x + bg[0] * (b.x - a.x) + bg[1] * (cc.x - a.x);
        float v = a.y + bg[0] * (b.y - a.y) + bg[1] * (cc.y - a.y);
        s.u = tiledUV(u);
        s.v = tiledUV(v);
        if (MAPS && (ob.flags & OBJF_MAPPED)) {
            // IntersectFace's local hit point (mesh.cpp:242), then the base mesh's transform
            const f3 lp = add(lr.o, muls(lr.d, h.t));
            n = makeUnit(xform(ob.baseInvT, mesh_mapped_normal(S, ob, h.face, lp, s.u, s.v), 0.0f));
        }
    }
    s.n = makeUnit(xform(ob.invT, n, 0.0f));                                          // mesh.cpp:179 / instancedMesh.cpp:57
    return s;
}

// SphericalEnvironmentLight::GetSample (sphericalEnvironmentLight.h:22-34)
DEV f3 env_sample(const DevScene& S, int e, f3 dir) {
    const DevImage im = S.images[S.env_images[e]];
    float u = (float)((1 + (atan2f(dir.x, -dir.z) / RT_PI)) / 2.0f);
    float v = (float)(acosf(dir.y) / RT_PI);
    int i = (int)(im.width * u);
    int j = (int)(im.height * v);
    return muls(muls(texel(S, im, i, j), (float)2), (float)RT_PI);
}

// GetDirection (sphericalEnvironmentLight.h:36-61): rejection sampling, returns the
// un-normalised candidate.  The reference spins forever on a NaN normal; bounded here.
// The draws are rnd(key, RP_ENV, e * 16384 + 3k + c); the inner hash of (purpose, index) does
// not depend on the key, so it comes from a table (S.env_mix, kEnvDraws per light, built by
// rtg_scene_create with the same mix64): one 64-bit hash per draw instead of two, the same bits.
// A wave runs until its last lane accepts (~17 candidates for 64 lanes at acceptance pi/12),
// and the table index is the loop counter, so the loads are scalar.
static_assert(RP_ENV == kRpEnv, "env_mix table purpose");
DEV float rnd_mixed(uint64_t key, uint64_t inner) {
    const uint64_t h = mix64(key ^ inner);
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}
DEV f3 env_direction(const DevScene& S, f3 surfaceNormal, uint64_t key, int e) {
    f3 n = makeUnit(surfaceNormal);
    f3 cand = mk(0, 0, 0);
    const unsigned long long* T = S.env_mix + (size_t)e * kEnvDraws;
    for (uint32_t k = 0; k < 4096; ++k) {
        cand.x = 2.0f * rnd_mixed(key, T[3 * k]) - 1.0f;
        cand.y = 2.0f * rnd_mixed(key, T[3 * k + 1]) - 1.0f;
        cand.z = 2.0f * rnd_mixed(key, T[3 * k + 2]) - 1.0f;
        float length = len(cand);
        if (length <= 1.0f && dot(n, cand) > 0.0f) break;
    }
    return cand;
}

// The same search for a whole wave (every lane calls it; `want`: the lane needs a direction).
// A lane's loop runs until its first accepted candidate (3.8 on average at acceptance pi/12),
// but the wave's until its last lane's (~17 for 64 lanes); here the lanes still searching get
// the others' help: with na of them, each gets g = 64 / na lanes testing its candidates
// k .. k+g-1 at once, and takes the smallest accepted index -- the candidate its own loop
// returns (the first accepted of 0..4095, else the 4095th), computed by the same operations.
DEV f3 env_candidate(const unsigned long long* T, uint64_t key, int k) {
    return mk(2.0f * rnd_mixed(key, T[3 * k]) - 1.0f, 2.0f * rnd_mixed(key, T[3 * k + 1]) - 1.0f,
              2.0f * rnd_mixed(key, T[3 * k + 2]) - 1.0f);
}
// position of the r-th (from 0) set bit of m (r < popcount(m))
DEV int nth_set_bit(uint64_t m, int r) {
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const uint64_t lo = m & ((1ull << w) - 1ull);
        const int c = __popcll(lo);
        const bool up = r >= c;
        r = up ? r - c : r;
        m = up ? m >> w : lo;
        pos = up ? pos + w : pos;
    }
    return pos;
}
DEV f3 env_direction_wave(const DevScene& S, f3 surfaceNormal, uint64_t key, int e, bool want) {
    const f3 n = makeUnit(surfaceNormal);
    const unsigned long long* T = S.env_mix + (size_t)e * kEnvDraws;
    const int lane = threadIdx.x & 63;
    int k = 0;
    bool done = !want;
    f3 cand = mk(0, 0, 0);
    for (;;) {
        const uint64_t act = __ballot(!done);
        if (!act) break;
        const int na = __popcll(act);
        const int g = 64 / na;
        if (g == 1) {                  // more than 32 searching: each tests its own next candidate
            if (!done) {
                const f3 c = env_candidate(T, key, k);
                if ((len(c) <= 1.0f && dot(n, c) > 0.0f) || ++k >= 4096) {
                    cand = c;
                    done = true;
                }
            }
            continue;
        }
        const int r = lane / g;                            // the searcher this lane helps
        const bool helper = r < na;
        const int owner = helper ? nth_set_bit(act, r) : lane;
        const uint64_t okey = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(key >> 32), owner) << 32) |
                              (uint32_t)__shfl((int)(uint32_t)key, owner);
        const f3 on = mk(__shfl(n.x, owner), __shfl(n.y, owner), __shfl(n.z, owner));
        const int kk = __shfl(k, owner) + (lane - r * g);
        f3 c = mk(0, 0, 0);
        bool acc = false;
        if (helper && kk < 4096) {
            c = env_candidate(T, okey, kk);
            acc = len(c) <= 1.0f && dot(on, c) > 0.0f;
        }
        const uint64_t am = __ballot(acc);
        const int rank = __popcll(act & ((1ull << lane) - 1ull));
        const uint64_t mine = done ? 0ull : (am >> (rank * g)) & (g >= 64 ? ~0ull : (1ull << g) - 1ull);
        const int src = mine ? rank * g + __ffsll((long long)mine) - 1 : lane;
        const f3 w = mk(__shfl(c.x, src), __shfl(c.y, src), __shfl(c.z, src));
        if (!done) {
            if (mine) {
                cand = w;
                done = true;
            } else if ((k += g) >= 4096) {
                cand = env_candidate(T, key, 4095);
                done = true;
            }
        }
    }
    return cand;
}

// ---------------------------------------------------------------------------
// BRDFs (brdf*.cpp) and Shade (raytracer.cpp:192-206, 478-554)
// ---------------------------------------------------------------------------
DEV f3 brdf_apply(const DevBrdf& B, float refrIdx, f3 kd, f3 ks, f3 w_i, f3 w_o, f3 normal) {
    const float th = (float)angleBetween(w_i, normal);
    const double ex = (double)B.exponent;
    switch (B.type) {
        case 0: {                                                       // brdfPhong.cpp:11-20
            if (th >= 90.0f || th < 0) return mk(0, 0, 0);
            f3 r = makeUnit(sub(muls(muls(normal, 2.0f), dot(normal, w_i)), w_i));
            double angleR = angleBetween(r, w_o);
            return add(kd, muls(ks, (float)(pow(cosDeg(angleR), ex) / cosDeg(th))));
        }
        case 1: {                                                       // brdfBlinnPhong.cpp:11-20
            if (th >= 90.0f) return mk(0, 0, 0);
            f3 half = divs(add(w_i, w_o), len(add(w_i, w_o)));
            double a = angleBetween(half, normal);
            return add(kd, muls(ks, (float)(pow(cosDeg(a), ex) / cosDeg(th))));
        }
        case 2: {                                                       // brdfModifiedPhong.cpp:14-33
            if (th >= 90.0f || th < 0) return mk(0, 0, 0);
            f3 r = makeUnit(sub(muls(muls(normal, 2.0f), dot(normal, w_i)), w_i));
            double angleR = angleBetween(r, w_o);
            if (B.energy_conserving) {
                f3 kdTerm = muls(kd, (float)(1.0f / RT_PI));
                double ksCons = (B.exponent + 2) / (2 * RT_PI);
                double cosTerm = pow(cosDeg(angleR), ex);
                return add(kdTerm, muls(ks, (float)(ksCons * cosTerm)));
            }
            return add(kd, muls(ks, (float)pow(cosDeg(angleR), ex)));
        }
        case 3: {                                                       // brdfModifiedBlinnPhong.cpp:11-29
            if (th >= 90.0f) return mk(0, 0, 0);
            f3 half = divs(add(w_i, w_o), len(add(w_i, w_o)));
            double a = angleBetween(half, normal);
            if (B.energy_conserving) {
                f3 kdTerm = muls(kd, (float)(1.0f / RT_PI));
                double ksCons = (B.exponent + 8) / (8 * RT_PI);
                double cosTerm = pow(cosDeg(a), ex);
                return add(kdTerm, muls(ks, (float)(ksCons * cosTerm)));
            }
            return add(kd, muls(ks, (float)pow(cosDeg(a), ex)));
        }
        default: {                                                      // brdfTorranceSparrow.cpp:15-59
            if (th >= 90.0f) return mk(0, 0, 0);
            f3 half = divs(add(w_i, w_o), len(add(w_i, w_o)));
            double cosAlpha = dot(half, normal);
            double d = (ex + 2) * pow(cosAlpha, ex) / (2 * RT_PI);
            double cosbeta = dot(half, w_o), n = refrIdx;
            double r0 = pow(n - 1, 2.0) / pow(n + 1, 2.0);
            double f = r0 + (1.0 - r0) * pow((1.0 - cosbeta), 5.0);
            double ndoth = dot(normal, half), ndotwo = dot(normal, w_o), ndotwi = dot(normal, w_i), wodoth = dot(w_o, half);
            double ga = 2.0f * ndoth * ndotwo / wodoth, gb = 2.0 * ndoth * ndotwi / wodoth;
            double gm = (gb < ga) ? gb : ga;
            double g = (gm < 1.0) ? gm : 1.0;
            double kdCoeff = (1.0f / RT_PI);
            if (B.kd_fresnel) kdCoeff *= (1 - f);
            f3 kdTerm = muls(kd, (float)kdCoeff);
            double costheta = dot(normal, w_i), cosphi = dot(normal, w_o);
            f3 ksTerm = muls(ks, (float)((d * f * g) / (4 * costheta * cosphi)));
            return add(kdTerm, ksTerm);
        }
    }
}

struct ShadeCtx {
    const DevObject* ob;
    const DevMaterial* mat;
    Surf s;
};

template <bool TEX = true>
DEV f3 kd_coeff(const DevScene& S, const ShadeCtx& c) {                // raytracer.cpp:478-508
    f3 refl = ld3(c.mat->diffuse);
    if (TEX && c.ob->tex_diffuse >= 0) {
        const DevTexture tx = S.textures[GIDX(S, c.ob->tex_diffuse, S.num_textures, 2)];
        f3 t;
        if (tx.kind == 1) { float p = perlin(S, tx, c.s.p.x, c.s.p.y, c.s.p.z); t = mk(p, p, p); }
        else t = divs(image_rgb(S, tx, c.s.u, c.s.v), 255.0f);
        refl = tx.blend ? divs(add(t, ld3(c.mat->diffuse)), 2.0f) : t;
    }
    return refl;
}
template <bool TEX = true>
DEV f3 ks_coeff(const DevScene& S, const ShadeCtx& c) {                // raytracer.cpp:509-539 (reads diffuseTex)
    f3 refl = ld3(c.mat->specular);
    if (TEX && c.ob->tex_specular >= 0 && c.ob->tex_diffuse >= 0) {
        const DevTexture tx = S.textures[GIDX(S, c.ob->tex_diffuse, S.num_textures, 2)];
        f3 t;
        if (tx.kind == 1) { float p = perlin(S, tx, c.s.p.x, c.s.p.y, c.s.p.z); t = mk(p, p, p); }
        else t = divs(image_rgb(S, tx, c.s.u, c.s.v), 255.0f);
        refl = tx.blend ? divs(add(t, ld3(c.mat->diffuse)), 2.0f) : t;
    }
    return refl;
}

// Shade (raytracer.cpp:192-206).  TP: also ray.throughput *= brdf (:202), which Russian
// roulette reads (path tracing only).
template <bool TP = false, int SK = SK_ALL>
DEV f3 shade(const DevScene& S, const ShadeCtx& c, f3 w_i, f3 w_o, f3 Li, f3* tp = nullptr) {
    constexpr bool TEX = (SK & SK_TEX) != 0;
    if ((SK & SK_BRDF) && c.mat->brdf >= 0) {
        float costheta_i = fmax0(dot(w_i, c.s.n));
        f3 kd = kd_coeff<TEX>(S, c), ks = ks_coeff<TEX>(S, c);
        f3 res = brdf_apply(S.brdfs[c.mat->brdf], c.mat->refractive_index, kd, ks, w_i, w_o, c.s.n);
        if (TP) *tp = mulv(*tp, res);
        return muls(mulv(res, Li), costheta_i);
    }
    f3 kd = kd_coeff<TEX>(S, c);                                        // GetDiffuse
    float costheta = fmax0(dot(w_i, c.s.n));
    f3 diff = muls(mulv(kd, Li), costheta);
    f3 ks = ks_coeff<TEX>(S, c);                                        // GetSpecular
    f3 half = divs(add(w_i, w_o), len(add(w_i, w_o)));
    float cosAlpha = fmax0(dot(c.s.n, half));
    f3 spec = muls(mulv(ks, Li), powf(cosAlpha, c.mat->phong_exponent));
    return add(diff, spec);
}

// IsInShadow (raytracer.cpp:567-584); IsInShadowDirectional (:555-566)
template <bool STATS>
DEV bool in_shadow(const DevScene& S, f3 p, f3 n, f3 lightPos, float mbTime, Cnt<STATS>& c) {
    f3 dir = sub(lightPos, p);
    float lightT = len(dir);
    Ray sr;
    sr.d = divs(dir, lightT);
    sr.o = add(p, muls(n, S.eps));
    Hit h;
    c.shd();
    return trace<true, STATS>(S, sr, mbTime, lightT + 0.01f, lightT, h, c);
}
template <bool STATS>
DEV bool in_shadow_dir(const DevScene& S, f3 p, f3 n, f3 lightDir, float mbTime, Cnt<STATS>& c) {
    Ray sr;
    sr.d = neg(lightDir);
    sr.o = add(p, muls(n, S.eps));
    Hit h;
    c.shd();
    return trace<true, STATS>(S, sr, mbTime, INFINITY, INFINITY, h, c);
}

// One light of SampleDirectLighting (raytracer.cpp:701-805), slots in the reference's
// type order point, area, env, dir, spot: the incident direction, the irradiance and,
// where the reference casts one, the shadow ray (IsInShadow :567-584 /
// IsInShadowDirectional :555-566).
// MeshLight::getSample (meshLight.h:27-47) and the irradiance of SampleDirectLighting's
// mesh-light branch (raytracer.cpp:780-803: radiance * weight * 2 * M_PI, no distance
// term).  The reference draws the face from uniform_int_distribution(0, faceCount) --
// inclusive, so 1 draw in faceCount+1 indexes past the face vector (undefined); here the
// face is uniform over the faceCount faces.
DEV void mesh_light_sample(const DevScene& S, int l, uint64_t key, f3& pos, f3& E) {
    const DevMeshLight& L = S.mesh_lights[l];
    int k = (int)(rndd(key, RP_MESHLIGHT, 3 * l) * L.face_count);
    k = k < L.face_count ? k : L.face_count - 1;
    const DevLightFace& F = S.light_faces[L.face_begin + k];
    const double selectionWeight = F.area / L.surface_area;
    const double rand1 = rndd(key, RP_MESHLIGHT, 3 * l + 1);
    const double rand2 = rndd(key, RP_MESHLIGHT, 3 * l + 2);
    const f3 a = ld3(F.v0), b = ld3(F.v1), c = ld3(F.v2);
    f3 q = add(muls(b, (float)(1 - rand2)), muls(c, (float)rand2));
    pos = add(muls(a, (float)(1 - sqrt(rand1))), muls(q, (float)sqrt(rand1)));
    pos = xform(L.xf, pos, 1.0f);                                      // ApplyTransformToPoint(transform)
    E = muls(muls(muls(ld3(L.radiance), (float)selectionWeight), 2.0f), (float)RT_PI);
}

struct LightSample {
    f3 w_i, E;
    bool shadow;
    bool skip;         // mesh light hit by this node's GI ray (raytracer.cpp:784): no term
    Ray sr;
    float minT, limit;
};
// SK without SK_XLIGHT: the scene has no env / spot / mesh lights (their code is left out).
template <int SK = SK_ALL>
DEV LightSample light_sample(const DevScene& S, int slot, f3 p, f3 n, uint64_t key, int skipId = -1) {
    LightSample ls;
    ls.shadow = true;
    ls.skip = false;
    ls.sr.o = add(p, muls(n, S.eps));
    f3 lpos = mk(0, 0, 0);
    bool positional = true;
    int i = slot;
    constexpr bool XL = (SK & SK_XLIGHT) != 0;
    if (i < S.num_point) {
        const f3 lp = ld3(S.point_lights[i].pos);
        lpos = lp;
        ls.w_i = makeUnit(sub(lp, p));
        float dist = len(sub(lp, p));
        ls.E = divs(ld3(S.point_lights[i].intensity), dist * dist);
    } else if ((i -= S.num_point) < S.num_area) {
        const DevAreaLight& L = S.area_lights[i];
        float offU = rnd(key, RP_AREA, 2 * i) - 0.5f;                     // areaLight.h:34-41
        float offV = rnd(key, RP_AREA, 2 * i + 1) - 0.5f;
        f3 sp = add(add(ld3(L.pos), muls(ld3(L.u), L.extent * offU)), muls(ld3(L.v), L.extent * offV));
        lpos = sp;
        f3 w_i = sub(sp, p);
        float dist = len(w_i);
        float dSqr = dist * dist;
        w_i = divs(w_i, dist);
        float lc = dot(ld3(L.normal), neg(w_i));
        if (lc < 0) lc = dot(ld3(L.normal), w_i);
        ls.w_i = w_i;
        ls.E = muls(ld3(L.radiance), L.area * lc / dSqr);
    } else if (XL && (i -= S.num_area) < S.num_env) {                     // no shadow ray (:741-755)
        f3 sd = env_direction(S, n, key, i);
        ls.E = env_sample(S, i, sd);
        ls.w_i = n;
        ls.shadow = false;
    } else if (!XL || (i -= S.num_env) < S.num_dir) {
        if (!XL) i -= S.num_area;
        const f3 ldir = ld3(S.dir_lights[i].dir);
        ls.w_i = neg(ldir);
        ls.E = ld3(S.dir_lights[i].radiance);
        ls.sr.d = neg(ldir);
        ls.minT = INFINITY;
        ls.limit = INFINITY;
        positional = false;
    } else if ((i -= S.num_dir) >= S.num_spot) {
        i -= S.num_spot;                                                // mesh lights (:780-803)
        ls.skip = S.mesh_lights[i].id == skipId;
        f3 sp, E;
        mesh_light_sample(S, i, key, sp, E);
        lpos = sp;
        f3 w_i = sub(sp, p);
        float dist = len(w_i);
        ls.w_i = divs(w_i, dist);
        ls.E = E;
    } else {
        const DevSpotLight& L = S.spot_lights[i];
        const f3 lp = ld3(L.pos);
        lpos = lp;
        ls.w_i = makeUnit(sub(lp, p));
        // SpotLight::GetIrradiance (spotLight.h:33-57)
        float distToPoint = len(sub(p, lp));
        f3 toPoint = divs(sub(p, lp), distToPoint);
        double alpha = angleBetween(ld3(L.dir), toPoint);
        f3 E;
        if (alpha <= 0 || alpha > (L.coverage_deg / 2.0f)) {
            E = mk(0, 0, 0);
        } else {
            float distSqr = distToPoint * distToPoint;
            E = divs(ld3(L.intensity), distSqr);
            if (alpha > (L.falloff_deg / 2.0f)) {
                double cosAlpha = cos(alpha * (RT_PI / 180.0f));
                double sv = pow((cosAlpha - L.cos_half_coverage) / (L.cos_half_falloff - L.cos_half_coverage), (double)4.0f);
                E = muls(E, (float)sv);
            }
        }
        ls.E = E;
    }
    if (ls.shadow && positional) {
        f3 dir = sub(lpos, p);
        float lightT = len(dir);
        ls.sr.d = divs(dir, lightT);
        ls.minT = lightT + 0.01f;
        ls.limit = lightT;
    }
    return ls;
}

// SampleDirectLighting (raytracer.cpp:701-805): the unshadowed lights' Shade terms summed in
// slot order.  One trace and one Shade call site for all light types (the BRDF code and the
// traversal are inlined once).
// TP / skipId: path tracing -- throughput update per Shade, and the mesh light the node's
// GI ray hit is not sampled (raytracer.cpp:92,784).
// SK / FEAT: shading and traversal features the scene may use (the path tracer's variants).
template <bool STATS, bool TP = false, int SK = SK_ALL, int FEAT = FEAT_ALL>
DEV f3 direct(const DevScene& S, const ShadeCtx& c, f3 w_o, float mbTime, uint64_t key, Cnt<STATS>& cn,
              int skipId = -1, f3* tp = nullptr) {
    f3 color = mk(0, 0, 0);
    const f3 p = c.s.p, n = c.s.n;
    const int nslots = S.num_point + S.num_area + S.num_env + S.num_dir + S.num_spot + S.num_mesh;
    for (int l = 0; l < nslots; ++l) {
        LightSample ls = light_sample<SK>(S, l, p, n, key, skipId);
        if (ls.skip) continue;
        if (ls.shadow) {
            Hit h;
            cn.shd();
            if (trace<true, STATS, FEAT>(S, ls.sr, mbTime, ls.minT, ls.limit, h, cn)) continue;
        }
        color = add(color, shade<TP, SK>(S, c, ls.w_i, w_o, ls.E, tp));
    }
    return color;
}

// Raytracer::Reflect (raytracer.cpp:424-440)
DEV f3 reflect(f3 normal, f3 w_o, float roughness, uint64_t key, uint32_t purpose) {
    f3 r = makeUnit(sub(muls(muls(normal, 2.0f), dot(normal, w_o)), w_o));
    if (roughness > 0.001) {
        f3 u, v;
        onb(r, u, v);
        float psi1 = rnd(key, purpose, 0) - 0.5f;
        float psi2 = rnd(key, purpose, 1) - 0.5f;
        return makeUnit(add(r, muls(add(muls(u, psi1), muls(v, psi2)), roughness)));
    }
    return r;
}

DEV f3 beer(float x, const float* c, f3 L0) {                          // raytracer.cpp:416-423
    return mk(L0.x * expf(-c[0] * x), L0.y * expf(-c[1] * x), L0.z * expf(-c[2] * x));
}

}  // namespace rtg
