// Surface queries (rtgpu.h rtg_surface_rays*): what a render's PerformShading knows about the
// point a caller's ray hits, one ray per lane.
//
//   k_surface   IntersectObjects (trace<>, per lane or as wave packets: k_query's closest-hit
//               branch), then the hit's surface() with normal / bump maps applied, its geometric
//               normal, and GetDiffuse's coefficient (kd_coeff: diffuse textures applied)
//
// One fused kernel: surface() needs Hit::o, the origin at the moment the hit was accepted (a
// motion-blurred instance whose world box is missed leaves its offset on it), which a second pass
// over rtg_hit records cannot recover.  The device functions are the render's own, so the values
// are the ones k_shade / the fused kernel shade with.
#include "rtg_common.hpp"
#include "rtg_kernels.hpp"

namespace rtg {

static_assert(sizeof(rtg_surface) == 64 && sizeof(rtg_ray) == 32, "two 16-byte loads per ray, four 16-byte stores per result");

// Occupancy: the walk's own bound, as k_query has it with the normal.  TEX = false (scenes without
// textures or maps, shade_sk & SK_TEX == 0: surface<false, false> and kd_coeff<false> give the same
// values there) is its own instantiation because it sheds the scratch: 0 - 12 B per lane on plain
// scenes against 508 - 656 B for the mapped variant, whose bump / Perlin code needs 218 VGPRs
// unspilled.  The mapped variant still runs fastest at the walk's bound: on the textured fixture
// surface / trace-with-normals is 1.32 at eight waves, 1.42 at four (128 VGPRs, 300 B) and 1.97 at two
// (no scratch) -- the spills sit in the shading tail, run once per ray, and the walk wants the
// occupancy (profiles/r09_surface_resources.txt, r09_surface_waves_ab.txt).
constexpr int surface_waves(int feat, bool pk, bool tex) {
    const int w = RTG_TRACE_WAVES(feat);
    return (!tex && !pk && w > 7) ? 7 : w;
}

// Lanes past n take no part (the packet walk's ballots count live lanes only), as in k_query.
template <int FEAT, bool PK, bool TEX>
__global__ __launch_bounds__(256, surface_waves(FEAT, PK, TEX)) void k_surface(const DevScene S, const float4* __restrict__ rays,
                                                                          const int n, float4* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];
    Cnt<false> cn;
    Ray r;
    r.o = mk(a.x, a.y, a.z);
    r.d = mk(b.x, b.y, b.z);
    Hit h;
    trace<false, false, FEAT, PK>(S, r, b.w, a.w, INFINITY, h, cn);
    // a miss: t = tmax, object = face = material = -1, everything else +0
    float4 o0 = make_float4(h.t, __int_as_float(h.obj), __int_as_float(h.face), __int_as_float(-1));
    float4 o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1, o3 = o1;
    if (h.obj >= 0) {
        const DevObject& ob = S.objects[GIDX(S, h.obj, S.num_objects, 0)];
        ShadeCtx c;
        c.ob = &ob;
        c.mat = &S.materials[GIDX(S, ob.material, S.num_materials, 7)];
        c.s = surface<false, TEX>(S, r, b.w, h, cn);                    // PerformShading's normal and uv
        // the geometric normal: the same value where no map is in effect, k_query's otherwise
        f3 g = c.s.n;
        if constexpr (TEX)
            if (ob.flags & OBJF_MAPPED) g = surface<false, false>(S, r, b.w, h, cn).n;
        const f3 kd = kd_coeff<TEX>(S, c);                             // GetDiffuse
        o0.w = __int_as_float(ob.material);
        o1 = make_float4(c.s.n.x, c.s.n.y, c.s.n.z, c.s.u);
        o2 = make_float4(g.x, g.y, g.z, c.s.v);
        o3 = make_float4(kd.x, kd.y, kd.z, 0.f);
    }
    float4* __restrict__ o = out + 4 * (size_t)i;
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    o[3] = o3;
}

template <int FEAT, bool TEX>
static hipError_t launch_surface_f(const DevScene& S, const rtg_ray* rays, int n, uint32_t flags, rtg_surface* out,
                                   hipStream_t st) {
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    const float4* R = reinterpret_cast<const float4*>(rays);
    float4* O = reinterpret_cast<float4*>(out);
    // the packet walk under the hint, except on large-leaf scenes (launch_query_f)
    if constexpr (!(FEAT & FEAT_BIGLEAF)) {
        if (flags & RTG_QUERY_COHERENT) {
            hipLaunchKernelGGL((k_surface<FEAT, true, TEX>), grid, block, 0, st, S, R, n, O);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_surface<FEAT, false, TEX>), grid, block, 0, st, S, R, n, O);
    return hipGetLastError();
}

hipError_t launch_surface(const DevScene& S, int sk, int feat, const rtg_ray* rays, int n, uint32_t flags, rtg_surface* out,
                          hipStream_t stream) {
    return with_trav_feat(feat, [&](auto F) {
        constexpr int FEAT = decltype(F)::value;
        return (sk & SK_TEX) ? launch_surface_f<FEAT, true>(S, rays, n, flags, out, stream)
                             : launch_surface_f<FEAT, false>(S, rays, n, flags, out, stream);
    });
}

}  // namespace rtg
