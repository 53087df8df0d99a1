// Kernel variants: which instantiation of a kernel a scene, a camera and a render take.
// The only place the choice is made -- every launch site asks here.  Host only: the rules
// are pure functions of the feature bits (tests/kernel_variants_main.cpp prints them all),
// the with_*() dispatchers hand the chosen values to a generic lambda as
// std::integral_constant arguments, so `decltype(F)::value` is a template argument there.
// A dispatcher names exactly the instantiations that exist: adding a value to one adds a
// kernel to every translation unit that uses it.
#pragma once

#include <hip/hip_runtime.h>   // vector types only (rtg_device.hpp's records)

#include <cstdlib>
#include <type_traits>

#include "rtg_device.hpp"

namespace rtg {

template <int V>
using int_c = std::integral_constant<int, V>;

// fn(int_c<V>) for the V of the list that equals v (which is one of them; else the last)
template <int V, int... Vs, typename Fn>
auto with_value(int v, Fn&& fn) {
    if constexpr (sizeof...(Vs) == 0) {
        return fn(int_c<V>{});
    } else {
        if (v == V) return fn(int_c<V>{});
        return with_value<Vs...>(v, fn);
    }
}

// ---------------------------------------------------------------------------
// Traversal (FEAT) sets of the walks: meshes only (identity transforms) / + spheres /
// everything, each with the sequential or the cooperative (large-leaf) BVH walk.
// The list is split as the wavefront pipeline's two translation units are (compile time).
// ---------------------------------------------------------------------------
#define RTG_TRAV_FEATS_SMALL(X) X(0) X(FEAT_SPHERE) X(FEAT_ALL & ~FEAT_BIGLEAF)
#define RTG_TRAV_FEATS_BIG(X) X(FEAT_BIGLEAF) X(FEAT_SPHERE | FEAT_BIGLEAF) X(FEAT_ALL)

// the set a scene with features `feat` walks under (a superset of them)
constexpr int trav_feat(int feat) {
    const int base = feat & ~FEAT_BIGLEAF;
    return (base == 0 ? 0 : base == FEAT_SPHERE ? FEAT_SPHERE : FEAT_ALL & ~FEAT_BIGLEAF) | (feat & FEAT_BIGLEAF);
}

// fn(int_c<F>) with F = trav_feat(feat)
template <typename Fn>
auto with_trav_feat(int feat, Fn&& fn) {
    const int f = trav_feat(feat);
#define RTG_X(F) \
    if (f == (F)) return fn(int_c<(F)>{});
    RTG_TRAV_FEATS_SMALL(RTG_X)
    RTG_TRAV_FEATS_BIG(RTG_X)
#undef RTG_X
    __builtin_unreachable();
}

// Shadow rays (k_shadow*, occlusion queries) take the any-hit packet walk: the scene has an
// any-hit tree, its large leaves are split there or deferred (`defer_any`, renders only), and
// the reference walk is not asked for (RTG_RENDER_EXACT_SHADOW)
inline bool any_hit_wide(const DevScene& S, int feat, bool defer_any = false) {
    return S.anodes != nullptr && (!(feat & FEAT_BIGLEAF) || S.ahb_split || defer_any) && !S.exact_shadow;
}

// ---------------------------------------------------------------------------
// The fused kernel (k_render) and the radiance queries on its ray tree (k_radiance)
// ---------------------------------------------------------------------------
// Ray-tree levels of the largest frame stack: deeper scenes are refused at creation
constexpr int kMaxDepth = 32;
inline int max_supported_depth() { return kMaxDepth; }

// RTG_MEGA_GENERAL=1: the general instantiations always (A/B); read per launch
inline bool mega_general() { return std::getenv("RTG_MEGA_GENERAL") != nullptr; }

struct MegaVariant {
    int maxd;   // frame-stack depth: 0 (ray trees of depth 0), 8 or kMaxDepth
    bool pt;    // path-tracing camera
    int sk, feat;
    constexpr bool special() const { return sk != SK_ALL; }
};

// depth / pt / rr: the scene's MaxRecursionDepth, the camera's renderer flags; sk / feat: the
// scene's shading and traversal features; stats: a counted render; general: mega_general().
// General: (SK_ALL, FEAT_ALL), the kernels' default template arguments.  Special: scenes without
// textures or maps, instances or transforms -- BRDF shading with or without env / spot / mesh
// lights, meshes and spheres with small or large leaves; never counted, never at depth 0.
// Same code, same results: the bits only drop code the scene cannot reach.
constexpr MegaVariant mega_variant(int depth, bool pt, bool rr, int sk, int feat, bool stats, bool general) {
    // Russian roulette: unbounded GI recursion, cut at kMaxDepth ray-tree levels (the frame stack)
    const int maxd = pt ? (depth <= 8 && !rr ? 8 : kMaxDepth) : depth <= 0 ? 0 : depth <= 8 ? 8 : kMaxDepth;
    const bool special =
        !(sk & SK_TEX) && !(feat & (FEAT_INSTANCE | FEAT_XFORM)) && !general && !stats && (pt || depth > 0);
    if (!special) return {maxd, pt, SK_ALL, FEAT_ALL};
    return {maxd, pt, (sk & ~SK_BRDF) == 0 ? SK_BRDF : SK_BRDF | SK_XLIGHT, FEAT_SPHERE | (feat & FEAT_BIGLEAF)};
}

// fn(int_c<MAXD>, std::bool_constant<PT>) of a general variant: depth 0 for ray trees only
template <typename Fn>
auto with_general(const MegaVariant& v, Fn&& fn) {
    if (v.pt) return with_value<8, kMaxDepth>(v.maxd, [&](auto D) { return fn(D, std::true_type{}); });
    return with_value<0, 8, kMaxDepth>(v.maxd, [&](auto D) { return fn(D, std::false_type{}); });
}

// fn(int_c<MAXD>, int_c<SK>, int_c<FEAT>) of a special variant (PT is the caller's: the sets
// compile in one translation unit per renderer)
template <typename Fn>
auto with_special(const MegaVariant& v, Fn&& fn) {
    return with_value<8, kMaxDepth>(v.maxd, [&](auto D) {
        return with_value<SK_BRDF, SK_BRDF | SK_XLIGHT>(v.sk, [&](auto K) {
            return with_value<FEAT_SPHERE, FEAT_SPHERE | FEAT_BIGLEAF>(v.feat, [&](auto F) { return fn(D, K, F); });
        });
    });
}

// ---------------------------------------------------------------------------
// Smaller choices
// ---------------------------------------------------------------------------
// The wavefront path tracer's step kernel (uncounted renders; counted ones take (SK_ALL,
// FEAT_ALL)): shading BRDF / + env, spot, mesh lights / all; traversal meshes + spheres with
// small or large leaves / all
struct StepVariant {
    int sk, feat;
};
constexpr StepVariant step_variant(int sk, int feat) {
    return {(sk & ~SK_BRDF) == 0 ? SK_BRDF : (sk & ~(SK_BRDF | SK_XLIGHT)) == 0 ? SK_BRDF | SK_XLIGHT : SK_ALL,
            (feat & (FEAT_INSTANCE | FEAT_XFORM)) ? FEAT_ALL : FEAT_SPHERE | (feat & FEAT_BIGLEAF)};
}

// fn(int_c<SK>, int_c<FEAT>) with step_variant(sk, feat)
template <typename Fn>
auto with_step_variant(int sk, int feat, Fn&& fn) {
    const StepVariant v = step_variant(sk, feat);
    return with_value<SK_BRDF, SK_BRDF | SK_XLIGHT, SK_ALL>(v.sk, [&](auto K) {
        return with_value<FEAT_SPHERE, FEAT_SPHERE | FEAT_BIGLEAF, FEAT_ALL>(v.feat, [&](auto F) { return fn(K, F); });
    });
}

// k_tree_shade: scenes with plain shading (textures and maps at most) take the lean variant
constexpr int tree_shade_sk(int sk) { return (sk & ~SK_TEX) == 0 ? SK_TEX : SK_ALL; }

// k_multihit: the hit list's slots per field (registers), k in [1, RTG_MULTIHIT_MAX] rounded up
// to 2, 4 or 8
constexpr int multi_kmax(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : 8; }

}  // namespace rtg
