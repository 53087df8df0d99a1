// Device code shared by the render and query kernels: the umbrella over the topical headers
// below, in dependency order -- a header includes what it uses and nothing to its right
// (tests/test_headers_standalone.py compiles each one alone).
//
//   rtg_occupancy.hpp        waves per SIMD of every kernel family (RTG_*_WAVES)
//   rtg_math.hpp             DEV, RTG_GUARD / GIDX, f3, onb, xform, the RNG, the stats counters
//   rtg_isect.hpp            rays, slab and triangle tests, scalar record loads, keys, reductions
//   rtg_walk.hpp             the reference BVH walks, sphere_t, trav_ray, trace
//   rtg_anyhit.hpp           the any-hit tree's packet walks: shadow rays, ordered closest hit
//   rtg_shade.hpp            surface, textures, normal maps, environment, BRDFs, lights, direct
//   rtg_frame.hpp            camera rays, sample weights, pixel / tile / work indexing
//   rtg_shadow_kernels.hpp   k_shadow, k_bigleaf_any
//
// Numerics: this code is compiled with -ffp-contract=off and IEEE div/sqrt, and every
// expression keeps the reference's association and float/double choices, so the
// only differences from the CPU path are the last-ulp results of transcendental
// library calls (powf, acosf, expf, atan2f, double pow/cos).
#pragma once
#include "rtg_occupancy.hpp"
#include "rtg_math.hpp"
#include "rtg_isect.hpp"
#include "rtg_walk.hpp"
#include "rtg_anyhit.hpp"
#include "rtg_shade.hpp"
#include "rtg_frame.hpp"
#include "rtg_shadow_kernels.hpp"
