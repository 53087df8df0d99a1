// Occupancy knobs of the render kernels: the minimum waves per SIMD each kernel family is compiled
// for (__launch_bounds__'s second argument: the register budget is 512 / waves).  Every number is
// an A/B result; DESIGN.md §5 tells the rounds.
#pragma once
#include "rtg_device.hpp"

// The fused kernel at its natural 256 VGPR + AGPRs runs one wave per SIMD; two (a few hundred
// spilled registers) measured 5% faster on C2 and 40-60% faster on path tracing, four slower.
#ifndef RTG_MEGA_WAVES
#define RTG_MEGA_WAVES 2
#endif
// A fused-kernel build for four waves per SIMD faulted once in round 1 (an out-of-range scratch
// address in k_render<0>): guarded and plain rebuilds of this code did not
// reproduce it and no index of the kernel is out of range, but the cause is not identified, so
// builds above two waves stay experimental and must say so (make EXTRA="-DRTG_MEGA_WAVES=4
// -DRTG_MEGA_WAVES_EXPERIMENTAL=1").
#if RTG_MEGA_WAVES > 2 && !defined(RTG_MEGA_WAVES_EXPERIMENTAL)
#error "RTG_MEGA_WAVES > 2 is experimental (round-1 scratch fault, DESIGN.md §7): add -DRTG_MEGA_WAVES_EXPERIMENTAL=1"
#endif
// k_shade (212 VGPRs natural) at three waves: -17% kernel time on the headline; the tree
// pipeline's k_tree_shade at three costs C5 5%
#ifndef RTG_SHADE_WAVES
#define RTG_SHADE_WAVES 3
#endif
#ifndef RTG_TREE_SHADE_WAVES
#define RTG_TREE_SHADE_WAVES 1
#endif

// The reference walks (trace).  The traversal kernels of plain scenes (meshes with small leaves,
// spheres: 57-84 VGPRs) run at eight (+8% on C5); the large-leaf and transform variants (88-129
// VGPRs) keep their natural allocation -- eight costs C3 20-30%.
#ifndef RTG_LEAN_WAVES
#define RTG_LEAN_WAVES 8
#endif
// instance scenes' walks (camera and any-hit) at six waves: C4 2 944 -> 3 150 Mrays/s, C3-ton
// 5 450 -> 5 600 (profiles/r05n_pairs_inst6_deferany_ab.txt)
#ifndef RTG_INST_WAVES
#define RTG_INST_WAVES 6
#endif
#define RTG_TRACE_WAVES(FEAT) \
    (((FEAT) & ~FEAT_SPHERE) ? (((FEAT) & FEAT_INSTANCE) ? RTG_INST_WAVES : 1) : RTG_LEAN_WAVES)

// The any-hit packet walk (k_shadow<FAST>, the fused shade kernel: the wide walk + the in-place
// reference fallback).  Headline k_shade_shadow at five waves 0.193 ms, six 0.1804, seven 0.1742,
// eight 0.270 (spills); large-leaf configurations unchanged (profiles/r04ad_wide_waves_ab.txt,
// r04ae_wide_waves_configs_ab.txt)
#ifndef RTG_WIDE_WAVES_PLAIN
#define RTG_WIDE_WAVES_PLAIN 7
#endif
// instance scenes' any-hit walks (their own knob): the deferring shadow walk spills 124 B per
// lane at six waves, 76 at five and none at four (118 VGPRs), and six is the fastest -- C4
// 3 163 / 3 093 / 2 963 Mrays/s (profiles/r05w_c4_any_waves_ab.txt): occupancy over spill traffic
#ifndef RTG_INST_ANY_WAVES
#define RTG_INST_ANY_WAVES 6
#endif
#define RTG_WIDE_WAVES(FEAT) (((FEAT) & FEAT_INSTANCE) ? RTG_INST_ANY_WAVES : RTG_WIDE_WAVES_PLAIN)
