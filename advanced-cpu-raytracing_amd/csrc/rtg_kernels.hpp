#pragma once

#include <hip/hip_runtime.h>

#include "rtg_device.hpp"
#include "rtg_pointxf.hpp"
#include "rtg_variants.hpp"
#include "rtgpu.h"

namespace rtg {

// large leaves of the camera walk deferred to k_bigleaf (rtg_wave_shade.hip; RTG_DEFER=0: off)
bool defer_leaves();
// FNV-1a of a camera's device record (view, image size, samples, renderer flags): the ray-tree and
// path plans are kept per frame part of one camera
inline unsigned long long camera_hash(const DevCamera& C) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&C);
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < sizeof(DevCamera); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
// fused kernel (rtg_mega.hip): any scene
// `ev` (nullable): events recorded around every kernel of the last sample pass
// sk / feat: the scene's shading / traversal features (rtg_variants.hpp mega_variant)
hipError_t launch_mega(const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr, unsigned char* ldr,
                       float* accum, DevCounters* counters, bool stats, int sk, int feat, hipStream_t stream,
                       hipEvent_t* ev);
// its special variants `v` (v.special()): path tracing (rtg_mega_pt.hip), ray trees (rtg_mega_wh.hip)
hipError_t launch_mega_pt(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P,
                          float* hdr, unsigned char* ldr, float* accum, DevCounters* counters, hipStream_t stream);
hipError_t launch_mega_wh(const MegaVariant& v, const DevScene& S, const DevCamera& C, const RenderParams& P,
                          float* hdr, unsigned char* ldr, float* accum, DevCounters* counters, hipStream_t stream);
// wavefront pipeline (rtg_wave.hip): scenes without secondary rays / motion blur
hipError_t launch_wave(const DevScene& S, const DevCamera& C, const RenderParams& P, const WaveBufs& W, float* hdr,
                       unsigned char* ldr, DevCounters* counters, bool stats, int feat, int sk, hipStream_t stream,
                       hipEvent_t* ev, int* layout);
// wavefront ray trees (rtg_tree.hip): scenes with mirror / conductor / dielectric materials;
// host-synchronous per tree level (the next level's size); state (buffers) kept in `tree`
struct TreeState;
void tree_destroy(TreeState* tree);
hipError_t launch_tree(TreeState*& tree, const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr,
                       unsigned char* ldr, float4* accum, DevCounters* counters, bool stats, int feat, int sk,
                       hipStream_t stream, hipEvent_t* ev);
// wavefront path tracing (rtg_path.hip): path-tracing cameras without motion blur; path
// queues and frame stacks kept in `path`.  hipErrorNotSupported: a pass needed more than
// its iteration bound (the caller renders with the fused kernel instead)
struct PathState;
void path_destroy(PathState* path);
hipError_t launch_path(PathState*& path, const DevScene& S, const DevCamera& C, const RenderParams& P, float* hdr,
                       unsigned char* ldr, float4* accum, DevCounters* counters, bool stats, int feat, int sk,
                       hipStream_t stream, hipEvent_t* ev);
// photographic tonemapper (rtg_tonemap.hip); scratch of tonemap_scratch_bytes()
size_t tonemap_scratch_bytes(long long pixels);
size_t tonemap_avg_offset();   // byte offset of the log-average luminance (double) in the scratch
void launch_log_average(const float* hdr, long long n, int mode, uint32_t idx, void* scratch, hipStream_t st);
hipError_t launch_tonemap(const float* hdr, int width, int height, float key, float burn, float saturation,
                          float gamma, unsigned char* ldr, void* scratch, hipStream_t stream);
// device scene ingest (rtg_bvh.hip): the reference's midpoint BVH of one mesh built on the
// GPU from its faces in parse order (d_faces, device copy of the desc's), written as walk
// records at node index nodeBase and as face arrays at faceOff (BVH order); d_perm
// (nullable) receives the final order (mesh-local indices).  Synchronises `st`.
hipError_t build_mesh_bvh(const rtg_face* d_faces, int n, const float root_mn[3], const float root_mx[3],
                          int faceOff, int nodeBase, float4* d_nodes, int2* d_ext, float4* d_tris, float4* d_fn,
                          float2* d_fuv, float4* d_v12, int* d_perm, int* nodeCount, bool* bigleaf,
                          hipStream_t st);
// ray queries (rtg_query.hip): one ray per lane.  launch_query: closest hit (IntersectObjects) or,
// with RTG_QUERY_ANY_HIT, occlusion (CastShadowRay) of n rays; normals nullable (closest hit only).
// launch_camera_rays: the camera rays of rows [row_begin, row_end) at `sample`, in pixel order.
hipError_t launch_query(const DevScene& S, int feat, const rtg_ray* rays, int n, uint32_t flags, rtg_hit* hits,
                        float4* normals, hipStream_t stream);
hipError_t launch_camera_rays(const DevCamera& C, int row_begin, int row_end, int sample, unsigned long long seed,
                              rtg_ray* rays, hipStream_t stream);
// multi-hit queries (rtg_multihit.hip): the k nearest hits of n rays (k in [1, RTG_MULTIHIT_MAX]), one
// ray per lane; hits: n * k records, ray-major; counts nullable (filled slots per ray).
hipError_t launch_multihit(const DevScene& S, int feat, const rtg_ray* rays, int n, int k, rtg_hit* hits, int* counts,
                           hipStream_t stream);
// closest-point queries (rtg_closest.hip): the nearest surface point to each of n points, one point
// per lane; xf: the per-object placement records (rtg_pointxf.hpp), num_objects of them.
hipError_t launch_closest(const DevScene& S, const PointXf* xf, int feat, const rtg_point* points, int n,
                          rtg_nearest* out, hipStream_t stream);
// crossing counts (rtg_crossings.hip): per ray the number of hits with 0 < t < tmax and how many of
// them enter, one ray per lane; no bound on the number.
hipError_t launch_crossings(const DevScene& S, int feat, const rtg_ray* rays, int n, rtg_crossings* out,
                            hipStream_t stream);
// signed distances (rtg_crossings.hip): launch_closest's record per point, then the crossing walk
// from the point along dir (three floats, host memory, passed by value): the count in pad0, an odd
// one on a hit's sign bit.  feat: launch_closest's (a superset of the ray walks').
hipError_t launch_signed_distance(const DevScene& S, const PointXf* xf, int feat, const rtg_point* points, int n,
                                  const float dir[3], rtg_nearest* out, hipStream_t stream);
// surface queries (rtg_surface.hip): closest hit of n rays, one ray per lane, with the hit's shading
// normal (normal / bump maps applied), texture coordinates, geometric normal, material and
// GetDiffuse's coefficient; flags: RTG_QUERY_COHERENT only.  sk / feat as for launch_mega (a scene
// without SK_TEX runs the variant compiled without maps and texture fetches: the same values).
hipError_t launch_surface(const DevScene& S, int sk, int feat, const rtg_ray* rays, int n, uint32_t flags, rtg_surface* out,
                          hipStream_t stream);
// radiance queries (rtg_radiance.hip): the fused kernel's ray tree below n caller rays, one ray per
// lane; ray i plays pixel ids ? ids[i] : first_pixel + i (RNG key, background-texture lookup).
// Of C: the renderer flags, width / height and -- with camera_eye -- the position.  sk / feat as
// for launch_mega.  rgbt: 4 floats per ray (colour, the primary hit's t).
struct RadianceParams {
    int n, first_pixel;
    int sample_begin, sample_count;
    int camera_eye, pad0;
    unsigned long long seed;
};
hipError_t launch_radiance(const DevScene& S, const DevCamera& C, const RadianceParams& P, int sk, int feat,
                           const rtg_ray* rays, const int* ids, float* rgbt, hipStream_t stream);
enum { WAVE_STAGES = 4, MEGA_STAGES = 1, TREE_STAGES = 2, PATH_STAGES = 1, MAX_STAGES = 4 };
// Timed stage layouts (RTG_RENDER_TIMING): which kernels ran between the recorded events.
enum { LAYOUT_WAVE = 0,          // k_primary, k_shade, k_shadow, k_resolve
       LAYOUT_WAVE_ONE = 1,      // k_primary, k_shade, k_shadow (k_shadow_one finishes pixels)
       LAYOUT_WAVE_FUSED = 2,    // k_primary, k_shade_shadow
       LAYOUT_TREE = 3, LAYOUT_MEGA = 4,
       LAYOUT_PATH = 5,            // the last sample pass of the wavefront path tracer
       LAYOUT_WAVE_FRAME = 6 };    // k_frame: the fused layout's whole sample pass in one kernel

}  // namespace rtg
