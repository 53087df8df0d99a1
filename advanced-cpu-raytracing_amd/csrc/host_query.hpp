// Host-only ray queries over a scene description (rtgpu.h rtg_desc_trace_rays).
#pragma once

#include <cstdint>
#include <string>

#include "rtgpu.h"

namespace rtg {

// The reference's IntersectObjects / CastShadowRay for n rays over the description's own BVH
// nodes; normals nullable (4 floats per ray, closest hit only).  Returns an rtg_status; `err`
// describes a failure.
int host_trace_rays(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_hit* hits,
                    float* normals, std::string& err);

// The same walk keeping the k nearest hits per ray (rtgpu.h rtg_desc_trace_rays_multi): hits n * k,
// ray-major; counts nullable.
int host_trace_rays_multi(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags,
                          rtg_hit* hits, int32_t* counts, std::string& err);

// Closest-point queries (rtgpu.h rtg_desc_closest_points): the nearest surface point to each
// point, by the walk that defines the query (the yardstick of k_closest, bit for bit).
int host_closest_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, uint32_t flags, rtg_nearest* out,
                        std::string& err);
// RTG_OK, or RTG_ERR_UNSUPPORTED with the message naming the first object whose record lacks
// PXF_SPHERE_OK (a sphere that the scene's transform makes an ellipsoid).
struct PointXf;
int closest_unsupported(const PointXf* xf, int num_objects, std::string& err);

// Crossing counts (rtgpu.h rtg_desc_count_crossings): per ray the number of accepted hits and how
// many of them enter, by the walk that defines the query (the yardstick of k_crossings).
int host_count_crossings(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_crossings* out,
                         std::string& err);
// Signed distances (rtgpu.h rtg_desc_signed_distance_points): the closest-point walk, then the
// crossing walk from the point along dir (nullable: the default direction).
int host_signed_distance_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, const float* dir,
                                uint32_t flags, rtg_nearest* out, std::string& err);
// dir (nullable: the documented default) into out[3]; null, or what is wrong with it
const char* signed_distance_dir(const float* dir, float out[3]);

}  // namespace rtg
