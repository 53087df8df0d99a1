// The closest-point queries' per-object side table (rtgpu.h rtg_closest_points*): what a point
// query needs of an object's placement, in float, beside DevObject (which stays the ray walks').
// Built by point_xf_record (scene_tables.cpp) from rtg_object.transform / inv_transform, for the
// device table (SceneTables::point_xf, updated by rtg_scene_update) and for the host walk
// (host_query.cpp) alike, so both read the same bits.  No dependency: host and device sources.
#pragma once

#include "rtgpu.h"

namespace rtg {

enum : int {
    PXF_IDENTITY = 1,    // transform is exactly the identity: no transform arithmetic on either side
    PXF_SPHERE_OK = 2    // not a sphere, or a sphere under a similarity (it stays a sphere)
};

struct PointXf {
    float fwd[12];       // rows 0..2 of transform, narrowed to float
    float inv[12];       // rows 0..2 of inv_transform, narrowed to float
    float lip2;          // sigma_max(inv 3x3)^2 * (1 + 1e-5), rounded up: local d2 <= lip2 * world d2
    float scale;         // spheres: cbrt(|det transform 3x3|), the similarity's factor
    int flags, pad0;
};
static_assert(sizeof(PointXf) == 112, "seven 16-byte words");

void point_xf_record(const rtg_object& o, PointXf& X);

}  // namespace rtg
