// Host-only conversion of an rtg_scene_desc into every table the kernels read
// (rtg_device.hpp).  No HIP runtime call: rtg_scene_create validates, builds these tables and
// uploads them; rtg_desc_anyhit_check and the CPU test (tests/scene_tables_main.cpp) stop
// after the build.  Host sources only include this header, never a .hip file's header.
#pragma once
#include <hip/hip_runtime.h>   // vector types only

#include <string>
#include <vector>

#include "rtg_ahb.hpp"
#include "rtg_device.hpp"
#include "rtg_pointxf.hpp"
#include "rtgpu.h"

namespace rtg {

// The environment's knobs, read once by the caller (the builder reads no environment variable).
struct TableOptions {
    bool fast_shadow = true;        // any-hit trees and face -> leaf (off: shadow rays walk the reference BVH)
    AhbMode ahb_mode = AHB_EXACT;
    bool coop = true;               // large-leaf scenes take the cooperative walk (FEAT_BIGLEAF)
    bool verbose = false;           // any-hit tree statistics on stderr
};

// What the device BVH build (rtg_bvh.hip) hands back.  nodes / ext / tris are host copies of
// the walk records and are only needed with TableOptions::fast_shadow.
struct BvhReadback {
    std::vector<float4> nodes, tris;
    std::vector<int2> ext;
    std::vector<int> perm;          // final face position -> description face
    std::vector<int> mesh_begin, mesh_end;
    bool bigleaf = false;
    int node_count = 0;             // nodes in use, the pad node included
};

struct SceneTables {
    // walk and face tables (empty with a read-back: the device build wrote them in place)
    std::vector<float4> nodes, tris, face_n, face_v12;
    std::vector<int2> node_ext;
    std::vector<float2> face_uv;
    std::vector<DevObject> objects;
    std::vector<float4> group_box;
    std::vector<PointXf> point_xf;      // per object: the closest-point queries' placement record (rtg_pointxf.hpp)
    std::vector<DevMaterial> materials;
    std::vector<DevBrdf> brdfs;
    std::vector<DevTexture> textures;
    std::vector<DevImage> images;
    std::vector<float> texels;
    std::vector<DevPointLight> point_lights;
    std::vector<DevAreaLight> area_lights;
    std::vector<DevDirLight> dir_lights;
    std::vector<DevSpotLight> spot_lights;
    std::vector<int> env_images;
    std::vector<unsigned long long> env_mix;
    std::vector<DevMeshLight> mesh_lights;
    std::vector<DevLightFace> light_faces;
    std::vector<WNode> anodes;
    std::vector<float4> ahtris;
    std::vector<int> face_leaf;
    std::vector<int> perm;
    std::vector<float> grad;
    // per mesh: its node range and its root in anodes (-1: none)
    std::vector<int> mesh_begin, mesh_end, aroot;
    int node_count = 0;             // nodes in use, the pad node included
    int feat = 0, shade_sk = 0, num_slots = 0;
    bool wave_ok = false, tree_ok = false, path_ok = false;
    int ahb_mode = AHB_EXACT;       // the mode the any-hit trees were built in
    bool ahb_split = false;
    bool ahb_ok = true;             // false: a leaf range exceeded the trees' encoding (no trees built)
    bool bigleaf = false;           // a leaf of more than kBigLeaf faces (FEAT_BIGLEAF with TableOptions::coop)
    AhbStats ahb;
};

// What a scene keeps of its creation for update_scene_tables: the results of the geometry's
// processing that the mutable tables refer to, and the signature a later description must match
// (rtgpu.h, rtg_scene_update's same-geometry contract).
struct KeptTables {
    std::vector<int> mesh_begin, mesh_end, aroot;   // aroot empty: no any-hit trees were asked for
    bool bigleaf = false;
    int ahb_mode = AHB_EXACT;
    bool ahb_ok = true, ahb_split = false;
    bool has_uv = false, has_v12 = false;           // face_uv / face_v12 exist (any_uv / any_mapped at creation)
    std::vector<int> light_face_begin, light_face_count, light_object;   // per mesh light
    std::vector<long long> image_offset;            // per image, into the texel pool
    struct Mesh { int face_offset, face_count, node_offset, node_count, has_uv; };
    struct Image { int width, height, channels, is_hdr; };
    long long num_faces = 0, num_nodes = 0;
    std::vector<Mesh> meshes;
    std::vector<int2> objects;                      // kind, mesh
    std::vector<Image> images;
};

// scenes with UVs carry face_uv, scenes with a normal / bump map in effect face_v12
bool any_uv(const rtg_scene_desc* d);
bool any_mapped(const rtg_scene_desc* d);

// Every check on a description; RTG_OK or the code, with the message in `err`.
int validate_desc(const rtg_scene_desc* d, std::string& err);
// The same without the checks that read geometry (face count, BVH links, texels): what an update
// re-checks.  The description's meshes[] and the objects' mesh indices must be valid already.
int validate_desc_update(const rtg_scene_desc* d, std::string& err);

// `rb` null: the description's own BVH, re-laid in pre-order.
int build_scene_tables(const rtg_scene_desc* d, const TableOptions& opt, const BvhReadback* rb, SceneTables& T,
                       std::string& err);

// The kept state of tables just built from `d`.
void keep_tables(const rtg_scene_desc* d, const SceneTables& T, KeptTables& K);
// RTG_OK when `d` matches the signature in K, else RTG_ERR_INVALID with the first difference.
int same_geometry(const rtg_scene_desc* d, const KeptTables& K, std::string& err);
// The mutable tables and scalars of `d` over the geometry K was kept from: objects, group_box,
// point_xf, materials, brdfs, textures, the image records, the four analytic light arrays, env_images,
// env_mix, the mesh-light records, feat, shade_sk, num_slots, wave_ok, tree_ok, path_ok (and
// mesh_begin / mesh_end / aroot / the ahb_* flags, copied from K) -- each equal, byte for byte, to
// build_scene_tables(d)'s; every other table of T is left empty.  Reads neither d->faces, d->nodes
// nor any texel.  `opt`: the options of the creation.  Checks same_geometry and
// validate_desc_update first; RTG_ERR_UNSUPPORTED for a map that needs face_v12 where K has none
// and for split any-hit trees.
int update_scene_tables(const rtg_scene_desc* d, const KeptTables& K, const TableOptions& opt, SceneTables& T,
                        std::string& err);

}  // namespace rtg
