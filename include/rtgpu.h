/*
 * rtgpu.h -- C-ABI drop-in boundary for the per-pixel trace/shade hot path of
 * dorukb/Advanced-CPU-Raytracing, re-implemented as hand-written HIP for gfx950.
 *
 * The reference has no plugin/FFI API: its only seam between the CLI driver and
 * the hot path is
 *     Vec3f DorkTracer::Raytracer::RenderPixel(int i, int j, Camera& cam)
 *         (src/raytracer.hpp:19, src/raytracer.cpp:33-36)
 * called once per pixel-sample by renderThreadMain (src/main.cpp:26-130) from the
 * 8-thread row-band block of main() (src/main.cpp:142-196).  This header replaces
 * that block with ONE call per camera (rtg_render), and the scene object graph
 * (src/scene.h:32-89) with a flattened POD description (rtg_scene_desc).
 *
 * Conventions: plain C, no C++ types, no exceptions across the ABI.  Every
 * function returns 0 (RTG_OK) or a negative RTG_ERR_* code; rtg_last_error()
 * returns a thread-local description of the last failure.  Buffers passed in are
 * owned by the caller and never freed by the library.
 */
#ifndef RTGPU_H
#define RTGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTG_ABI_VERSION 6

enum rtg_status {
    RTG_OK = 0,
    RTG_ERR_INVALID = -1,     /* bad argument / inconsistent scene description      */
    RTG_ERR_IO = -2,          /* file could not be read / written                    */
    RTG_ERR_PARSE = -3,       /* malformed XML / PLY / image                         */
    RTG_ERR_HIP = -4,         /* HIP runtime error (no device, launch failure, ...)  */
    RTG_ERR_NOMEM = -5,       /* host or device allocation failed                    */
    RTG_ERR_UNSUPPORTED = -6  /* feature outside the implemented hot path            */
};

/* ------------------------------------------------------------------------- */
/* Flattened scene description (all host memory, produced by the XML loader   */
/* below or by any other front end, e.g. an adapter over the reference's own  */
/* DorkTracer::Scene -- see INTEGRATION.md).                                   */
/* ------------------------------------------------------------------------- */

typedef struct { float x, y, z; } rtg_float3;

/* material.hpp:14-20 */
enum rtg_material_type {
    RTG_MAT_MIRROR = 0, RTG_MAT_DIELECTRIC = 1, RTG_MAT_CONDUCTOR = 2,
    RTG_MAT_EMISSIVE = 3, RTG_MAT_DEFAULT = 4
};

/* Material (material.hpp:8-48).  Index in rtg_scene_desc.materials is the
 * reference's matId-1 (raytracer.cpp:73). */
typedef struct {
    int32_t id;
    int32_t type;            /* rtg_material_type */
    int32_t brdf;            /* index into brdfs[] or -1 (Material::brdf == nullptr) */
    int32_t pad0;
    rtg_float3 ambient, diffuse, specular, mirror;
    float phong_exponent;
    float refractive_index;
    float absorption_index;  /* conductorAbsorptionIndex */
    float roughness;
    rtg_float3 absorption;   /* absorptionCoefficient (Beer's law) */
    rtg_float3 radiance;     /* emissive materials only */
} rtg_material;

/* BRDF kinds (parser.cpp:870-982, brdf*.cpp) */
enum rtg_brdf_type {
    RTG_BRDF_PHONG = 0,               /* <OriginalPhong>       brdfPhong.cpp              */
    RTG_BRDF_BLINN_PHONG = 1,         /* <OriginalBlinnPhong>  brdfBlinnPhong.cpp         */
    RTG_BRDF_MODIFIED_PHONG = 2,      /* <ModifiedPhong>       brdfModifiedPhong.cpp      */
    RTG_BRDF_MODIFIED_BLINN_PHONG = 3,/* <ModifiedBlinnPhong>  brdfModifiedBlinnPhong.cpp */
    RTG_BRDF_TORRANCE_SPARROW = 4     /* <TorranceSparrow>     brdfTorranceSparrow.cpp    */
};
typedef struct {
    int32_t id, type;
    float exponent;
    int32_t energy_conserving;   /* BRDF::isEnergyConserving ("normalized" attribute) */
    int32_t kd_fresnel;          /* TorranceSparrow "kdfresnel" */
    int32_t pad0;
} rtg_brdf;

/* Lights (pointLight.h, areaLight.h, directionalLight.h, spotLight.h,
 * sphericalEnvironmentLight.h).  Evaluated in this type order
 * (raytracer.cpp:706-803). */
typedef struct { rtg_float3 position, intensity; } rtg_point_light;
typedef struct {
    rtg_float3 position, normal, radiance;
    rtg_float3 u, v;          /* GetOrthonormalBasis(normal) (areaLight.h:30) */
    float extent, area;
} rtg_area_light;
typedef struct { rtg_float3 dir /* unit */, radiance; } rtg_directional_light;
typedef struct {
    rtg_float3 position, dir /* unit */, intensity;
    float coverage_deg, falloff_deg;
    double cos_half_coverage, cos_half_falloff;   /* spotLight.h:24-25 */
} rtg_spot_light;
typedef struct { int32_t image; int32_t pad0; } rtg_env_light;
/* MeshLight (meshLight.h:9-47), in scene.meshLights order (parser.cpp:1474-1481).
 * object: its index in objects[] (a LightMesh entry); radiance: its own <Radiance> --
 * the emissive material carries the radiance of the LAST LightMesh sharing it
 * (parser.cpp:1484-1487), the light keeps its own (raytracer.cpp:800). */
typedef struct { int32_t object; rtg_float3 radiance; } rtg_mesh_light;

/* Images: texels stored as float, w*h*channels, row-major (LDRImage.h:16-26 keeps
 * the raw 0..255 byte values; HDRImage.h keeps linear floats). */
typedef struct {
    int32_t id, width, height, channels;
    int32_t is_hdr, pad0;
    const float* texels;
} rtg_image;

enum rtg_texture_kind { RTG_TEX_IMAGE = 0, RTG_TEX_PERLIN = 1 };
/* Texture::Textures (texture.h:31-38) plus the replace_background decal */
enum rtg_texture_slot {
    RTG_TEXSLOT_DIFFUSE = 0, RTG_TEXSLOT_SPECULAR = 1, RTG_TEXSLOT_BUMP = 2,
    RTG_TEXSLOT_NORMAL = 3, RTG_TEXSLOT_REPLACE_ALL = 4, RTG_TEXSLOT_NONE = 5
};
typedef struct {
    int32_t id, kind, slot;
    int32_t blend;            /* OperationMode::Blend (decal "blend_kd") */
    int32_t is_background;    /* decal "replace_background" */
    int32_t image;            /* image textures: index into images[] or -1 */
    int32_t nearest;          /* image textures: 1 = nearest, 0 = bilinear */
    float normalizer, bump_factor;
    float noise_scale;        /* perlin */
    int32_t noise_abs;        /* perlin: 1 = "absval", 0 = "linear" */
    int32_t pad0;
} rtg_texture;

/* Objects in the reference's IntersectObjects order (raytracer.cpp:625-643):
 * scene.meshes (Mesh, LightMesh, MeshInstance, Triangle-as-1-face-Mesh;
 * parser.cpp:348-512) followed by scene.spheres (parser.cpp:514-574). */
enum rtg_object_kind { RTG_OBJ_MESH = 0, RTG_OBJ_INSTANCE = 1, RTG_OBJ_SPHERE = 2 };
enum rtg_object_flags {
    RTG_OBJF_SHADOW_SKIP = 1,    /* emissive mesh: skipped by CastShadowRay (raytracer.cpp:590) */
    RTG_OBJF_NORMAL_TWICE = 2,   /* geometry has no UVs: IntersectFace applies the normal
                                    transform once more (mesh.cpp:362-364)               */
    RTG_OBJF_MOTION_BLUR = 4
};
typedef struct {
    int32_t kind;                /* rtg_object_kind */
    int32_t material;            /* 0-based index into materials[] */
    int32_t mesh;                /* geometry index into meshes[] (mesh/instance) */
    int32_t flags;               /* rtg_object_flags */
    int32_t tex_diffuse, tex_specular, tex_normal, tex_bump, tex_replace_all;
    int32_t id;
    /* 4x4 row-major double matrices (matrix.hpp).  For instances inv_transform and
     * inv_transpose are the instance's composed matrices (parser.cpp:429-451) and
     * base_inv_transpose is the base mesh's own (applied first by IntersectFace). */
    double inv_transform[16];
    double inv_transpose[16];
    double base_inv_transpose[16];
    double transform[16];
    float bbox_min[3], bbox_max[3];   /* mesh: local bbox (parser.cpp:1392-1468, with the
                                         FLT_MIN max-corner quirk); instance: world bbox
                                         (parser.cpp:749-805)                            */
    rtg_float3 motion_blur;
    rtg_float3 center;           /* sphere (local space) */
    float radius;
    int32_t pad0;
} rtg_object;

/* Triangle geometry with its BVH in the reference's topology (mesh.cpp:23-156). */
typedef struct {
    int32_t face_offset, face_count;   /* into faces[]   */
    int32_t node_offset, node_count;   /* into nodes[]   */
    int32_t has_uv;
    int32_t id;
    double surface_area;
} rtg_mesh;

/* Faces in the final BVH-permuted order (mesh.cpp:92-102 swaps faces in place). */
typedef struct {
    rtg_float3 v0, v1, v2;      /* object-space vertices (mesh.cpp:203-205) */
    rtg_float3 n;               /* makeUnit(cross(v1-v0, v2-v0)) (parser.cpp:724-733) */
    float uv0[2], uv1[2], uv2[2];
    double area;
} rtg_face;

/* BVH nodes, indices relative to the owning mesh's node_offset; node 0 is the
 * root; children are allocated pairwise (right == left + 1, mesh.cpp:109-122). */
typedef struct {
    float bmin[3], bmax[3];
    int32_t left;               /* -1 for a leaf */
    int32_t first, count;       /* leaf face range (relative to face_offset) */
    int32_t pad0;
} rtg_bvh_node;

/* Camera after Camera::SetupDefault / SetupLookAt (camera.cpp:5-72). */
typedef struct {
    rtg_float3 position, gaze, up, right, q;   /* q = m_q, image-plane corner */
    float left, right_ext, bottom, top, near_dist;
    int32_t width, height, spp;
    float focus_distance, aperture;
    int32_t has_tonemapper;
    float tm_key, tm_burn, tm_saturation, tm_gamma;
    int32_t path_tracing, importance_sampling, next_event, russian_roulette;
    char image_name[256];
} rtg_camera;

typedef struct {
    int32_t background[3];            /* BackgroundColor (integer, parser.cpp:47-53) */
    float shadow_epsilon;             /* Scene::shadow_ray_epsilon */
    int32_t max_recursion_depth;
    int32_t bg_texture;               /* replace_background texture index or -1 */
    rtg_float3 ambient_light;

    const rtg_camera* cameras;        int32_t num_cameras;
    const rtg_material* materials;    int32_t num_materials;
    const rtg_brdf* brdfs;            int32_t num_brdfs;
    const rtg_point_light* point_lights;          int32_t num_point_lights;
    const rtg_area_light* area_lights;            int32_t num_area_lights;
    const rtg_directional_light* dir_lights;      int32_t num_dir_lights;
    const rtg_spot_light* spot_lights;            int32_t num_spot_lights;
    const rtg_env_light* env_lights;              int32_t num_env_lights;
    const rtg_texture* textures;      int32_t num_textures;
    const rtg_image* images;          int32_t num_images;
    const rtg_object* objects;        int32_t num_objects;
    const rtg_mesh* meshes;           int32_t num_meshes;
    const rtg_face* faces;            int64_t num_faces;
    const rtg_bvh_node* nodes;        int64_t num_nodes;
    const rtg_mesh_light* mesh_lights; int32_t num_mesh_lights;
    int32_t pad0;
} rtg_scene_desc;

/* ------------------------------------------------------------------------- */
/* Host ingest: the XML scene format of the reference.                        */
/* ------------------------------------------------------------------------- */
typedef struct rtg_host_scene rtg_host_scene;

/* Replaces DorkTracer::Scene::loadFromXml (parser.cpp:26-577), called from
 * main.cpp:135-137.  Relative asset paths follow the reference: PLY files are
 * opened relative to the current directory (parser.cpp:1404), images as
 * "inputs/<name>" (parser.cpp:107,110). */
int rtg_host_scene_load_xml(const char* xml_path, rtg_host_scene** out);
/* Load flags.  RTG_LOAD_DEVICE_BVH: skip the host BVH build (mesh.cpp:23-156); the
 * description then holds faces in parse order, num_nodes == 0 and every mesh's node range
 * empty, and rtg_scene_create builds the same BVH and face order on the GPU (SURVEY §8f,
 * device scene ingest).  Such a description is for rtg_scene_create only. */
enum rtg_load_flags { RTG_LOAD_DEVICE_BVH = 1 };
int rtg_host_scene_load_xml_ex(const char* xml_path, uint32_t flags, rtg_host_scene** out);
/* The flattened description; valid until rtg_host_scene_free. */
const rtg_scene_desc* rtg_host_scene_desc(const rtg_host_scene* hs);
void rtg_host_scene_free(rtg_host_scene* hs);
/* Convenience accessors (cameras: scene.cameras[i], main.cpp:142-152). */
int rtg_desc_camera_info(const rtg_scene_desc* desc, int camera, int32_t* width,
                         int32_t* height, int32_t* spp, int32_t* has_tonemapper);
int rtg_desc_counts(const rtg_scene_desc* desc, int64_t* num_objects, int64_t* num_faces,
                    int64_t* num_nodes, int64_t* num_lights);
/* Diagnostic (ABI 5, host only, no device): builds the shadow rays' any-hit trees of a
 * description with a BVH as rtg_scene_create does (mode 0 = the reference's BVH collapsed,
 * 1 = binned SAH over its leaves, the default, 2 = large leaves split into faces) and checks
 * them -- every face reached once, box nesting, triangle containment.  out[0..7] = wide
 * nodes, leaf entries, depth, whole-leaf primitives, split faces, split faces kept on their
 * leaf box, violations, built (1) or not (0: leaf encoding exceeded). */
int rtg_desc_anyhit_check(const rtg_scene_desc* desc, int32_t mode, int64_t* out, int32_t n_out);

/* ------------------------------------------------------------------------- */
/* Device scene + render                                                      */
/* ------------------------------------------------------------------------- */
typedef struct rtg_scene rtg_scene;

/* Replaces Raytracer::Raytracer(Scene&) (raytracer.cpp:7-16, which copies the
 * scene): uploads a device-resident replica of `desc` to HIP device `device`.
 * The caller may free `desc` after return.  At most 2^25 faces (RTG_ERR_INVALID
 * beyond: the traversal kernels address records by 32-bit byte offsets). */
int rtg_scene_create(const rtg_scene_desc* desc, int device, rtg_scene** out);
/* The device's traversal data, for inspection and tests: the walk's node records (8 floats
 * per node, pre-order layout of the BVH nodes, the trailing pad node included) and the
 * per-face triangle records (12 floats per face, BVH face order).  Either buffer may be
 * NULL; counts are reported even when the buffers are too small (then nothing is copied). */
int rtg_scene_export_bvh(const rtg_scene* s, float* nodes, int64_t max_nodes, float* tris, int64_t max_faces,
                         int64_t* num_nodes, int64_t* num_faces);
void rtg_scene_destroy(rtg_scene* scene);
int rtg_device_count(int32_t* count);

/* Multi-GPU scene (replaces the reference's 8 row-band threads,
 * main.cpp:38-39,164-185, with the GPUs of one node): one device-resident replica per
 * entry of `devices`, each with its own stream (an entry may repeat: several replicas on
 * one device).  rtg_render on such a scene deals the frame to the replicas -- replica i
 * renders part i of num_devices (rtg_render_opts.part_index) -- and each copies its rows
 * straight into the caller's host buffers: the host framebuffer gather, no collective.
 * rtg_render_device, rtg_scene_timings and rtg_scene_export_bvh use the first replica;
 * rtg_scene_stats sums all replicas. */
int rtg_scene_create_multi(const rtg_scene_desc* desc, const int32_t* devices, int32_t num_devices,
                           rtg_scene** out);
int rtg_scene_num_devices(const rtg_scene* scene, int32_t* num_devices);

enum rtg_render_flags {
    RTG_RENDER_COUNT_STATS = 1,   /* accumulate rtg_stats (slower kernel variant)      */
    RTG_RENDER_ACCUM_ONLY = 2,    /* write the weighted sample sum (r,g,b,w) only; used
                                     when samples are split across devices            */
    RTG_RENDER_FUSED = 4,         /* force the fused per-pixel kernel even where the
                                     wavefront pipeline applies (for cross-checks)     */
    RTG_RENDER_TIMING = 8,        /* record HIP events around every kernel of the
                                     render (last sample pass); see rtg_scene_timings */
    RTG_RENDER_TREE = 16,         /* force the wavefront ray-tree pipeline for scenes with
                                     mirror / conductor / dielectric materials (default:
                                     frames of >= 2^21 pixel-samples; one stream
                                     synchronisation per render once its level sizes are
                                     planned).  ABI 5: for path-tracing cameras, the
                                     wavefront path tracer (opt-in; same image as the
                                     fused kernel bit for bit)                         */
    RTG_RENDER_EXACT_SHADOW = 32, /* shadow rays walk the reference BVH instead of the
                                     any-hit wide BVH (same answers; for cross-checks)  */
    RTG_RENDER_ORDERED = 64,      /* opt-in (ABI 4): camera rays of plain mesh scenes walk
                                     the 4-wide BVH nearest child first with a checked
                                     result (the reference walk where the check fails);
                                     agreement with the reference order is measured, not
                                     proven -- DESIGN.md §5                          */
    RTG_RENDER_SAMPLE_PASSES = 128 /* ABI 6: one sample per pass.  By default the wavefront
                                     and ray-tree pipelines carry several consecutive
                                     samples of the rendered pixels in one pass (about
                                     8 Mi camera rays per pass; env RTG_PASS_RAYS) and
                                     add each pixel's samples in sample order, so the image
                                     is the same bit for bit; this flag restores one
                                     sample per pass (for cross-checks)               */
};

typedef struct {
    int32_t camera;               /* index into cameras[] */
    int32_t sample_begin;         /* first sample index (default 0) */
    int32_t sample_count;         /* number of samples, <0 = camera spp */
    int32_t row_begin, row_end;   /* rows to render, row_end<=0 = all; the reference's
                                     row bands (main.cpp:38-39) are one choice */
    int32_t flags;                /* rtg_render_flags */
    uint64_t seed;                /* counter-based RNG key (stochastic features) */
    /* Image partition (ABI 3).  The rows [row_begin, row_end) are cut into bands of
     * RTG_PART_BAND_ROWS rows (counted from row_begin), dealt round-robin with the order
     * rotated by one slot per round (ABI 5): the k-th band of part p of N is band
     * k * N + ((p - k) mod N) -- so every part samples every position within a round of N
     * bands, and a cost peak a few bands tall (a horizon) is shared out.  A render with part_count > 1 computes and writes only the pixels
     * of part part_index; the union of parts 0..part_count-1 is bit-identical to the
     * whole render (pixels are independent, the RNG is keyed by pixel).  Exception: for
     * a camera with a <Tonemap>, a part's LDR rows hold clamp((int)c), not the tonemapped
     * value -- the tonemapper needs the whole frame (tonemapper.h:28-60); a caller that
     * gathers parts itself runs rtg_tonemap on the gathered float image (multigpu.py
     * finish_frame), while rtg_render on a multi-replica scene does it internally.  This
     * is how the frame is dealt to the GPUs of a node (main.cpp:38-39 deals row bands to
     * threads).  part_count <= 0 means 1. */
    int32_t part_index, part_count;
} rtg_render_opts;

/* ABI 5: 8-row bands (16 in ABI 3-4): 1080 rows over 8 parts give 17 or 16 bands per part
 * (a 0.7 % imbalance) instead of 9 or 8 (6.6 %) */
#define RTG_PART_BAND_ROWS 8

/* The rows of part `part_index` of `part_count` within [row_begin, row_end), as maximal
 * runs of consecutive rows: runs[2k] = first row, runs[2k+1] = one past the last.  Writes
 * up to `cap` runs; *count = number of runs.  Pure host arithmetic (no device needed). */
int rtg_part_runs(int32_t row_begin, int32_t row_end, int32_t part_index, int32_t part_count, int32_t* runs,
                  int32_t cap, int32_t* count);

typedef struct {
    uint64_t camera_rays;         /* primary rays (one per pixel-sample)            */
    uint64_t secondary_rays;      /* reflection / refraction extend rays             */
    uint64_t shadow_rays;         /* CastShadowRay queries                           */
    uint64_t node_visits;         /* BVH node box tests, extend rays                 */
    uint64_t tri_tests;           /* Mesh::IntersectFace calls, extend rays          */
    uint64_t sphere_tests;        /* Sphere::Intersect calls (all rays)              */
    uint64_t object_tests;        /* per-object visits (all rays)                    */
    uint64_t shadow_node_visits;  /* BVH node box tests, shadow rays (early exit)    */
    uint64_t shadow_tri_tests;    /* triangle tests, shadow rays (early exit)        */
    uint64_t shadow_wide_visits;  /* any-hit wide BVH nodes visited (shadow rays; each
                                     tests four child boxes; A/B builds only)          */
    uint64_t shadow_fallbacks;    /* shadow rays the fast any-hit walk left undecided,
                                     answered by the reference walk                    */
    uint64_t extend_wide_visits;  /* RTG_RENDER_ORDERED: wide BVH nodes visited by
                                     camera rays (ABI 4)                               */
    uint64_t extend_fallbacks;    /* RTG_RENDER_ORDERED: camera rays whose check failed,
                                     answered by the reference walk (ABI 4)           */
} rtg_stats;

/* One call per camera, replacing main.cpp:164-185 (threads -> renderThreadMain ->
 * RenderPixel).  Host buffers of width*height*3, layout 3*(x + y*width)
 * (main.cpp:109).  hdr_rgb receives the float colour (what main.cpp:114-116
 * stores for tonemapped cameras); ldr_rgb receives clamp((int)c) (main.cpp:121), or,
 * for a camera with a <Tonemap> rendered over all its rows, the tonemapped image
 * main.cpp:187-192 produces (a row band gets the clamp: tonemap the gathered image
 * with rtg_tonemap).  Either may be NULL. */
int rtg_render(rtg_scene* scene, const rtg_render_opts* opts, float* hdr_rgb, uint8_t* ldr_rgb);

/* Same on device-resident buffers (hipMalloc'd / torch tensors) on `stream`
 * (a hipStream_t, NULL = default stream).  Asynchronous: returns after enqueue.
 * d_accum (width*height*4 floats: sum w*r, sum w*g, sum w*b, sum w) is required
 * with RTG_RENDER_ACCUM_ONLY and ignored otherwise. */
int rtg_render_device(rtg_scene* scene, const rtg_render_opts* opts, float* d_hdr_rgb,
                      uint8_t* d_ldr_rgb, float* d_accum, void* stream);

/* Host framebuffer gather for one process per GPU: enqueue on `stream` the copies of the
 * rows of part opts->part_index (opts as given to rtg_render_device) from full-frame device
 * buffers into the same offsets of full-frame host buffers (either pair may be NULL).  With
 * page-locked host memory (rtg_host_alloc / rtg_host_register, e.g. a shared-memory frame
 * mapped by every rank) the copies are asynchronous DMA. */
int rtg_copy_part_to_host(rtg_scene* scene, const rtg_render_opts* opts, const float* d_hdr_rgb,
                          const uint8_t* d_ldr_rgb, float* hdr_rgb, uint8_t* ldr_rgb, void* stream);

/* Page-locked host memory for frame buffers (hipHostMalloc / hipHostRegister). */
int rtg_host_alloc(size_t bytes, void** out);
int rtg_host_free(void* ptr);
int rtg_host_register(void* ptr, size_t bytes);
int rtg_host_unregister(void* ptr);

/* Normalise an accumulation buffer (sum over devices) into hdr/ldr, host side. */
int rtg_resolve_accum(const float* accum, int32_t width, int32_t height, float* hdr_rgb,
                      uint8_t* ldr_rgb);

/* Stats of the last RTG_RENDER_COUNT_STATS render (waits for the scene's last render,
 * not for the device). */
int rtg_scene_stats(rtg_scene* scene, rtg_stats* out);
int rtg_scene_reset_stats(rtg_scene* scene);

/* Kernel durations (ms, HIP events on the render's stream) of the last render issued
 * with RTG_RENDER_TIMING, for its last sample pass; synchronises on that render.
 * Wavefront pipeline: names "k_primary", "k_shade", "k_shadow", "k_resolve"; fused
 * kernel: "k_render"; ray-tree pipeline: "tree_levels" (all levels' trace / shade /
 * shadow kernels), "tree_resolve".  Writes up to `cap` entries; *count = number of stages. */
int rtg_scene_timings(rtg_scene* scene, float* ms, const char** names, int32_t cap, int32_t* count);
/* ABI 6: samples per pixel the stages rtg_scene_timings reports covered -- the last pass's
 * samples (a pass carries several, RTG_RENDER_SAMPLE_PASSES), or the whole render's for the
 * fused kernel. */
int rtg_scene_timed_samples(const rtg_scene* scene, int32_t* samples);

/* ------------------------------------------------------------------------- */
/* Ray queries: closest hit, occlusion, camera-ray batches.  Added symbols    */
/* only -- RTG_ABI_VERSION stays 6 (nothing existing changed layout or        */
/* meaning).                                                                  */
/* ------------------------------------------------------------------------- */
/* 32 B: two 16-byte loads per ray */
typedef struct {
    float ox, oy, oz, tmax;   /* tmax: the walk's initial minT; INFINITY = unbounded */
    float dx, dy, dz, time;   /* time: the reference's motion-blur time in [0,1) */
} rtg_ray;
/* 16 B: one 16-byte store per hit */
typedef struct { float t; int32_t object; int32_t face; int32_t pad; } rtg_hit;
enum rtg_query_flags {
    RTG_QUERY_ANY_HIT = 1,    /* occlusion instead of closest hit */
    RTG_QUERY_COHERENT = 2    /* hint: 64 consecutive rays are similar (e.g. camera rays) */
};

/* Semantics (the reference's own, raytracer.cpp:585-643):
 *  - Closest hit: the result of IntersectObjects with its initial minT set to tmax.  t is the
 *    accepted distance, object the index into objects[], face the global index into faces[] in
 *    BVH order (the order rtg_scene_export_bvh reports; -1 for a sphere).  A miss is
 *    object = face = -1 with t = tmax.  Ties and the strict t < minT are the reference's: among
 *    equal distances the first object, and within a mesh the first face its BVH walk meets, win.
 *    Like the reference's ray, a motion-blurred instance whose world box is missed leaves its
 *    offset on the origin the later objects see.
 *  - RTG_QUERY_ANY_HIT: CastShadowRay's boolean with minT0 = limit = tmax: object is 0 if
 *    occluded and -1 if not; t and face are unspecified.  As in the reference, objects flagged
 *    RTG_OBJF_SHADOW_SKIP (emissive meshes) are skipped and `time` is ignored (shadow rays
 *    carry time 0).
 *  - normals (closest hit only; nullable; 4 floats per ray): the world-space unit normal of the
 *    hit -- the face's or sphere's normal through the object's inverse transpose, as the
 *    reference computes it before any normal or bump map -- with a fourth component of 0; a
 *    miss gives all zeros.  Ignored with RTG_QUERY_ANY_HIT.
 *  - RTG_QUERY_COHERENT is a performance hint only: results are bit-identical with and
 *    without it.
 *  - n == 0 is RTG_OK; n above INT32_MAX or a null buffer is RTG_ERR_INVALID. */

/* Device-resident buffers on `stream`; asynchronous like rtg_render_device, no allocation per
 * call.  A multi-device scene answers on its first replica. */
int rtg_trace_rays_device(rtg_scene* scene, const rtg_ray* d_rays, int64_t n, uint32_t flags, rtg_hit* d_hits,
                          float* d_normals, void* stream);
/* Same on host buffers (synchronous). */
int rtg_trace_rays(rtg_scene* scene, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_hit* hits,
                   float* normals);
/* The rays rtg_render traces for opts->camera: rows [row_begin, row_end) (row_end <= 0: all),
 * sample opts->sample_begin, in pixel order (width * rows rays), each from the RNG key of
 * (opts->seed, pixel, sample) -- GenerateRay's ray, depth-of-field and motion-blur draws
 * included.  tmax is INFINITY and time the motion-blur draw.  The other fields of opts are
 * ignored. */
int rtg_camera_rays_device(rtg_scene* scene, const rtg_render_opts* opts, rtg_ray* d_rays, void* stream);
int rtg_camera_rays(rtg_scene* scene, const rtg_render_opts* opts, rtg_ray* rays);
/* Host only, no device: the reference's object loop restated plainly (recursive BVH descent
 * over the description's own nodes) -- the yardstick of the device queries, bit for bit.
 * RTG_ERR_INVALID for a description without nodes (RTG_LOAD_DEVICE_BVH). */
int rtg_desc_trace_rays(const rtg_scene_desc* desc, const rtg_ray* rays, int64_t n, uint32_t flags,
                        rtg_hit* hits, float* normals);

/* ------------------------------------------------------------------------- */
/* Multi-hit ray queries: the k nearest hits along a ray, in order.  Added    */
/* symbols only -- RTG_ABI_VERSION stays 6.                                   */
/* ------------------------------------------------------------------------- */
#define RTG_MULTIHIT_MAX 8

/* Semantics (IntersectObjects, raytracer.cpp:625-643, keeping k distances instead of one):
 *  - The walk: the ray holds the k smallest accepted distances.  Its minT is the k-th of them, or
 *    tmax while fewer than k are held, and it is used wherever the reference uses minT: box
 *    tests, instance world boxes and group boxes, the moved-origin rule of a missed
 *    motion-blurred instance, and t > 0 && t < minT at faces and spheres.  It never increases.
 *    The boxes, the faces and their order are those of the closest-hit walk.
 *  - Ordering and ties: an accepted hit enters the list in ascending t, after any held hit of
 *    equal t; what falls off the end is dropped.  So among equal distances the first object
 *    takes the earlier slot, and within a mesh the first face its BVH walk meets.
 *  - Output: slot j of ray i is hits[i * k + j].  Filled slots come first and carry t, object,
 *    face and pad = 0 as rtg_trace_rays does; unfilled slots are its miss record (tmax's own
 *    bits, object = face = -1).  counts[i] (nullable) is the number of filled slots.  With k = 1
 *    the result equals rtg_trace_rays without flags byte for byte, tmax <= 0 and NaN included.
 *    (The answer for k is the first k slots of the answer for a larger k except on near ties: a
 *    larger minT culls fewer boxes, and a face whose distance rounds a hair below the entry
 *    distance of a box the shorter list's walk culls is found only by the longer one's.)
 *  - Spheres contribute both roots: first the one Sphere::Intersect selects (sphere.cpp:13-70),
 *    with face = -1, then the other one if it differs, under the same t > 0 && t < minT, with
 *    face = -2.  (For k = 1 the second root can never displace the first.)
 *  - RTG_OBJF_SHADOW_SKIP objects are hit like any other; time is the motion-blur time.
 *  - flags: RTG_QUERY_COHERENT is accepted as a hint that never changes an answer (ignored
 *    today); RTG_QUERY_ANY_HIT or an unknown bit is RTG_ERR_INVALID.  k outside
 *    [1, RTG_MULTIHIT_MAX], n above INT32_MAX, or a null scene, ray or hit buffer is
 *    RTG_ERR_INVALID; n == 0 is RTG_OK.
 *  - Cost: an unbounded ray visits every box it pierces until k hits are held, and only then
 *    culls at the k-th distance.  Give tmax where the caller knows a bound. */

/* Device-resident buffers on `stream` (d_hits: n * k records; d_counts: n, nullable);
 * asynchronous, allocates nothing and touches no render state.  A multi-device scene answers on
 * its first replica.  Works on clones and after rtg_scene_update. */
int rtg_trace_rays_multi_device(rtg_scene* scene, const rtg_ray* d_rays, int64_t n, int32_t k, uint32_t flags,
                                rtg_hit* d_hits, int32_t* d_counts, void* stream);
/* Same on host buffers (synchronous). */
int rtg_trace_rays_multi(rtg_scene* scene, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags,
                         rtg_hit* hits, int32_t* counts);
/* Host only, no device: the same walk restated plainly over the description's own nodes -- the
 * yardstick of the device query, bit for bit.  RTG_ERR_INVALID for a description without nodes
 * (RTG_LOAD_DEVICE_BVH). */
int rtg_desc_trace_rays_multi(const rtg_scene_desc* desc, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags,
                              rtg_hit* hits, int32_t* counts);

/* ------------------------------------------------------------------------- */
/* Closest-point queries: the nearest point of the scene's surface to a       */
/* point, its distance, and the object and face it lies on.  No ray in it:    */
/* the same BVH, pruned by distance to a box.  Added symbols only --          */
/* RTG_ABI_VERSION stays 6.                                                   */
/* ------------------------------------------------------------------------- */
typedef struct { float x, y, z, max_dist; } rtg_point;        /* 16 B; max_dist = INFINITY: unbounded */
typedef struct { float dist; int32_t object, face, pad0;       /* 32 B: two 16-byte stores            */
                 float px, py, pz, pad1; } rtg_nearest;

/* Semantics (the host walk of rtg_desc_closest_points defines them; the device repeats its
 * decisions with the same float arithmetic in the same order, so the two agree bit for bit):
 *  - Result: dist is the world-space distance, object the object index, face the global face
 *    index (-1 for a sphere), (px, py, pz) the world-space closest point; pad0 = pad1 = 0.
 *    Miss -- nothing strictly nearer than |max_dist|, or a coordinate of the point not finite:
 *    dist = max_dist (its own bits), object = face = -1, the point zeros.
 *  - Candidates are compared on the squared distance d2.  A candidate (d2, object, face) replaces
 *    the held one iff d2 < best_d2, or d2 == best_d2 and (object, face) is lexicographically
 *    smaller.  best_d2 starts at max_dist * max_dist with nothing held; while nothing is held only
 *    d2 < best_d2 accepts.  A NaN d2 is never accepted.  dist = sqrtf(best_d2).  Only the square of
 *    max_dist enters: its sign is ignored (-3 admits what 3 admits, and a miss still reports
 *    max_dist's own bits, -3); max_dist = 0 or NaN admits nothing.
 *  - Every object counts, RTG_OBJF_SHADOW_SKIP meshes included.  Motion blur is ignored: objects
 *    stand where they are at time 0.
 *  - Meshes: the point-to-triangle test is the region-based one (Ericson, Real-Time Collision
 *    Detection 5.1.5) on the walk's face record a = v0, ab = -(v0 - v1), ac = -(v0 - v2), the
 *    regions tested in the order A, B, AB, C, AC, BC, interior; the closest point is
 *    a + ab v + ac w.  On well-shaped triangles dist is within a few ulp of the largest coordinate
 *    involved; on slivers the cross terms cancel and the error can be a thousand times that, so
 *    what is promised there is device == host, not a tolerance.  A zero-area face contributes
 *    whatever the region tests give it (possibly nothing: a NaN d2).
 *  - The walk, per mesh object, over the (base) mesh's BVH: first a descent from the root to one
 *    leaf, at each inner node towards the child whose box is nearer (a tie goes left), whose faces
 *    seed the bound; then the pre-order walk, a node skipped iff the squared distance from the
 *    point to its box exceeds best_d2 * lip2.  There is no object-level box test.
 *  - Transforms: an object whose transform is exactly the identity does no transform arithmetic
 *    (lip2 = 1).  Otherwise boxes are tested against the local point inv_transform * p, with
 *    lip2 = sigma_max(inv_transform 3x3)^2 * (1 + 1e-5) (a local displacement is at most sigma_max
 *    times the world one), and every visited face is carried to world space by `transform` and
 *    tested there against the world point: leaves are exact in world space.  Both matrices are
 *    narrowed to float first.
 *  - Spheres: d = |length(p - centre) - radius|, the closest point centre + (p - centre) * (radius /
 *    length), or centre + (radius, 0, 0) at the centre itself.  A sphere under a similarity
 *    (transform^T transform within 1e-6 s^2 of s^2 I, s = cbrt(|det|)) is the sphere of world
 *    centre transform * centre and radius radius * s.  Any other transform makes an ellipsoid, whose
 *    closest point is iterative: such a scene is refused by all three entry points with
 *    RTG_ERR_UNSUPPORTED and a message naming the object; no buffer is touched.
 *  - flags must be 0 (any bit: RTG_ERR_INVALID).  n in [0, INT32_MAX]; n == 0 is RTG_OK and touches
 *    no buffer.  A null scene, or a null buffer with n > 0, is RTG_ERR_INVALID.  The refusal of
 *    an ellipsoid scene comes before the n == 0 rule: such a scene answers RTG_ERR_UNSUPPORTED for
 *    every n, 0 included (the argument errors above come before both).
 *  - Out of scope: the k nearest primitives, ellipsoids, a motion-blur time, a packet walk.  The
 *    sign of the distance is rtg_signed_distance_points' (below). */

/* Device-resident buffers on `stream`; asynchronous, allocates nothing and touches no render
 * state.  A multi-device scene answers on its first replica.  Works on clones and after
 * rtg_scene_update (the placement records are updated with the objects). */
int rtg_closest_points_device(rtg_scene* scene, const rtg_point* d_points, int64_t n, uint32_t flags,
                              rtg_nearest* d_out, void* stream);
/* Same on host buffers (synchronous; the scene's query scratch and its own stream). */
int rtg_closest_points(rtg_scene* scene, const rtg_point* points, int64_t n, uint32_t flags, rtg_nearest* out);
/* Host only, no device: the walk that defines the query -- the yardstick of the device query, bit
 * for bit.  RTG_ERR_INVALID for a description without nodes (RTG_LOAD_DEVICE_BVH). */
int rtg_desc_closest_points(const rtg_scene_desc* desc, const rtg_point* points, int64_t n, uint32_t flags,
                            rtg_nearest* out);

/* ------------------------------------------------------------------------- */
/* Crossing counts and signed distances: how many surfaces a ray meets, with  */
/* no bound on their number, and the closest-point distance signed by the     */
/* parity of that count.  Added symbols and one type only -- RTG_ABI_VERSION  */
/* stays 6.                                                                   */
/* ------------------------------------------------------------------------- */
/* 8 B: one 8-byte store per ray */
typedef struct { int32_t count; int32_t entering; } rtg_crossings;

/* Semantics of a crossing count (no reference code stands behind it: rtg_desc_count_crossings'
 * host walk defines it, the device repeats it bit for bit):
 *  - The walk is rtg_trace_rays_multi's with a minT that is tmax from start to end: the same object
 *    loop, the same group and instance world-box tests, the same moved-origin rule for a
 *    motion-blurred instance whose world box is missed, the same box, face and sphere arithmetic.
 *    Nothing is kept, so nothing is culled: every hit with t > 0 && t < tmax is counted, whatever
 *    their number.  Large leaves are tested face by face like any other.
 *  - count: the number of accepted hits.  A sphere gives both roots; a double root counts once (the
 *    second root counts only if it differs from the first).  Coincident surfaces are all counted.
 *    RTG_OBJF_SHADOW_SKIP objects count.  time is the motion-blur time.  Consequence: wherever
 *    rtg_trace_rays_multi with k = 8 reports counts[i] < 8, count equals it exactly (that walk's minT
 *    never left tmax either); where it reports 8, count >= 8.
 *  - entering: the number of counted hits at which the ray goes against the geometric normal.  At a
 *    face: (dx nx + dy ny) + dz nz < 0 in float, d the ray's direction in the object's local space
 *    (the walk's own ray) and n the face's normal (rtg_face.n, what rtg_trace_rays' `normals` is
 *    built from); the sign is the same in world space, mirrored transforms included.  At a sphere
 *    the root (-b - delta) / a enters and the other leaves (a double root enters).  A counted hit
 *    that is not entering is leaving: count - entering is a winding-style test on consistently
 *    oriented meshes, count & 1 the parity test.
 *  - tmax <= 0, a NaN tmax and non-finite rays give whatever the comparisons give: the promise is
 *    device == host, as for the other queries.
 *  - flags: RTG_QUERY_COHERENT is accepted and ignored.  RTG_QUERY_ANY_HIT or an unknown bit is
 *    RTG_ERR_INVALID.  n == 0 is RTG_OK; n above INT32_MAX or a null scene / buffer is
 *    RTG_ERR_INVALID.
 *  - Cost: an unbounded ray visits every box it pierces and tests every face in them; a caller
 *    who knows a bound should give it as tmax.
 *  - A ray through an edge or a vertex shared by faces may count it once or twice, as the face
 *    test's comparisons fall: the host walk decides, and the device agrees with it. */

/* Device-resident buffers on `stream`: asynchronous, allocates nothing and touches no render
 * state.  A multi-device scene answers on its first replica.  Works on clones and after
 * rtg_scene_update. */
int rtg_count_crossings_device(rtg_scene* scene, const rtg_ray* d_rays, int64_t n, uint32_t flags,
                               rtg_crossings* d_out, void* stream);
/* Same on host buffers (synchronous; the scene's query scratch and its own stream). */
int rtg_count_crossings(rtg_scene* scene, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_crossings* out);
/* Host only, no device: the walk that defines the query.  RTG_ERR_INVALID for a description
 * without nodes (RTG_LOAD_DEVICE_BVH). */
int rtg_desc_count_crossings(const rtg_scene_desc* desc, const rtg_ray* rays, int64_t n, uint32_t flags,
                             rtg_crossings* out);

/* Signed distances: per point the closest-point query, then one crossing walk from the point.
 *  - The closest point: exactly rtg_closest_points' -- same candidates, same tie rule, same miss
 *    record, same ellipsoid refusal.
 *  - The crossing walk above on the ray (origin = the point, direction = dir, tmax = INFINITY,
 *    time = 0).
 *  - The record is rtg_closest_points' with two differences.  pad0 is the crossing count.  On a hit
 *    with an odd count dist has its sign bit set: -sqrtf(best_d2), which is -0.0f on the surface.
 *    On a miss dist stays max_dist's own bits and pad0 still carries the count: a caller baking a
 *    narrow band still learns the side.  A point with a non-finite coordinate gives the
 *    closest-point miss record with pad0 = 0 (no walk is run).
 *  - dir: a host pointer to three floats in all three entry points (the device path hands it to the
 *    kernel by value).  NULL selects (0.8213f, 0.4402f, 0.3628f), which lies in no coordinate or
 *    diagonal plane.  It need not be of unit length: only counts are read.  A non-finite or
 *    all-zero dir is RTG_ERR_INVALID.
 *  - What the sign means: the parity of the surfaces crossed along dir.  That is "inside" for
 *    closed surfaces (inside an odd number of them: the cavity of a hollow shell is outside), and
 *    for an open surface along a direction that leaves through it: on a height field dir =
 *    (0, 0, 1) answers "below the terrain".  A ray through an edge or a vertex may count it once or
 *    twice (the host walk decides); pad0 lets a caller see the count and ask again with another
 *    dir.  For consistently oriented meshes count - entering is available from
 *    rtg_count_crossings.
 *  - flags must be 0.  n and null rules as for rtg_closest_points, the ellipsoid refusal
 *    (RTG_ERR_UNSUPPORTED) before the n == 0 rule and after the argument errors, dir's among them.
 *  - Out of scope: generalised winding numbers, a motion-blur time, a packet walk. */
int rtg_signed_distance_points_device(rtg_scene* scene, const rtg_point* d_points, int64_t n, const float dir[3],
                                      uint32_t flags, rtg_nearest* d_out, void* stream);
int rtg_signed_distance_points(rtg_scene* scene, const rtg_point* points, int64_t n, const float dir[3],
                               uint32_t flags, rtg_nearest* out);
int rtg_desc_signed_distance_points(const rtg_scene_desc* desc, const rtg_point* points, int64_t n,
                                    const float dir[3], uint32_t flags, rtg_nearest* out);

/* ------------------------------------------------------------------------- */
/* Surface queries: what the renderer knows about the point a ray hits --     */
/* shading normal, texture coordinates, material and diffuse coefficient.     */
/* Added symbols and one type only -- RTG_ABI_VERSION stays 6.                */
/* ------------------------------------------------------------------------- */
/* 64 B: four 16-byte stores per ray */
typedef struct {
    float t; int32_t object, face, material;   /* as rtg_hit; material = objects[object].material, -1 on a miss */
    float nx, ny, nz, u;                       /* shading normal (world, unit); texture coordinate u */
    float gx, gy, gz, v;                       /* geometric normal (world, unit); texture coordinate v */
    float kd_r, kd_g, kd_b, pad;               /* diffuse coefficient; pad = 0 */
} rtg_surface;

/* Semantics (PerformShading's view of a primary hit, raytracer.cpp:65-134):
 *  - t, object, face: the closest hit rtg_trace_rays reports for the same ray, bit for bit
 *    (tmax, ties and the moved-origin rule of motion-blurred instances included).
 *  - gx, gy, gz: the `normals` output of rtg_trace_rays, bit for bit: the face's or sphere's
 *    normal through the object's inverse transpose, before any normal or bump map.
 *  - nx, ny, nz: the normal PerformShading receives for a primary ray: a mesh's replace_normal /
 *    bump_normal map or a sphere's bump map (image or Perlin) applied in the object's space, then
 *    the object's inverse transpose.  As in the reference it is not flipped towards the ray.  For
 *    an object without a normal or bump map it equals g bit for bit.
 *  - u, v: the texture coordinates the reference's intersection reports.  Mesh with UVs: the
 *    face's coordinates interpolated with the hit's barycentrics, each through the reference's
 *    tiling rule (a value above 1.0001 keeps its fractional part; a fractional part below 0.0001
 *    becomes 1).  Mesh without UVs: 0.  Sphere: u = (pi - atan2(z, x)) / (2 pi), v = acos(y / r) / pi
 *    of the local hit point relative to the centre.
 *  - kd_r, kd_g, kd_b: the coefficient GetDiffuse hands to Shade (raytracer.cpp:478-508).  Without
 *    a diffuse texture it is the material's DiffuseReflectance, bit for bit.  With one it is the
 *    image sample / 255 (nearest or bilinear) or the Perlin value, replacing the material's value
 *    (replace_kd) or averaged with it (blend_kd).  It is reported for every hit, also for emissive
 *    materials and replace_all objects, whose render never reads it.
 *  - A miss: t = tmax (its bits), object = face = material = -1, every other field +0.0f.
 *  - flags: RTG_QUERY_COHERENT is a performance hint only: results are bit-identical with and
 *    without it.  RTG_QUERY_ANY_HIT or an unknown bit is RTG_ERR_INVALID.
 *  - time is the motion-blur time, as for rtg_trace_rays.
 *  - The arithmetic is the reference's float32, singular points included: u, v of a ray in or
 *    near a face's plane carry the barycentrics' error (about 2^-24 / cos(ray, face normal)), and a
 *    hit on the very pole of a sphere, where rounding puts |y| above r, has acos(y / r) = NaN: v,
 *    and the normal of a bumped sphere, are NaN there, as in the render.
 *  - n == 0 is RTG_OK; n above INT32_MAX or a null scene / buffer is RTG_ERR_INVALID.  Without a
 *    device: RTG_ERR_HIP (no scene can exist). */

/* Device-resident buffers on `stream`: asynchronous, no allocation, and no render state touched.
 * A multi-device scene answers on its first replica. */
int rtg_surface_rays_device(rtg_scene* scene, const rtg_ray* d_rays, int64_t n, uint32_t flags,
                            rtg_surface* d_out, void* stream);
/* Same on host buffers (synchronous; copies through the scene's query scratch). */
int rtg_surface_rays(rtg_scene* scene, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_surface* out);

/* ------------------------------------------------------------------------- */
/* Radiance queries: the colour the renderer computes along caller-supplied   */
/* rays.  Added symbols and types only -- RTG_ABI_VERSION stays 6.            */
/* ------------------------------------------------------------------------- */
enum rtg_radiance_flags {
    RTG_RADIANCE_CAMERA_EYE = 1   /* primary hits are shaded as seen from the camera's position, not
                                     from the ray's origin: the reference's own behaviour for its
                                     depth-of-field rays (raytracer.cpp: PerformShading gets the camera
                                     position, GenerateRay moved the origin onto the lens) */
};
typedef struct {
    int32_t camera;        /* supplies the renderer flags (path tracing, NEE, importance sampling,
                              Russian roulette), width/height for the background-texture lookup, and
                              the eye under RTG_RADIANCE_CAMERA_EYE.  Nothing else of it is used. */
    int32_t sample_begin;  /* first sample index (<0 = 0) */
    int32_t sample_count;  /* samples per ray (<=0 = 1) */
    uint32_t flags;        /* rtg_radiance_flags */
    uint64_t seed;
    int32_t first_pixel;   /* ray i plays pixel first_pixel + i when pixel_ids is NULL */
    int32_t pad0;
} rtg_radiance_opts;

/* Semantics (RenderPixel's, raytracer.cpp:38-63, below a ray of the caller's instead of
 * GenerateRay's):
 *  - Pixel and key: ray i takes the role of pixel p = pixel_ids ? pixel_ids[i] : first_pixel + i.
 *    Sample s of it draws its random numbers from the key of (seed, p, s), the key rtg_render
 *    uses for that pixel and sample; equal (seed, p, s) and equal rays give equal colours.  The
 *    only other use of p is the background texture of a primary ray that misses: it is looked up
 *    at px = p % width, py = p / width of opts->camera's image, as in a render.  A negative p is
 *    RTG_ERR_INVALID where the host can see it (first_pixel, pixel_ids of rtg_radiance_rays);
 *    device-resident ids are the caller's responsibility.
 *  - Primary ray: origin, direction and time are taken as given; time is the motion-blur time,
 *    which the whole ray tree inherits as in a render.  tmax bounds the primary ray only (the
 *    walk's initial minT, as for rtg_trace_rays); a render's is INFINITY, which rtg_camera_rays
 *    writes.  The eye of a primary hit is the ray's origin, or the camera's position under
 *    RTG_RADIANCE_CAMERA_EYE.
 *  - Value: 4 floats per ray.  With one sample, rgb is RenderPixel's colour for the ray -- the
 *    whole ray tree, every light, textures, the miss colour -- unclamped: what rtg_render stores in
 *    hdr_rgb for a camera of one sample, bit for bit, when the rays are rtg_camera_rays' of the
 *    same seed and RTG_RADIANCE_CAMERA_EYE is set.  With sample_count = k > 1,
 *    rgb = (((0 + c_0) + c_1) + ... + c_{k-1}) / (float)k per component, in float, in ascending
 *    sample order, c_j being the colour of sample sample_begin + j.  The Gaussian pixel-filter
 *    weights belong to rtg_render's pixel loop and are not applied.  The fourth float is the
 *    primary hit's t (the same for every sample); tmax on a miss.
 *  - n == 0 is RTG_OK.  n above INT32_MAX, a null scene / opts / ray / output buffer, an unknown
 *    flag bit or a bad camera index is RTG_ERR_INVALID.  Without a device: RTG_ERR_HIP.
 *  - Always the fused kernel's walk (the pipelines rtg_render may choose give the same image). */

/* Device-resident buffers on `stream`: asynchronous, no allocation, and no render state touched
 * (work buffers, plans, events, counters, timings).  d_pixel_ids nullable.  A multi-device scene
 * answers on its first replica. */
int rtg_radiance_rays_device(rtg_scene* scene, const rtg_radiance_opts* opts, const rtg_ray* d_rays,
                             const int32_t* d_pixel_ids, int64_t n, float* d_rgbt, void* stream);
/* Same on host buffers (synchronous; copies through the scene's query scratch). */
int rtg_radiance_rays(rtg_scene* scene, const rtg_radiance_opts* opts, const rtg_ray* rays,
                      const int32_t* pixel_ids, int64_t n, float* rgbt);

/* ------------------------------------------------------------------------- */
/* Scene updates: cameras, lights, materials and object transforms of a live  */
/* scene replaced in place, over geometry that stays as uploaded.  Added      */
/* symbols and one type only -- RTG_ABI_VERSION stays 6.                      */
/* ------------------------------------------------------------------------- */
/* Replaces every non-geometric part of `scene` by `desc`'s: the cameras (their count may change);
 * background, bg_texture, shadow_epsilon, max_recursion_depth, ambient_light; materials, BRDFs and
 * texture records; all six light arrays (their counts may change); and per object the transforms,
 * boxes, flags, material, texture slots, motion-blur vector, sphere centre and radius, and id.
 *
 * Guarantee: afterwards rtg_render*, rtg_trace_rays*, rtg_camera_rays*, rtg_surface_rays* and
 * rtg_radiance_rays* behave bit for bit as on a scene freshly created from `desc` (with the
 * environment knobs the scene was created under).  No BVH is walked or built, no any-hit tree
 * rebuilt, no texel uploaded: the device side is a handful of small copies into existing tables.
 *
 * Same-geometry contract, checked before anything is changed; a mismatch is RTG_ERR_INVALID and
 * leaves the scene untouched.  Against the description the scene was created from:
 *  - num_meshes, num_faces, num_nodes, num_objects equal; per mesh face_offset, face_count,
 *    node_offset, node_count, has_uv equal; per object kind and mesh equal;
 *  - num_images equal, and per image width, height, channels, is_hdr;
 *  - num_mesh_lights equal, and each mesh_lights[i].object.
 * desc->faces, desc->nodes and images[].texels are never read (they may be NULL): face data, BVH,
 * any-hit trees, the mesh lights' faces and the texel pool stay as uploaded, and the caller
 * promises they still match.  Vertex edits need a new scene.
 *
 * Refused with RTG_ERR_UNSUPPORTED, scene untouched:
 *  - `desc` needs a table the scene was created without: the faces' raw vertices exist only if
 *    some object had a normal or bump map in effect at creation, so a map newly attached in a
 *    scene that had none is refused;
 *  - the scene's any-hit trees were built in the split mode (RTG_AHB=split): their padding
 *    depends on the transforms and lights;
 *  - max_recursion_depth above the kernels' bound.
 * The other checks of rtg_scene_create that do not concern geometry apply with their codes; a null
 * argument is RTG_ERR_INVALID.
 *
 * Ordering: the copies are enqueued on `stream` (a hipStream_t, NULL = default stream), like
 * rtg_render_device's work.  Work enqueued on that stream before the call sees the old tables,
 * work enqueued after it the new ones; the scene's own stream (rtg_render and the host-buffer
 * queries) waits for the copies too.  Work of this scene in flight on any other stream during the
 * call races with it: that is the caller's to order.  Host-side state (cameras, counts, pipeline
 * choice) switches at the call.  A table that outgrows its capacity (more lights, materials or
 * textures than ever before) is reallocated, which waits for the device.  On a multi-device scene
 * every replica is updated synchronously and a non-NULL `stream` is RTG_ERR_INVALID.  A HIP error
 * part-way (RTG_ERR_HIP / RTG_ERR_NOMEM) leaves the scene unusable. */
int rtg_scene_update(rtg_scene* scene, const rtg_scene_desc* desc, void* stream);

/* Cameras without a description.  rtg_scene_set_camera replaces camera `index`, or appends with
 * index == the count; it touches no device memory (cameras travel to the kernels by value) and
 * sets every replica of a multi-device scene.  A camera with a non-positive size is accepted: the
 * queries take it, the renders refuse it. */
int rtg_scene_set_camera(rtg_scene* scene, int32_t index, const rtg_camera* cam);
int rtg_scene_num_cameras(const rtg_scene* scene, int32_t* count);
typedef struct {
    rtg_float3 position, gaze, up;     /* gaze: direction, or the gaze point with look_at */
    int32_t look_at;
    float near_plane[4];               /* left right bottom top; ignored with look_at */
    float fov_y;                       /* degrees; look_at only */
    float near_dist;
    int32_t width, height;
} rtg_camera_view;
/* Host only: Camera::SetupDefault / SetupLookAt (camera.cpp:5-72) -- the loader's own arithmetic,
 * so a camera set up here from a <Camera>'s numbers equals the loaded one bit for bit.  Fills
 * position, gaze, up, right, q, left, right_ext, bottom, top, near_dist, width and height of *cam
 * and leaves its other fields (samples, lens, tonemapper, renderer flags, name) as they are. */
int rtg_camera_setup(const rtg_camera_view* view, rtg_camera* cam);

/* A second scene on the same device over the source's geometry: the clone shares the immutable
 * buffers (BVH, faces, any-hit trees, mesh-light faces, texel pool and image records, noise
 * tables) by reference count and owns everything rtg_scene_update may write (objects, materials,
 * textures, lights, cameras) as well as its stream, work buffers, plans, counters and scratch.
 * One clone per frame in flight, each updated to its own state, animates over one copy of the
 * geometry.  Either scene may be destroyed first.  A multi-device source is RTG_ERR_INVALID. */
int rtg_scene_clone(const rtg_scene* scene, rtg_scene** out);
int rtg_scene_shares_geometry(const rtg_scene* a, const rtg_scene* b, int32_t* yes);

/* ------------------------------------------------------------------------- */
/* Tonemapping (tonemapper.h, main.cpp:187-192)                               */
/* ------------------------------------------------------------------------- */
/* Tonemapper(opType, keyValue, burnPerct, saturation, gamma) (tonemapper.h:18-25);
 * the parser's defaults are 0.18, 1, 1, 2.2 (parser.cpp:845-863). */
typedef struct { float key, burn_percent, saturation, gamma; } rtg_tonemap_params;

/* Replaces Camera::GetTonemappedImage -> Tonemapper::Tonemap (tonemapper.h:28-60):
 * photographic operator over a whole width*height float RGB image in device memory,
 * writing the 8-bit image main.cpp:195 saves.  Asynchronous on `stream`. */
int rtg_tonemap_device(const float* d_hdr_rgb, int32_t width, int32_t height, const rtg_tonemap_params* params,
                       uint8_t* d_ldr_rgb, int32_t device, void* stream);
/* Same on host buffers (copies through device `device`; synchronous). */
int rtg_tonemap(const float* hdr_rgb, int32_t width, int32_t height, const rtg_tonemap_params* params,
                uint8_t* ldr_rgb, int32_t device);
/* Tonemapper::avgLuminance (tonemapper.h:35-48): exp(sum of log(0.01f + Y) / pixelCount) with
 * the sum taken as the reference takes it, sequentially in pixel order, on host buffers
 * (synchronous).  mode: -1 the library default (3), 3 windowed exact sum with the windows
 * summarised in parallel beforehand (ABI 5), 2 windowed exact sum, 1 plain sequential chain
 * (modes 1-3 give the same bits), 0 parallel fixed-order reduction (last bits differ from
 * the reference's). */
int rtg_tonemap_log_average(const float* hdr_rgb, int32_t width, int32_t height, int32_t mode, double* avg_out,
                            int32_t device);

/* ------------------------------------------------------------------------- */
/* Output (main.cpp:187-195)                                                  */
/* ------------------------------------------------------------------------- */
/* stbi_write_png replacement: 8-bit RGB, zlib-compressed PNG. */
int rtg_write_png(const char* path, int32_t width, int32_t height, const uint8_t* rgb);
/* stbi_write_hdr replacement: Radiance RGBE. */
int rtg_write_hdr(const char* path, int32_t width, int32_t height, const float* rgb);

const char* rtg_last_error(void);
int rtg_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RTGPU_H */
