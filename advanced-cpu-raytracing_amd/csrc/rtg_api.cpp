// C-ABI implementation (include/rtgpu.h): scene ingest, device upload, render.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>
#include <tuple>
#include <cstdlib>

#include "host_assets.hpp"
#include "host_query.hpp"
#include "host_scene.hpp"
#include "rtg_device.hpp"
#include "rtg_devmem.hpp"
#include "rtg_kernels.hpp"
#include "rtgpu.h"
#include "scene_tables.hpp"
#include "work_layout.hpp"

namespace {

thread_local std::string g_err;

int set_err(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return set_err(RTG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

}  // namespace

using rtg::DevBuf;

// Wavefront work buffers of a scene (rtg_scene::work), each one allocation carved by
// work_layout.hpp for the shape beside it.
struct WaveWork {
    DevBuf<char> mem;                 // ensure_wave
    rtg::WaveShape shape;
    DevBuf<char> dq;                  // deferred-leaf queue + per-pixel hit keys (ensure_defer)
    rtg::DeferShape dq_shape;         // (its pixel count decides its layout)
    rtg::WaveBufs W{};
};
struct TileMap {
    int tx, ty;
    DevBuf<int> map;
};

// What rtg_scene_update never writes: the geometry and everything derived from it alone.  One
// copy per created scene, shared with its clones (rtg_scene_clone) by reference count; freed on
// the device of the scene that drops the last reference (all of them are on the same one).
struct SceneGeom {
    DevBuf<float4> nodes, tris, face_n;
    int node_count = 0;               // nodes in use (device-built BVH: <= nodes.n / 2)
    DevBuf<int2> node_ext;
    DevBuf<float2> face_uv;
    DevBuf<float4> face_v12;
    DevBuf<rtg::DevLightFace> light_faces;
    DevBuf<rtg::DevImage> images;
    DevBuf<float> texels;
    DevBuf<rtg::WNode> anodes;
    DevBuf<float4> ahtris;
    DevBuf<int> face_leaf;
    DevBuf<int> perm;
    DevBuf<float> grad;
};

// The host-buffer queries' scratch (rtg_scene::q): one slot per kind of buffer
enum QuerySlot { Q_RAYS, Q_HITS, Q_NORMALS, Q_RADIANCE, Q_PIXEL_IDS, Q_SURFACE, Q_COUNTS, Q_POINTS, Q_NEAREST, Q_SLOTS };

struct rtg_scene {
    int device = 0;
    rtg::DevScene ds;
    std::vector<rtg_camera> cameras;
    int max_depth = 0;
    std::shared_ptr<SceneGeom> geom;
    // env_direction's hashes depend on the light's index alone: shared until an update needs more
    std::shared_ptr<DevBuf<unsigned long long>> env_mix;
    // the mutable tables (rtg_scene_update copies into them in place)
    DevBuf<int> env_images;
    DevBuf<rtg::DevMeshLight> mesh_lights;
    DevBuf<rtg::DevObject> objects;
    DevBuf<float4> group_box;
    DevBuf<rtg::PointXf> point_xf;    // closest-point queries: per object (a kernel argument of its own, not in DevScene)
    DevBuf<rtg::DevMaterial> materials;
    DevBuf<rtg::DevBrdf> brdfs;
    DevBuf<rtg::DevTexture> textures;
    DevBuf<rtg::DevPointLight> point_lights;
    DevBuf<rtg::DevAreaLight> area_lights;
    DevBuf<rtg::DevDirLight> dir_lights;
    DevBuf<rtg::DevSpotLight> spot_lights;
    DevBuf<rtg::DevCounters> counters;
    DevBuf<int> guard;                // RTG_GUARD builds: index-violation bits
    // rtg_scene_update: the options and kept state of the creation; the host copies of the
    // mutable tables in effect (the sources of the update's asynchronous copies, and of a
    // clone's uploads), and the event after those copies -- waited for before `staged` is
    // overwritten or freed
    rtg::TableOptions opt;
    rtg::KeptTables kept;
    rtg::SceneTables staged;
    hipEvent_t updated = nullptr;
    bool wave_ok = false;             // scene renders on the wavefront pipeline
    bool tree_ok = false;             // scene may render on the wavefront ray-tree pipeline
    rtg::TreeState* tree = nullptr;   // its buffers
    bool path_ok = false;             // path-tracing cameras may render on the wavefront path tracer
    rtg::PathState* path = nullptr;   // its buffers
    int feat = rtg::FEAT_ALL;         // scene feature bits (traversal specialisation)
    int closest_feat = rtg::FEAT_ALL; // ... of k_closest: FEAT_XFORM too where a mesh record lacks PXF_IDENTITY
    int closest_bad = -1;             // first sphere that is an ellipsoid (closest-point queries refuse the scene)
    int num_slots = 0;                // lights per pixel (wavefront light slots)
    int shade_sk = rtg::SK_ALL;       // shading features (k_shade variant, rtg_device.hpp SK_*)
    // wavefront buffers, grown on demand
    WaveWork work;
    // scratch for the host-buffer entry point (both of the same pixel count)
    DevBuf<float> d_hdr;
    DevBuf<unsigned char> d_ldr;
    // scratch of the host-buffer ray queries (rtg_trace_rays, rtg_camera_rays, rtg_radiance_rays,
    // rtg_surface_rays): rays, hits, normals, radiance output, pixel ids, surface output; grown on
    // demand, never touched by the device-buffer entry points
    DevBuf<char> q[Q_SLOTS];          // by QuerySlot, in bytes
    // block -> tile tables, one per (tiles_x, tiles_y) met (never re-uploaded: kernels of
    // several streams may be reading them)
    std::vector<std::unique_ptr<TileMap>> tile_maps;
    // RTG_RENDER_TIMING events (stage k runs between ev[k] and ev[k+1])
    hipEvent_t ev[rtg::MAX_STAGES + 1] = {};
    int timed_layout = -1;            // stage layout of the last timed render (rtg_kernels.hpp LAYOUT_*)
    int timed_samples = 1;            // samples per pixel its timed stages covered (rtg_scene_timed_samples)
    // the scene's own stream (rtg_render) and the event marking the end of its last render
    // on whatever stream it was issued (rtg_scene_stats waits for it, not for the device)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    // rtg_scene_create_multi: the other replicas (replica i renders part i of 1 + size())
    std::vector<rtg_scene*> replicas;
    ~rtg_scene() {
        for (rtg_scene* r : replicas) delete r;
        (void)hipSetDevice(device);
        if (updated) {                // an update's copies may still be reading `staged`
            (void)hipEventSynchronize(updated);
            (void)hipEventDestroy(updated);
        }
        if (guard.p) {
            int bits = 0;
            if (hipMemcpy(&bits, guard.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && bits)
                std::fprintf(stderr, "rtgpu guard: index violations, bits 0x%x\n", bits);
        }
        if (tree) rtg::tree_destroy(tree);
        if (path) rtg::path_destroy(path);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        // (the members' device memory is freed after this body, on the device set above)
    }
};

extern "C" {

const char* rtg_last_error(void) { return g_err.c_str(); }
int rtg_abi_version(void) { return RTG_ABI_VERSION; }

// Build provenance (not part of the ABI): the SHA-256 prefix of the sources this library was
// compiled from (csrc/*, include/rtgpu.h, the Makefile's recipe), so that smoke() can show the
// prebuilt library that travels to the GPU box is the build of the tree it runs beside.
#ifndef RTG_SRC_HASH
#define RTG_SRC_HASH "unknown"
#endif
extern "C" __attribute__((visibility("default"))) const char rtg_source_hash[] = RTG_SRC_HASH;

int rtg_host_scene_load_xml(const char* xml_path, rtg_host_scene** out) {
    return rtg_host_scene_load_xml_ex(xml_path, 0, out);
}

int rtg_host_scene_load_xml_ex(const char* xml_path, uint32_t flags, rtg_host_scene** out) {
    if (!xml_path || !out) return set_err(RTG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)RTG_LOAD_DEVICE_BVH) return set_err(RTG_ERR_INVALID, "unknown load flags 0x%x", flags);
    std::unique_ptr<rtg_host_scene> hs(new (std::nothrow) rtg_host_scene);
    if (!hs) return set_err(RTG_ERR_NOMEM, "out of memory");
    std::string err;
    hs->s.deferBvh = (flags & RTG_LOAD_DEVICE_BVH) != 0;
    int rc = hs->s.load(xml_path, err);
    if (rc != RTG_OK) return set_err(rc, "%s: %s", xml_path, err.c_str());
    *out = hs.release();
    return RTG_OK;
}

const rtg_scene_desc* rtg_host_scene_desc(const rtg_host_scene* hs) { return hs ? &hs->s.desc : nullptr; }
void rtg_host_scene_free(rtg_host_scene* hs) { delete hs; }

int rtg_desc_camera_info(const rtg_scene_desc* d, int camera, int32_t* width, int32_t* height, int32_t* spp,
                         int32_t* has_tonemapper) {
    if (!d || camera < 0 || camera >= d->num_cameras) return set_err(RTG_ERR_INVALID, "bad camera index %d", camera);
    const rtg_camera& c = d->cameras[camera];
    if (width) *width = c.width;
    if (height) *height = c.height;
    if (spp) *spp = c.spp;
    if (has_tonemapper) *has_tonemapper = c.has_tonemapper;
    return RTG_OK;
}

int rtg_desc_counts(const rtg_scene_desc* d, int64_t* num_objects, int64_t* num_faces, int64_t* num_nodes,
                    int64_t* num_lights) {
    if (!d) return set_err(RTG_ERR_INVALID, "null desc");
    if (num_objects) *num_objects = d->num_objects;
    if (num_faces) *num_faces = d->num_faces;
    if (num_nodes) *num_nodes = d->num_nodes;
    if (num_lights)
        *num_lights = (int64_t)d->num_point_lights + d->num_area_lights + d->num_dir_lights + d->num_spot_lights +
                      d->num_env_lights + d->num_mesh_lights;
    return RTG_OK;
}

int rtg_scene_export_bvh(const rtg_scene* s, float* nodes, int64_t max_nodes, float* tris, int64_t max_faces,
                         int64_t* num_nodes, int64_t* num_faces) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    const SceneGeom& g = *s->geom;
    const int64_t nn = g.node_count, nf = (int64_t)(g.tris.n / 3);
    if (num_nodes) *num_nodes = nn;
    if (num_faces) *num_faces = nf;
    HIP_TRY(hipSetDevice(s->device));
    if (nodes && max_nodes >= nn) HIP_TRY(hipMemcpy(nodes, g.nodes.p, nn * 2 * sizeof(float4), hipMemcpyDeviceToHost));
    if (tris && max_faces >= nf) HIP_TRY(hipMemcpy(tris, g.tris.p, nf * 3 * sizeof(float4), hipMemcpyDeviceToHost));
    return RTG_OK;
}

int rtg_device_count(int32_t* count) {
    if (!count) return set_err(RTG_ERR_INVALID, "null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = e == hipSuccess ? n : 0;
    return RTG_OK;
}

// Device ingest: every mesh's BVH and face order built on the GPU (rtg_bvh.hip) straight
// into the scene's walk buffers; rb receives the node ranges and the final face order (mesh
// lights sample it) and, with `records`, host copies of the walk records (the any-hit trees
// are built from them).
static int build_bvh_on_device(SceneGeom* sc, const rtg_scene_desc* d, bool records, rtg::BvhReadback& rb) {
    const int64_t F = d->num_faces;
    const bool anyUV = rtg::any_uv(d), anyMapped = rtg::any_mapped(d);
    const size_t maxNodes = (size_t)2 * F + 1;          // <= 2n - 1 per mesh, + the pad node
    HIP_TRY(sc->nodes.alloc(2 * maxNodes));
    HIP_TRY(sc->node_ext.alloc(maxNodes));
    HIP_TRY(sc->tris.alloc(3 * F));
    HIP_TRY(sc->face_n.alloc(F));
    if (anyUV) HIP_TRY(sc->face_uv.alloc(3 * F));
    if (anyMapped) HIP_TRY(sc->face_v12.alloc(2 * F));
    HIP_TRY(hipMemset(sc->nodes.p, 0, sc->nodes.n * sizeof(float4)));
    DevBuf<rtg_face> faces;
    DevBuf<int> perm;
    HIP_TRY(faces.alloc(F));
    HIP_TRY(hipMemcpy(faces.p, d->faces, F * sizeof(rtg_face), hipMemcpyHostToDevice));
    HIP_TRY(perm.alloc(F));
    hipStream_t st = nullptr;
    int nodeBase = 0;
    rb.mesh_begin.resize(d->num_meshes);
    rb.mesh_end.resize(d->num_meshes);
    for (int m = 0; m < d->num_meshes; ++m) {
        const rtg_mesh& M = d->meshes[m];
        if (M.face_count <= 0 || M.face_offset < 0 || M.face_offset + (int64_t)M.face_count > F)
            return set_err(RTG_ERR_INVALID, "mesh %d: bad face range", m);
        // root box: the mesh's bbox (parser.cpp:1393-1468), carried by its Mesh object
        const rtg_object* owner = nullptr;
        for (int i = 0; i < d->num_objects && !owner; ++i)
            if (d->objects[i].kind == RTG_OBJ_MESH && d->objects[i].mesh == m) owner = &d->objects[i];
        if (!owner) return set_err(RTG_ERR_INVALID, "mesh %d: no Mesh object carries its bbox", m);
        int count = 0;
        bool bl = false;
        HIP_TRY(rtg::build_mesh_bvh(faces.p + M.face_offset, M.face_count, owner->bbox_min, owner->bbox_max,
                                    M.face_offset, nodeBase, sc->nodes.p, sc->node_ext.p, sc->tris.p, sc->face_n.p,
                                    anyUV ? sc->face_uv.p : nullptr, anyMapped ? sc->face_v12.p : nullptr,
                                    perm.p + M.face_offset, &count, &bl, st));
        rb.mesh_begin[m] = nodeBase;
        rb.mesh_end[m] = nodeBase + count;
        nodeBase += count;
        rb.bigleaf |= bl;
    }
    rb.node_count = nodeBase + 1;                       // + the zeroed pad node
    rb.perm.resize(F);
    HIP_TRY(hipMemcpy(rb.perm.data(), perm.p, F * sizeof(int), hipMemcpyDeviceToHost));
    for (int m = 0; m < d->num_meshes; ++m)
        for (int k = 0; k < d->meshes[m].face_count; ++k) rb.perm[d->meshes[m].face_offset + k] += d->meshes[m].face_offset;
    if (records) {
        rb.nodes.resize(2 * (size_t)rb.node_count);
        HIP_TRY(hipMemcpy(rb.nodes.data(), sc->nodes.p, rb.nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
        rb.ext.resize((size_t)rb.node_count);
        HIP_TRY(hipMemcpy(rb.ext.data(), sc->node_ext.p, rb.ext.size() * sizeof(int2), hipMemcpyDeviceToHost));
        rb.tris.resize(3 * (size_t)F);
        HIP_TRY(hipMemcpy(rb.tris.data(), sc->tris.p, rb.tris.size() * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return RTG_OK;
}

// The knobs of the table build: RTG_NO_FAST_SHADOW=1 (shadow rays walk the reference BVH
// top-down), RTG_AHB=ref|split (rtg_ahb.hpp), RTG_NO_COOP=1 (large leaves tested by their own
// lane), RTG_AHB_VERBOSE=1.
static rtg::TableOptions table_options() {
    rtg::TableOptions opt;
    opt.fast_shadow = !std::getenv("RTG_NO_FAST_SHADOW");
    const char* am = std::getenv("RTG_AHB");
    opt.ahb_mode = !am ? rtg::AHB_EXACT : (std::strcmp(am, "ref") == 0 ? rtg::AHB_REF
                                           : std::strcmp(am, "split") == 0 ? rtg::AHB_SPLIT : rtg::AHB_EXACT);
    opt.coop = !std::getenv("RTG_NO_COOP");
    opt.verbose = std::getenv("RTG_AHB_VERBOSE") != nullptr;
    return opt;
}

// The tables rtg_scene_update may write, uploaded afresh (creation, clone).
static int upload_mutable(rtg_scene* sc, const rtg::SceneTables& T) {
    HIP_TRY(sc->objects.upload(T.objects)); HIP_TRY(sc->group_box.upload(T.group_box));
    HIP_TRY(sc->point_xf.upload(T.point_xf));
    HIP_TRY(sc->materials.upload(T.materials)); HIP_TRY(sc->brdfs.upload(T.brdfs));
    HIP_TRY(sc->textures.upload(T.textures));
    HIP_TRY(sc->point_lights.upload(T.point_lights)); HIP_TRY(sc->area_lights.upload(T.area_lights));
    HIP_TRY(sc->dir_lights.upload(T.dir_lights)); HIP_TRY(sc->spot_lights.upload(T.spot_lights));
    HIP_TRY(sc->env_images.upload(T.env_images));
    HIP_TRY(sc->mesh_lights.upload(T.mesh_lights));
    // what every scene owns besides: counters, guard, its stream and its events
    HIP_TRY(sc->counters.alloc(1));
    HIP_TRY(hipMemset(sc->counters.p, 0, sizeof(rtg::DevCounters)));
    HIP_TRY(sc->guard.alloc(1));
    HIP_TRY(hipMemset(sc->guard.p, 0, sizeof(int)));
    HIP_TRY(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&sc->done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&sc->updated, hipEventDisableTiming));
    return RTG_OK;
}

// The scene's host-side state for description `d` with tables T (built or updated): the pipeline
// scalars, the cameras and the DevScene pointing at the scene's device tables as they are now.
static void scene_state(rtg_scene* sc, const rtg_scene_desc* d, const rtg::SceneTables& T) {
    sc->feat = T.feat;
    sc->shade_sk = T.shade_sk;
    sc->num_slots = T.num_slots;
    sc->wave_ok = T.wave_ok;
    sc->tree_ok = T.tree_ok;
    sc->path_ok = T.path_ok;
    sc->max_depth = d->max_recursion_depth;
    sc->cameras.assign(d->cameras, d->cameras + d->num_cameras);
    // k_closest's identity variants do no transform arithmetic: they are for scenes whose mesh
    // records all carry PXF_IDENTITY (rtg_pointxf.hpp judges `transform`, feat `inv_transform`)
    sc->closest_feat = T.feat;
    sc->closest_bad = -1;
    for (size_t i = 0; i < T.point_xf.size(); ++i) {
        const int f = T.point_xf[i].flags;
        if (d->objects[i].kind != RTG_OBJ_SPHERE && !(f & rtg::PXF_IDENTITY)) sc->closest_feat |= rtg::FEAT_XFORM;
        if (!(f & rtg::PXF_SPHERE_OK) && sc->closest_bad < 0) sc->closest_bad = (int)i;
    }
    const SceneGeom& g = *sc->geom;
    rtg::DevScene& S = sc->ds;
    std::memset(&S, 0, sizeof(S));
    S.nodes = g.nodes.p; S.node_ext = g.node_ext.p; S.tris = g.tris.p; S.face_n = g.face_n.p;
    S.face_uv = g.face_uv.p;
    S.face_v12 = g.face_v12.p;
    S.mesh_lights = sc->mesh_lights.ptr();
    S.light_faces = g.light_faces.p;
    S.num_mesh = d->num_mesh_lights;
    // (ptr(): null for an empty table, whether it never had entries or an update emptied it)
    S.objects = sc->objects.ptr(); S.group_box = sc->group_box.ptr(); S.materials = sc->materials.ptr();
    S.brdfs = sc->brdfs.ptr();
    S.textures = sc->textures.ptr(); S.images = g.images.p; S.texels = g.texels.p;
    S.point_lights = sc->point_lights.ptr(); S.area_lights = sc->area_lights.ptr(); S.dir_lights = sc->dir_lights.ptr();
    S.spot_lights = sc->spot_lights.ptr(); S.env_images = sc->env_images.ptr();
    S.env_mix = d->num_env_lights > 0 ? sc->env_mix->p : nullptr;
    S.perm = g.perm.p; S.grad = g.grad.p;
    S.num_objects = d->num_objects; S.num_point = d->num_point_lights; S.num_area = d->num_area_lights;
    S.num_dir = d->num_dir_lights; S.num_spot = d->num_spot_lights; S.num_env = d->num_env_lights;
    S.max_depth = d->max_recursion_depth;
    S.bg_texture = d->bg_texture;
    S.eps = d->shadow_epsilon;
    S.ambient[0] = d->ambient_light.x; S.ambient[1] = d->ambient_light.y; S.ambient[2] = d->ambient_light.z;
    for (int k = 0; k < 3; ++k) S.background[k] = d->background[k];
    S.coop = (sc->feat & rtg::FEAT_BIGLEAF) ? 1 : 0;
    S.anodes = g.anodes.p;              // null without trees: DevBuf::upload of an empty table
    S.ahtris = g.ahtris.p;
    S.ahb_split = T.ahb_split;
    S.face_leaf = g.face_leaf.p;
    S.guard = sc->guard.p;
    S.num_faces = (int)d->num_faces;
    S.num_textures = d->num_textures;
    S.num_images = d->num_images;
    S.num_materials = d->num_materials;
}

// The tables to the device and the DevScene that points at them (the walk and face tables of
// a device-built BVH are there already).
static int upload_tables(rtg_scene* sc, const rtg_scene_desc* d, const rtg::SceneTables& T, bool deviceBvh) {
    SceneGeom& g = *sc->geom;
    g.node_count = T.node_count;
    if (!deviceBvh) {
        HIP_TRY(g.nodes.upload(T.nodes)); HIP_TRY(g.node_ext.upload(T.node_ext)); HIP_TRY(g.tris.upload(T.tris));
        HIP_TRY(g.face_n.upload(T.face_n)); HIP_TRY(g.face_uv.upload(T.face_uv)); HIP_TRY(g.face_v12.upload(T.face_v12));
    }
    HIP_TRY(g.images.upload(T.images)); HIP_TRY(g.texels.upload(T.texels));
    HIP_TRY(g.light_faces.upload(T.light_faces));
    HIP_TRY(g.anodes.upload(T.anodes)); HIP_TRY(g.ahtris.upload(T.ahtris)); HIP_TRY(g.face_leaf.upload(T.face_leaf));
    HIP_TRY(g.perm.upload(T.perm)); HIP_TRY(g.grad.upload(T.grad));
    sc->env_mix = std::make_shared<DevBuf<unsigned long long>>();
    HIP_TRY(sc->env_mix->upload(T.env_mix));
    int rc = upload_mutable(sc, T);
    if (rc) return rc;
    scene_state(sc, d, T);
    HIP_TRY(hipDeviceSynchronize());
    return RTG_OK;
}

// Validate, find the device, build the BVH there when the description carries none (device
// ingest, RTG_LOAD_DEVICE_BVH; otherwise the host-built reference topology is re-laid), build the
// tables on the host (scene_tables.cpp), upload them.
int rtg_scene_create(const rtg_scene_desc* d, int device, rtg_scene** out) {
    if (!d || !out) return set_err(RTG_ERR_INVALID, "null argument");
    *out = nullptr;
    std::string err;
    int rc = rtg::validate_desc(d, err);
    if (rc) return set_err(rc, "%s", err.c_str());

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_err(RTG_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return set_err(RTG_ERR_INVALID, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rtg_scene> sc(new (std::nothrow) rtg_scene);
    if (!sc) return set_err(RTG_ERR_NOMEM, "out of memory");
    sc->device = device;
    sc->geom = std::make_shared<SceneGeom>();

    const rtg::TableOptions opt = table_options();
    const bool deviceBvh = d->num_faces > 0 && d->num_nodes == 0;
    rtg::BvhReadback rb;
    if (deviceBvh && (rc = build_bvh_on_device(sc->geom.get(), d, opt.fast_shadow, rb))) return rc;

    rtg::SceneTables T;
    rc = rtg::build_scene_tables(d, opt, deviceBvh ? &rb : nullptr, T, err);
    if (rc) return set_err(rc, "%s", err.c_str());

    if ((rc = upload_tables(sc.get(), d, T, deviceBvh))) return rc;
    // for rtg_scene_update / rtg_scene_clone: the options, the kept state and the host copies of
    // the mutable tables (the geometry's, by far the larger part, are dropped)
    sc->opt = opt;
    rtg::keep_tables(d, T, sc->kept);
    for (auto* v : {&T.nodes, &T.tris, &T.face_n, &T.face_v12, &T.ahtris}) std::vector<float4>().swap(*v);
    std::vector<int2>().swap(T.node_ext);
    std::vector<float2>().swap(T.face_uv);
    std::vector<float>().swap(T.texels);
    std::vector<rtg::DevLightFace>().swap(T.light_faces);
    std::vector<rtg::WNode>().swap(T.anodes);
    std::vector<int>().swap(T.face_leaf);
    sc->staged = std::move(T);
    *out = sc.release();
    return RTG_OK;
}

// ---- scene updates (rtgpu.h: rtg_scene_update, rtg_scene_set_camera, rtg_scene_clone)
int rtg_scene_update(rtg_scene* s, const rtg_scene_desc* d, void* stream) {
    if (!s || !d) return set_err(RTG_ERR_INVALID, "null argument");
    std::vector<rtg_scene*> reps(1, s);
    reps.insert(reps.end(), s->replicas.begin(), s->replicas.end());
    if (reps.size() > 1 && stream)
        return set_err(RTG_ERR_INVALID, "a multi-device scene is updated synchronously (stream must be NULL)");
    // every replica's tables first: nothing is changed unless all of them accept the description
    std::vector<rtg::SceneTables> tables(reps.size());
    try {
        for (size_t i = 0; i < reps.size(); ++i) {
            std::string err;
            const int rc = rtg::update_scene_tables(d, reps[i]->kept, reps[i]->opt, tables[i], err);
            if (rc) return set_err(rc, "%s", err.c_str());
        }
    } catch (const std::bad_alloc&) {
        return set_err(RTG_ERR_NOMEM, "out of memory");
    }
    for (size_t i = 0; i < reps.size(); ++i) {
        rtg_scene* r = reps[i];
        hipStream_t st = (hipStream_t)stream;
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipEventSynchronize(r->updated));       // the last update's copies read `staged`
        r->staged = std::move(tables[i]);
        const rtg::SceneTables& T = r->staged;
        HIP_TRY(r->objects.update(T.objects, st)); HIP_TRY(r->group_box.update(T.group_box, st));
        HIP_TRY(r->point_xf.update(T.point_xf, st));
        HIP_TRY(r->materials.update(T.materials, st)); HIP_TRY(r->brdfs.update(T.brdfs, st));
        HIP_TRY(r->textures.update(T.textures, st));
        HIP_TRY(r->point_lights.update(T.point_lights, st)); HIP_TRY(r->area_lights.update(T.area_lights, st));
        HIP_TRY(r->dir_lights.update(T.dir_lights, st)); HIP_TRY(r->spot_lights.update(T.spot_lights, st));
        HIP_TRY(r->env_images.update(T.env_images, st));
        HIP_TRY(r->mesh_lights.update(T.mesh_lights, st));
        // env_mix depends on the light's index alone: extended when there are more env lights
        // than ever, into a buffer of this scene's own (clones may share the old one)
        if (T.env_mix.size() > r->env_mix->n) {
            auto grown = std::make_shared<DevBuf<unsigned long long>>();
            HIP_TRY(grown->upload(T.env_mix));
            r->env_mix = grown;
        }
        HIP_TRY(hipEventRecord(r->updated, st));
        // rtg_render and the host-buffer queries run on the scene's own stream
        HIP_TRY(hipStreamWaitEvent(r->stream, r->updated, 0));
        scene_state(r, d, T);
        if (reps.size() > 1) HIP_TRY(hipEventSynchronize(r->updated));
    }
    return RTG_OK;
}

int rtg_scene_set_camera(rtg_scene* s, int32_t index, const rtg_camera* cam) {
    if (!s || !cam) return set_err(RTG_ERR_INVALID, "null argument");
    if (index < 0 || index > (int32_t)s->cameras.size())
        return set_err(RTG_ERR_INVALID, "camera index %d: the scene has %zu (index == count appends)", index,
                       s->cameras.size());
    std::vector<rtg_scene*> reps(1, s);
    reps.insert(reps.end(), s->replicas.begin(), s->replicas.end());
    for (rtg_scene* r : reps) {
        if (index == (int32_t)r->cameras.size()) r->cameras.push_back(*cam);
        else r->cameras[index] = *cam;
    }
    return RTG_OK;
}

int rtg_scene_num_cameras(const rtg_scene* s, int32_t* count) {
    if (!s || !count) return set_err(RTG_ERR_INVALID, "null argument");
    *count = (int32_t)s->cameras.size();
    return RTG_OK;
}

int rtg_camera_setup(const rtg_camera_view* view, rtg_camera* cam) {
    if (!view || !cam) return set_err(RTG_ERR_INVALID, "null argument");
    rtg::camera_setup(*view, *cam);
    return RTG_OK;
}

int rtg_scene_clone(const rtg_scene* src, rtg_scene** out) {
    if (!src || !out) return set_err(RTG_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!src->replicas.empty()) return set_err(RTG_ERR_INVALID, "a multi-device scene cannot be cloned");
    HIP_TRY(hipSetDevice(src->device));
    std::unique_ptr<rtg_scene> sc(new (std::nothrow) rtg_scene);
    if (!sc) return set_err(RTG_ERR_NOMEM, "out of memory");
    sc->device = src->device;
    sc->geom = src->geom;
    sc->env_mix = src->env_mix;
    sc->opt = src->opt;
    try {
        sc->kept = src->kept;
        sc->staged = src->staged;       // the source's tables in effect (read-only for its copies in flight)
        sc->cameras = src->cameras;
    } catch (const std::bad_alloc&) {
        return set_err(RTG_ERR_NOMEM, "out of memory");
    }
    if (int rc = upload_mutable(sc.get(), sc->staged)) return rc;
    sc->feat = src->feat; sc->shade_sk = src->shade_sk; sc->num_slots = src->num_slots;
    sc->wave_ok = src->wave_ok; sc->tree_ok = src->tree_ok; sc->path_ok = src->path_ok;
    sc->max_depth = src->max_depth;
    sc->closest_feat = src->closest_feat; sc->closest_bad = src->closest_bad;
    // the source's DevScene over the clone's own tables (pointers where the source has entries)
    rtg::DevScene& S = sc->ds;
    S = src->ds;
    S.objects = sc->objects.ptr(); S.group_box = sc->group_box.ptr(); S.materials = sc->materials.ptr();
    S.brdfs = sc->brdfs.ptr(); S.textures = sc->textures.ptr();
    S.point_lights = sc->point_lights.ptr(); S.area_lights = sc->area_lights.ptr(); S.dir_lights = sc->dir_lights.ptr();
    S.spot_lights = sc->spot_lights.ptr(); S.env_images = sc->env_images.ptr(); S.mesh_lights = sc->mesh_lights.ptr();
    S.guard = sc->guard.p;
    HIP_TRY(hipDeviceSynchronize());
    *out = sc.release();
    return RTG_OK;
}

int rtg_scene_shares_geometry(const rtg_scene* a, const rtg_scene* b, int32_t* yes) {
    if (!a || !b || !yes) return set_err(RTG_ERR_INVALID, "null argument");
    *yes = a->geom == b->geom ? 1 : 0;
    return RTG_OK;
}

int rtg_scene_create_multi(const rtg_scene_desc* d, const int32_t* devices, int32_t n, rtg_scene** out) {
    if (!d || !out || !devices || n < 1) return set_err(RTG_ERR_INVALID, "bad device list");
    *out = nullptr;
    rtg_scene* first = nullptr;
    int rc = rtg_scene_create(d, devices[0], &first);
    if (rc) return rc;
    std::unique_ptr<rtg_scene> sc(first);
    for (int i = 1; i < n; ++i) {
        rtg_scene* r = nullptr;
        rc = rtg_scene_create(d, devices[i], &r);
        if (rc) return rc;
        sc->replicas.push_back(r);
    }
    *out = sc.release();
    return RTG_OK;
}

int rtg_scene_num_devices(const rtg_scene* s, int32_t* n) {
    if (!s || !n) return set_err(RTG_ERR_INVALID, "null argument");
    *n = 1 + (int32_t)s->replicas.size();
    return RTG_OK;
}

void rtg_scene_destroy(rtg_scene* s) {
    delete s;
}

// Band k of part `part` of `parts` (rtgpu.h RTG_PART_BAND_ROWS; part_row in rtg_frame.hpp):
// round-robin, rotated by one slot per round of `parts` bands.  Increasing in k.
static int part_band(int part, int parts, int k) {
    int slot = (part - k) % parts;
    if (slot < 0) slot += parts;
    return k * parts + slot;
}

int rtg_part_runs(int32_t row_begin, int32_t row_end, int32_t part, int32_t parts, int32_t* runs, int32_t cap,
                  int32_t* count) {
    if (!count) return set_err(RTG_ERR_INVALID, "null argument");
    if (parts <= 0) parts = 1;
    if (part < 0 || part >= parts || row_begin < 0 || row_end < row_begin)
        return set_err(RTG_ERR_INVALID, "bad partition (part %d of %d, rows [%d, %d))", part, parts, row_begin, row_end);
    int n = 0, r0 = -1, r1 = -1;
    for (int k = 0, b = part_band(part, parts, 0); row_begin + b * RTG_PART_BAND_ROWS < row_end;
         b = part_band(part, parts, ++k)) {
        const int a = row_begin + b * RTG_PART_BAND_ROWS, e = std::min(a + RTG_PART_BAND_ROWS, (int)row_end);
        if (a == r1) { r1 = e; continue; }
        if (r0 >= 0) { if (runs && n < cap) { runs[2 * n] = r0; runs[2 * n + 1] = r1; } ++n; }
        r0 = a; r1 = e;
    }
    if (r0 >= 0) { if (runs && n < cap) { runs[2 * n] = r0; runs[2 * n + 1] = r1; } ++n; }
    *count = n;
    return RTG_OK;
}

// Block -> tile assignment.  The hardware deals workgroups to the 8 XCDs round-robin
// (block b runs on XCD b % 8), and each XCD has its own L2: each XCD gets whole 64x64-pixel
// super-tiles (4x4 tiles), dealt round-robin over the image, so an XCD's blocks share BVH nodes
// in its L2 while every XCD sees a spread of the image (traversal cost varies strongly with
// image position: one contiguous band per XCD left XCDs idle, 3.1 -> 5.3 Grays/s on the headline
// when this was fixed; super-tiles of 32 / 128 / 256 px and row-major tiles measured no better,
// DESIGN.md §4).
static std::vector<int> build_tile_map(int tx, int ty) {
    const int n = tx * ty;
    std::vector<int> order(n);
    for (int t = 0; t < n; ++t) order[t] = t;
    const int S = 4, stx = (tx + S - 1) / S;
    auto key = [&](int t) {
        const int x = t % tx, y = t / tx;
        const int st = (y / S) * stx + x / S;
        return std::make_tuple(st % 8, st / 8, (y % S) * S + x % S);
    };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
    // block 8k + x (XCD x) takes the k-th tile of XCD x's contiguous share of `order`
    std::vector<int> map(n);
    int prefix = 0;
    for (int x = 0; x < 8; ++x) {
        const int cnt = (n - x + 7) / 8;
        for (int k = 0; k < cnt; ++k) map[8 * k + x] = order[prefix + k];
        prefix += cnt;
    }
    return map;
}

static int ensure_tile_map(rtg_scene* s, int tx, int ty, const int** out) {
    for (auto& m : s->tile_maps)
        if (m->tx == tx && m->ty == ty) {
            *out = m->map.p;
            return RTG_OK;
        }
    HIP_TRY(hipSetDevice(s->device));
    std::unique_ptr<TileMap> m(new TileMap{tx, ty, {}});
    HIP_TRY(m->map.upload(build_tile_map(tx, ty)));
    *out = m->map.p;
    s->tile_maps.push_back(std::move(m));
    return RTG_OK;
}

// A camera's device record (shared by the renders and rtg_camera_rays*).
static void dev_camera(const rtg_camera& c, rtg::DevCamera& C) {
    std::memset(&C, 0, sizeof(C));
    auto cp = [](float* d, const rtg_float3& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; };
    cp(C.pos, c.position); cp(C.gaze, c.gaze); cp(C.up, c.up); cp(C.right, c.right); cp(C.q, c.q);
    C.left = c.left; C.right_ext = c.right_ext; C.bottom = c.bottom; C.top = c.top;
    C.focus_distance = c.focus_distance; C.aperture = c.aperture;
    C.width = c.width; C.height = c.height; C.spp = c.spp < 1 ? 1 : c.spp;
    C.path_tracing = c.path_tracing; C.next_event = c.next_event;
    C.importance_sampling = c.importance_sampling; C.russian_roulette = c.russian_roulette;
}

// Camera i of scene s; with `image`, one that has pixels.
static int scene_camera(const rtg_scene* s, int i, bool image, const rtg_camera*& c) {
    if (i < 0 || i >= (int)s->cameras.size()) return set_err(RTG_ERR_INVALID, "bad camera %d", i);
    c = &s->cameras[i];
    if (image && (c->width <= 0 || c->height <= 0)) return set_err(RTG_ERR_INVALID, "camera %d has an empty image", i);
    return RTG_OK;
}

// The rows [row_begin, row_end) a render's options name in an image of `height` rows.
static void clamp_rows(const rtg_render_opts* o, int height, int& row_begin, int& row_end) {
    row_begin = o->row_begin < 0 ? 0 : o->row_begin;
    row_end = (o->row_end <= 0 || o->row_end > height) ? height : o->row_end;
}

// A scene and its replicas (rtg_scene_create_multi).
static std::vector<rtg_scene*> with_replicas(rtg_scene* s) {
    std::vector<rtg_scene*> reps(1, s);
    reps.insert(reps.end(), s->replicas.begin(), s->replicas.end());
    return reps;
}

static int prepare(rtg_scene* s, const rtg_render_opts* o, rtg::DevCamera& C, rtg::RenderParams& P) {
    if (!s || !o) return set_err(RTG_ERR_INVALID, "null argument");
    const rtg_camera* cam = nullptr;
    if (int rc = scene_camera(s, o->camera, true, cam)) return rc;
    const rtg_camera& c = *cam;
    dev_camera(c, C);
    std::memset(&P, 0, sizeof(P));
    clamp_rows(o, c.height, P.row_begin, P.row_end);
    if (P.row_begin >= P.row_end) return set_err(RTG_ERR_INVALID, "empty row range");
    P.sample_begin = o->sample_begin < 0 ? 0 : o->sample_begin;
    P.sample_count = o->sample_count < 0 ? C.spp : o->sample_count;
    P.accum_only = (o->flags & RTG_RENDER_ACCUM_ONLY) ? 1 : 0;
    if (!P.accum_only && (P.sample_begin != 0 || P.sample_count != C.spp))
        return set_err(RTG_ERR_INVALID, "a partial sample range requires RTG_RENDER_ACCUM_ONLY");
    P.part_count = o->part_count <= 0 ? 1 : o->part_count;
    P.part_index = o->part_index;
    if (P.part_index < 0 || P.part_index >= P.part_count)
        return set_err(RTG_ERR_INVALID, "part %d of %d", P.part_index, P.part_count);
    // this part's bands of RTG_PART_BAND_ROWS rows (part_row in rtg_frame.hpp) and its row
    // count; tiles of 16 compact rows (two bands; a wave's 8 rows are one band)
    static_assert(RTG_PART_BAND_ROWS == 8, "part_row's band shift");
    const int bands = (P.row_end - P.row_begin + RTG_PART_BAND_ROWS - 1) / RTG_PART_BAND_ROWS;
    int own = 0;
    while (part_band(P.part_index, P.part_count, own) < bands) ++own;
    P.part_rows = 0;
    if (own > 0) {
        const int lastBand = part_band(P.part_index, P.part_count, own - 1);
        P.part_rows = (own - 1) * RTG_PART_BAND_ROWS +
                      std::min(RTG_PART_BAND_ROWS, P.row_end - P.row_begin - lastBand * RTG_PART_BAND_ROWS);
    }
    P.tiles_x = (c.width + 15) / 16;
    P.tiles_y = (P.part_rows + 15) / 16;
    P.num_tiles = P.tiles_x * P.tiles_y;
    if (P.num_tiles == 0) return RTG_OK;   // nothing of this part in the row range
    // one sample per pass until launch() chooses more (pass_slabs)
    P.slabs = 1;
    P.slab_tiles = P.num_tiles;
    P.slab_px = 16 * P.tiles_y * c.width;
    P.seed = o->seed;
    const int* map = nullptr;
    int rc = ensure_tile_map(s, P.tiles_x, P.tiles_y, &map);
    if (rc) return rc;
    P.tile_map = map;
    return RTG_OK;
}

// The wavefront pipeline's one-shadow-light layout (rtg_wave.hpp SH_ONE): payload float4s per
// queued shadow ray -- 2 with at most one light, 3 with one point / area light followed by one
// environment light (its term travels with the shadow ray: C4), 0 otherwise (general layout)
static int one_payload(const rtg_scene* s) {
    const rtg::DevScene& S = s->ds;
    if (s->num_slots <= 1) return 2;
    if (s->num_slots == 2 && S.num_env == 1 && S.num_point + S.num_area == 1 && S.num_dir + S.num_spot + S.num_mesh == 0)
        return 3;
    return 0;
}

// Sizes the wavefront buffers for `pixels` pixel entries x `slots` light slots and `tiles`
// shade blocks (queue segments of 256 * slots entries), one allocation; `pay`: one-layout
// payload float4s per queue entry (one_payload); `col`: with the colour buffer of multi-sample
// passes (one float4 per entry).
static int ensure_wave(WaveWork& ww, size_t pixels, int slots, size_t tiles, int pay, bool col = false) {
    const rtg::WaveShape want{pixels, tiles, slots, pay, col};
    if (ww.mem.p && ww.shape.covers(want)) return RTG_OK;
    ww.dq.release();
    ww.dq_shape = {};
    ww.mem.release();
    const rtg::WaveShape sh = ww.shape.merged(want);
    const rtg::WaveLayout L = rtg::wave_layout(sh);
    HIP_TRY(ww.mem.reserve(L.total));
    auto at = [&](rtg::WavePiece k) { return (void*)(ww.mem.p + L.off[k]); };
    rtg::WaveBufs& W = ww.W;
    W.hit_t = (float*)at(rtg::WP_HIT_T); W.hit_obj = (int*)at(rtg::WP_HIT_OBJ); W.hit_face = (int*)at(rtg::WP_HIT_FACE);
    W.base = (float4*)at(rtg::WP_BASE); W.term = (float4*)at(rtg::WP_TERM); W.occ = (unsigned char*)at(rtg::WP_OCC);
    W.q_o = (float4*)at(rtg::WP_Q_O); W.q_d = (float4*)at(rtg::WP_Q_D); W.q_slot = (int*)at(rtg::WP_Q_SLOT);
    W.q_count = (int*)at(rtg::WP_Q_COUNT); W.accum = (float4*)at(rtg::WP_ACCUM);
    W.q_pay = sh.pay ? (float4*)at(rtg::WP_Q_PAY) : nullptr;
    W.pay3 = sh.pay == 3;
    W.col = sh.col ? (float4*)at(rtg::WP_COL) : nullptr;
    ww.shape = sh;
    W.dq_e = nullptr;
    W.dq_count = nullptr;
    W.hit_key = nullptr;
    W.shadow_state = nullptr;
    W.dq_cap = 0;
    return RTG_OK;
}

// The deferred-leaf queue of a large-leaf scene's camera walk (work_layout.hpp defer_layout),
// for a pass of `pixels` entries and `nq` shadow-queue entries on stream `st`.
static int ensure_defer(WaveWork& ww, size_t pixels, size_t nq, hipStream_t st) {
    const rtg::DeferShape want{pixels, nq};
    if (ww.dq.p && ww.dq_shape.covers(want)) return RTG_OK;
    const rtg::DeferShape sh = ww.dq_shape.merged(want);
    const rtg::DeferLayout L = rtg::defer_layout(sh.pixels, sh.nq);
    HIP_TRY(ww.dq.reserve(L.total));
    // the counters start at zero; the kernels after their last readers zero them for the next
    // pass (k_shade: camera entries / unsettled pixels, k_shadow_fin*: shadow entries)
    HIP_TRY(hipMemsetAsync(ww.dq.p, 0, 256, st));
    char* b = ww.dq.p;
    ww.W.dq_count = (int*)(b + L.counts);
    ww.W.hit_key = (unsigned long long*)(b + L.keys);
    ww.W.dq_e = (float4*)(b + L.entries);
    ww.W.shadow_state = (int*)(b + L.states);
    ww.W.dq_cap = (int)L.cap;
    ww.dq_shape = sh;
    return RTG_OK;
}

// The render pipeline a frame part takes (launch): path tracer, ray trees, wavefront, fused.
enum { PIPE_PATH, PIPE_TREE, PIPE_WAVE, PIPE_MEGA };
static int pipeline(const rtg_scene* s, const rtg_render_opts* o, const rtg::DevCamera& C, const rtg::RenderParams& P) {
    if (C.path_tracing && s->path_ok && !(o->flags & RTG_RENDER_FUSED) && (o->flags & RTG_RENDER_TREE)) return PIPE_PATH;
    const long long work = (long long)P.part_rows * C.width * P.sample_count;
    const bool fused_only = (o->flags & RTG_RENDER_FUSED) || C.path_tracing;
    if (s->tree_ok && !fused_only && ((o->flags & RTG_RENDER_TREE) || work >= (1ll << 21))) return PIPE_TREE;
    if (s->wave_ok && !fused_only) return PIPE_WAVE;
    return PIPE_MEGA;
}

// Samples per pass of the wavefront and ray-tree pipelines (RenderParams::slabs): as many as
// keep a pass at most ~RTG_PASS_RAYS camera rays (default 16 Mi: a 1920x1080 frame of 8 samples,
// two 3840x2160 samples -- against 8 Mi: C4 3 519 -> 3 563 Mrays/s in flight, 3 203 -> 3 356
// serial, C5 2 265 -> 2 329; profiles/r06u_pass_rays_ab.txt), spread evenly over the passes.  A pass's launches then stay full when
// a GPU renders a small part of the frame, and a frame of few passes pays the tail of its
// slowest waves (C3's pole fans, C5's deepest trees) once per pass, not once per sample.
// RTG_PASS_RAYS=0: one sample per pass (round 5's passes; the image is the same bit for bit).
static int pass_slabs(const rtg::RenderParams& P, int width) {
    const char* v = std::getenv("RTG_PASS_RAYS");
    const long long target = v ? std::atoll(v) : (16ll << 20);
    const long long px = (long long)P.part_rows * width;
    if (target <= 0 || P.sample_count <= 1 || px <= 0) return 1;
    const long long k = std::max(1ll, std::min<long long>(target / px, P.sample_count));
    const long long passes = (P.sample_count + k - 1) / k;
    return (int)((P.sample_count + passes - 1) / passes);
}

// samples of the last pass (the one RTG_RENDER_TIMING times)
static int last_pass_samples(const rtg::RenderParams& P) {
    return P.sample_count - ((P.sample_count - 1) / P.slabs) * P.slabs;
}

static int launch(rtg_scene* s, const rtg_render_opts* o, const rtg::DevCamera& C, const rtg::RenderParams& P0,
                  float* d_hdr, uint8_t* d_ldr, float* d_accum, hipStream_t stream) {
    WaveWork& ww = s->work;
    int pipe = pipeline(s, o, C, P0);
    rtg::RenderParams P = P0;
    if ((pipe == PIPE_WAVE || pipe == PIPE_TREE) && !(o->flags & RTG_RENDER_SAMPLE_PASSES)) {
        P.slabs = pass_slabs(P, C.width);
        if (P.slabs > 1) P.slab_tiles = (P.num_tiles + 7) & ~7;   // a tile keeps its XCD in every slab
    }
    const bool stats = (o->flags & RTG_RENDER_COUNT_STATS) != 0;
    // RTG_RENDER_EXACT_SHADOW: shadow rays walk the reference BVH (cross-checks of the wide one)
    rtg::DevScene ds = s->ds;
    if (o->flags & RTG_RENDER_EXACT_SHADOW) ds.exact_shadow = 1;
    // RTG_RENDER_ORDERED: the checked closest-hit walk on the any-hit tree (its leaf boxes must be
    // the reference's: not the split tree).  (Round 3's per-lane walk of the reference tree
    // collapsed to 4 wide was removed in round 6.)
    if ((o->flags & RTG_RENDER_ORDERED) && ds.anodes && !ds.ahb_split && ds.face_leaf) ds.ordered = 1;
    hipEvent_t* ev = nullptr;
    if (o->flags & RTG_RENDER_TIMING) {
        for (auto& e : s->ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        ev = s->ev;
    }
    // ray trees: the wavefront tree pipeline for large frames (it synchronises once per tree
    // level), the fused kernel otherwise; RTG_RENDER_TREE / RTG_RENDER_FUSED force either.
    // Path tracing: the fused kernel; the wavefront path tracer (rtg_path.hip, same image bit
    // for bit) with RTG_RENDER_TREE -- measured slower than the fused kernel on the path-tracing
    // fixtures, so it is opt-in
    if (pipe == PIPE_PATH) {
        float4* acc = (float4*)d_accum;
        if (!P.accum_only && C.spp > 1) {   // internal accumulator indexed by absolute pixel
            int rc = ensure_wave(ww, (size_t)C.width * C.height, s->num_slots, (size_t)P.num_tiles, 0);
            if (rc) return rc;
            acc = ww.W.accum;
        }
        // a counted render that falls back to the fused kernel must not keep the abandoned
        // pass's counts: snapshot the counters, restore them before the fused kernel runs
        rtg::DevCounters snap{};
        if (stats) {
            HIP_TRY(hipMemcpyAsync(&snap, s->counters.p, sizeof(snap), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        const hipError_t pe = rtg::launch_path(s->path, ds, C, P, d_hdr, d_ldr, acc, s->counters.p, stats, s->feat,
                                               s->shade_sk, stream, ev);
        if (pe == hipSuccess) {
            if (ev) { s->timed_layout = rtg::LAYOUT_PATH; s->timed_samples = 1; }
            return RTG_OK;
        }
        if (pe != hipErrorNotSupported) HIP_TRY(pe);
        (void)hipGetLastError();
        if (stats) {
            HIP_TRY(hipMemcpyAsync(s->counters.p, &snap, sizeof(snap), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        pipe = PIPE_MEGA;                   // path-tracing cameras: the fused kernel
    }
    if (pipe == PIPE_TREE) {
        float4* acc = (float4*)d_accum;
        if (!P.accum_only && C.spp > 1) {   // internal accumulator indexed by absolute pixel
            int rc = ensure_wave(ww, (size_t)C.width * C.height, s->num_slots, (size_t)P.num_tiles, 0);
            if (rc) return rc;
            acc = ww.W.accum;
        }
        HIP_TRY(rtg::launch_tree(s->tree, ds, C, P, d_hdr, d_ldr, acc, s->counters.p, stats, s->feat, s->shade_sk,
                                 stream, ev));
        if (ev) { s->timed_layout = rtg::LAYOUT_TREE; s->timed_samples = last_pass_samples(P); }
        return RTG_OK;
    }
    if (pipe == PIPE_WAVE) {
        // work-buffer entries and shade blocks of a pass (all its sample slabs)
        const size_t entries = P.slabs > 1 ? (size_t)P.slabs * P.slab_px : (size_t)P.part_rows * C.width;
        const size_t blocks = (size_t)P.slab_tiles * P.slabs;
        int rc = ensure_wave(ww, entries, s->num_slots, blocks, one_payload(s), P.slabs > 1);
        if (rc) return rc;

        // the shadow-ray layout is the scene's as it is now: buffers sized for another one (before
        // an rtg_scene_update changed the lights) only have room to spare
        auto layout_now = [&](rtg::WaveBufs& B) {
            const int pay = one_payload(s);
            B.num_slots = s->num_slots;
            B.pay3 = pay == 3;
            if (!pay) B.q_pay = nullptr;
        };
        rtg::WaveBufs W = ww.W;
        layout_now(W);
        if (P.accum_only) W.accum = (float4*)d_accum;
        else if (C.spp > 1) {   // internal accumulator indexed by absolute pixel
            size_t need = (size_t)C.width * C.height;
            if (need > ww.shape.pixels) {
                int rc2 = ensure_wave(ww, need, s->num_slots, blocks, one_payload(s), P.slabs > 1);
                if (rc2) return rc2;
                W = ww.W;
                layout_now(W);
            }
        }
        if ((s->feat & rtg::FEAT_BIGLEAF) && !stats && rtg::defer_leaves()) {
            rc = ensure_defer(ww, entries, blocks * 256 * std::max(s->num_slots, 1), stream);
            if (rc) return rc;
            W.dq_e = ww.W.dq_e;
            W.dq_count = ww.W.dq_count;
            W.hit_key = ww.W.hit_key;
            W.shadow_state = ww.W.shadow_state;
            W.dq_cap = ww.W.dq_cap;
        }
        int layout = rtg::LAYOUT_WAVE;
        HIP_TRY(rtg::launch_wave(ds, C, P, W, d_hdr, d_ldr, s->counters.p, stats, s->feat, s->shade_sk, stream, ev,
                                 &layout));
        if (ev) { s->timed_layout = layout; s->timed_samples = last_pass_samples(P); }
        return RTG_OK;
    }
    HIP_TRY(rtg::launch_mega(ds, C, P, d_hdr, d_ldr, d_accum, s->counters.p, stats, s->shade_sk, s->feat, stream, ev));
    if (ev) { s->timed_layout = rtg::LAYOUT_MEGA; s->timed_samples = P.sample_count; }
    return RTG_OK;
}

int rtg_render_device(rtg_scene* s, const rtg_render_opts* o, float* d_hdr, uint8_t* d_ldr, float* d_accum,
                      void* stream) {
    rtg::DevCamera C;
    rtg::RenderParams P;
    int rc = prepare(s, o, C, P);
    if (rc) return rc;
    if (P.accum_only && !d_accum) return set_err(RTG_ERR_INVALID, "RTG_RENDER_ACCUM_ONLY needs an accumulation buffer");
    if (P.num_tiles == 0) return RTG_OK;
    HIP_TRY(hipSetDevice(s->device));
    rc = launch(s, o, C, P, d_hdr, d_ldr, d_accum, (hipStream_t)stream);
    if (rc) return rc;
    // the completion marker rtg_scene_stats waits for (round 4 measured a render without it: the
    // same part-frame time, profiles/r04f_parts_ab.jsonl)
    HIP_TRY(hipEventRecord(s->done, (hipStream_t)stream));
    return RTG_OK;
}

// D2H of the rows of opts' part: one async copy per run of consecutive rows, straight into
// the same offsets of the host frame (layout 3*(x + y*width), main.cpp:109).
static int copy_part(const rtg_render_opts* o, int width, int height, const float* d_hdr, const uint8_t* d_ldr,
                     float* hdr, uint8_t* ldr, hipStream_t st) {
    int rb, re;
    clamp_rows(o, height, rb, re);
    int32_t n = 0;
    int rc = rtg_part_runs(rb, re, o->part_index, o->part_count, nullptr, 0, &n);
    if (rc) return rc;
    std::vector<int32_t> runs(2 * (size_t)n);
    rc = rtg_part_runs(rb, re, o->part_index, o->part_count, runs.data(), n, &n);
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        const size_t off = (size_t)runs[2 * k] * width * 3, cnt = (size_t)(runs[2 * k + 1] - runs[2 * k]) * width * 3;
        if (hdr && d_hdr) HIP_TRY(hipMemcpyAsync(hdr + off, d_hdr + off, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
        if (ldr && d_ldr) HIP_TRY(hipMemcpyAsync(ldr + off, d_ldr + off, cnt, hipMemcpyDeviceToHost, st));
    }
    return RTG_OK;
}

int rtg_copy_part_to_host(rtg_scene* s, const rtg_render_opts* o, const float* d_hdr, const uint8_t* d_ldr,
                          float* hdr_rgb, uint8_t* ldr_rgb, void* stream) {
    if (!s || !o) return set_err(RTG_ERR_INVALID, "null argument");
    const rtg_camera* c = nullptr;
    if (int rc = scene_camera(s, o->camera, false, c)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    return copy_part(o, c->width, c->height, d_hdr, d_ldr, hdr_rgb, ldr_rgb, (hipStream_t)stream);
}

// (Round 4's overlapped host path -- the frame rendered in row chunks on two streams, each
// chunk's rows copied to the host under the next chunks -- measured slower than one launch + one
// copy at every chunk count, profiles/r04d_hostpath.jsonl, and was removed in round 6; page-locked
// frames take the direct writes below.)

// The device's view of a page-locked host buffer (rtg_host_alloc / rtg_host_register), or null.
static void* device_view(void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}
// Page-locked caller frames (rtg_host_alloc / rtg_host_register, as the CLIs and the shared
// frame of multigpu.py allocate them): the kernels write the pixels straight into the frame over
// the bus -- no device frame and no copy after the render, the writes overlap the rendering
// (headline 1080p frame: 0.53 -> 0.46 ms per frame, profiles/r04e_hostpath.jsonl).  Pageable
// frames take the render + copy path.  RTG_HOST_DIRECT=0: render + copy always (A/B).
static bool host_direct() {
    const char* v = std::getenv("RTG_HOST_DIRECT");
    return !v || std::strcmp(v, "0") != 0;
}

// Replaces main.cpp:164-185.  With replicas (rtg_scene_create_multi) replica i renders part
// i of n on its own stream and copies its rows into the caller's buffers; the renders of all
// replicas are enqueued before any copy (a copy to pageable memory may block the host), then
// every stream is synchronised -- never the whole device.
int rtg_render(rtg_scene* s, const rtg_render_opts* o, float* hdr_rgb, uint8_t* ldr_rgb) {
    if (!s || !o) return set_err(RTG_ERR_INVALID, "null argument");
    if (o->flags & RTG_RENDER_ACCUM_ONLY) return set_err(RTG_ERR_INVALID, "use rtg_render_device for RTG_RENDER_ACCUM_ONLY");
    const std::vector<rtg_scene*> reps = with_replicas(s);
    const int n = (int)reps.size();
    if (n > 1 && o->part_count > 1)
        return set_err(RTG_ERR_INVALID, "a multi-device scene deals its own partition (part_count must be <= 1)");
    const rtg_camera* camp = nullptr;
    if (int rc = scene_camera(s, o->camera, false, camp)) return rc;
    const rtg_camera& cam = *camp;
    std::vector<rtg_render_opts> ro(n, *o);
    bool whole = false;
    if (n == 1 && host_direct() && !cam.has_tonemapper && (hdr_rgb || ldr_rgb)) {
        float* dh = (float*)device_view(hdr_rgb);
        uint8_t* dl = (uint8_t*)device_view(ldr_rgb);
        if ((!hdr_rgb || dh) && (!ldr_rgb || dl)) {
            rtg::DevCamera C;
            rtg::RenderParams P;
            int rc = prepare(s, o, C, P);
            if (rc) return rc;
            if (P.num_tiles == 0) return RTG_OK;
            HIP_TRY(hipSetDevice(s->device));
            rc = launch(s, o, C, P, dh, dl, nullptr, s->stream);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(s->done, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            return RTG_OK;
        }
    }
    for (int i = 0; i < n; ++i) {
        rtg_scene* r = reps[i];
        if (n > 1) { ro[i].part_index = i; ro[i].part_count = n; }
        rtg::DevCamera C;
        rtg::RenderParams P;
        int rc = prepare(r, &ro[i], C, P);
        if (rc) return rc;
        whole = P.row_begin == 0 && P.row_end == C.height && (n > 1 || P.part_count == 1);
        HIP_TRY(hipSetDevice(r->device));
        const size_t pixels = (size_t)C.width * C.height;
        if (r->d_ldr.cap < pixels * 3) {
            HIP_TRY(hipStreamSynchronize(r->stream));
            r->d_hdr.release();
            r->d_ldr.release();
            HIP_TRY(r->d_hdr.reserve(pixels * 3));
            HIP_TRY(r->d_ldr.reserve(pixels * 3));
        }
        if (P.num_tiles == 0) continue;
        rc = launch(r, &ro[i], C, P, r->d_hdr.p, r->d_ldr.p, nullptr, r->stream);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(r->done, r->stream));
    }
    // tonemapped camera over the whole image: the LDR output is the tonemapped image
    // (main.cpp:187-192); it needs every pixel, so with several parts it runs on the
    // gathered float image
    const bool tonemap = cam.has_tonemapper && whole;
    const rtg_tonemap_params tp = {cam.tm_key, cam.tm_burn, cam.tm_saturation, cam.tm_gamma};
    if (tonemap && n == 1) {
        int rc = rtg_tonemap_device(s->d_hdr.p, cam.width, cam.height, &tp, s->d_ldr.p, s->device, s->stream);
        if (rc) return rc;
    }
    std::vector<float> tmp;
    float* hdr = hdr_rgb;
    if (tonemap && n > 1 && ldr_rgb && !hdr) {
        tmp.resize((size_t)cam.width * cam.height * 3);
        hdr = tmp.data();
    }
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipSetDevice(reps[i]->device));
        int rc = copy_part(&ro[i], cam.width, cam.height, reps[i]->d_hdr.p, reps[i]->d_ldr.p, hdr,
                           (tonemap && n > 1) ? nullptr : ldr_rgb, reps[i]->stream);
        if (rc) return rc;
    }
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipSetDevice(reps[i]->device));
        HIP_TRY(hipStreamSynchronize(reps[i]->stream));
    }
    if (tonemap && n > 1 && ldr_rgb) return rtg_tonemap(hdr, cam.width, cam.height, &tp, ldr_rgb, s->device);
    return RTG_OK;
}

// ---- ray queries (rtg_query.hip)
static int query_args(const rtg_scene* s, const void* rays, int64_t n, uint32_t flags, const void* hits) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld rays: at most INT32_MAX per call", (long long)n);
    if (flags & ~(uint32_t)(RTG_QUERY_ANY_HIT | RTG_QUERY_COHERENT))
        return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n > 0 && (!rays || !hits)) return set_err(RTG_ERR_INVALID, "null buffer");
    return RTG_OK;
}

int rtg_trace_rays_device(rtg_scene* s, const rtg_ray* d_rays, int64_t n, uint32_t flags, rtg_hit* d_hits,
                          float* d_normals, void* stream) {
    int rc = query_args(s, d_rays, n, flags, d_hits);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_query(s->ds, s->feat, d_rays, (int)n, flags, d_hits,
                              (flags & RTG_QUERY_ANY_HIT) ? nullptr : (float4*)d_normals, (hipStream_t)stream));
    return RTG_OK;
}

// One staged buffer of a call: copied in from `in` before the launch, out to `out` after it
// (either may be null); bytes == 0: the call does without it
struct Staged {
    QuerySlot slot;
    size_t bytes;
    const void* in;
    void* out;
};

// slot `k` of at least `bytes`
static int query_scratch(rtg_scene* s, QuerySlot k, size_t bytes) {
    if (s->q[k].cap >= bytes) return RTG_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->q[k].reserve(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(RTG_ERR_NOMEM, "query scratch of %zu bytes", bytes);
    }
    return RTG_OK;
}

// every buffer's capacity first, then the copies in, on the scene's stream
static int stage(rtg_scene* s, std::initializer_list<Staged> bufs) {
    for (const Staged& b : bufs)
        if (b.bytes)
            if (int rc = query_scratch(s, b.slot, b.bytes)) return rc;
    for (const Staged& b : bufs)
        if (b.bytes && b.in) HIP_TRY(hipMemcpyAsync(s->q[b.slot].p, b.in, b.bytes, hipMemcpyHostToDevice, s->stream));
    return RTG_OK;
}

// the copies out, then the stream's end
static int unstage(rtg_scene* s, std::initializer_list<Staged> bufs) {
    for (const Staged& b : bufs)
        if (b.bytes && b.out) HIP_TRY(hipMemcpyAsync(b.out, s->q[b.slot].p, b.bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return RTG_OK;
}

int rtg_trace_rays(rtg_scene* s, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_hit* hits, float* normals) {
    int rc = query_args(s, rays, n, flags, hits);
    if (rc || n == 0) return rc;
    if (flags & RTG_QUERY_ANY_HIT) normals = nullptr;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_RAYS, N * sizeof(rtg_ray), rays, nullptr},
                           {Q_HITS, N * sizeof(rtg_hit), nullptr, hits},
                           {Q_NORMALS, normals ? N * 4 * sizeof(float) : 0, nullptr, normals}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_query(s->ds, s->feat, (rtg_ray*)s->q[Q_RAYS].p, (int)n, flags, (rtg_hit*)s->q[Q_HITS].p,
                              normals ? (float4*)s->q[Q_NORMALS].p : nullptr, s->stream));
    return unstage(s, bufs);
}

// ---- multi-hit queries (rtg_multihit.hip)
static int multi_args(const rtg_scene* s, const void* rays, int64_t n, int32_t k, uint32_t flags, const void* hits) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld rays: at most INT32_MAX per call", (long long)n);
    if (k < 1 || k > RTG_MULTIHIT_MAX)
        return set_err(RTG_ERR_INVALID, "k = %d: a multi-hit query holds 1 to %d hits per ray", k, RTG_MULTIHIT_MAX);
    if (flags & RTG_QUERY_ANY_HIT) return set_err(RTG_ERR_INVALID, "RTG_QUERY_ANY_HIT does not apply to a multi-hit query");
    if (flags & ~(uint32_t)RTG_QUERY_COHERENT) return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n > 0 && (!rays || !hits)) return set_err(RTG_ERR_INVALID, "null buffer");
    return RTG_OK;
}

int rtg_trace_rays_multi_device(rtg_scene* s, const rtg_ray* d_rays, int64_t n, int32_t k, uint32_t flags,
                                rtg_hit* d_hits, int32_t* d_counts, void* stream) {
    int rc = multi_args(s, d_rays, n, k, flags, d_hits);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_multihit(s->ds, s->feat, d_rays, (int)n, k, d_hits, d_counts, (hipStream_t)stream));
    return RTG_OK;
}

int rtg_trace_rays_multi(rtg_scene* s, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags, rtg_hit* hits,
                         int32_t* counts) {
    int rc = multi_args(s, rays, n, k, flags, hits);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_RAYS, N * sizeof(rtg_ray), rays, nullptr},
                           {Q_HITS, N * (size_t)k * sizeof(rtg_hit), nullptr, hits},
                           {Q_COUNTS, counts ? N * sizeof(int32_t) : 0, nullptr, counts}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_multihit(s->ds, s->feat, (rtg_ray*)s->q[Q_RAYS].p, (int)n, k, (rtg_hit*)s->q[Q_HITS].p,
                                 counts ? (int*)s->q[Q_COUNTS].p : nullptr, s->stream));
    return unstage(s, bufs);
}

// ---- closest-point queries (rtg_closest.hip)
static int closest_args(const rtg_scene* s, const void* points, int64_t n, uint32_t flags, const void* out) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld points: at most INT32_MAX per call", (long long)n);
    if (flags) return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n > 0 && (!points || !out)) return set_err(RTG_ERR_INVALID, "null buffer");
    if (s->closest_bad >= 0) {
        std::string err;
        const int rc = rtg::closest_unsupported(s->staged.point_xf.data(), (int)s->staged.point_xf.size(), err);
        return set_err(rc, "%s", err.c_str());
    }
    return RTG_OK;
}

int rtg_closest_points_device(rtg_scene* s, const rtg_point* d_points, int64_t n, uint32_t flags, rtg_nearest* d_out,
                              void* stream) {
    int rc = closest_args(s, d_points, n, flags, d_out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_closest(s->ds, s->point_xf.ptr(), s->closest_feat, d_points, (int)n, d_out, (hipStream_t)stream));
    return RTG_OK;
}

int rtg_closest_points(rtg_scene* s, const rtg_point* points, int64_t n, uint32_t flags, rtg_nearest* out) {
    int rc = closest_args(s, points, n, flags, out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_POINTS, N * sizeof(rtg_point), points, nullptr},
                                                {Q_NEAREST, N * sizeof(rtg_nearest), nullptr, out}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_closest(s->ds, s->point_xf.ptr(), s->closest_feat, (rtg_point*)s->q[Q_POINTS].p, (int)n,
                                (rtg_nearest*)s->q[Q_NEAREST].p, s->stream));
    return unstage(s, bufs);
}

// ---- crossing counts and signed distances (rtg_crossings.hip)
static int crossings_args(const rtg_scene* s, const void* rays, int64_t n, uint32_t flags, const void* out) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld rays: at most INT32_MAX per call", (long long)n);
    if (flags & RTG_QUERY_ANY_HIT) return set_err(RTG_ERR_INVALID, "RTG_QUERY_ANY_HIT does not apply to a crossing count");
    if (flags & ~(uint32_t)RTG_QUERY_COHERENT) return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n > 0 && (!rays || !out)) return set_err(RTG_ERR_INVALID, "null buffer");
    return RTG_OK;
}

int rtg_count_crossings_device(rtg_scene* s, const rtg_ray* d_rays, int64_t n, uint32_t flags, rtg_crossings* d_out,
                               void* stream) {
    int rc = crossings_args(s, d_rays, n, flags, d_out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_crossings(s->ds, s->feat, d_rays, (int)n, d_out, (hipStream_t)stream));
    return RTG_OK;
}

int rtg_count_crossings(rtg_scene* s, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_crossings* out) {
    int rc = crossings_args(s, rays, n, flags, out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_RAYS, N * sizeof(rtg_ray), rays, nullptr},
                                                {Q_COUNTS, N * sizeof(rtg_crossings), nullptr, out}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_crossings(s->ds, s->feat, (rtg_ray*)s->q[Q_RAYS].p, (int)n, (rtg_crossings*)s->q[Q_COUNTS].p,
                                  s->stream));
    return unstage(s, bufs);
}

// closest_args with the direction between the argument errors and the ellipsoid refusal
static int signed_distance_args(const rtg_scene* s, const void* points, int64_t n, const float* dir, uint32_t flags,
                                const void* out, float v[3]) {
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld points: at most INT32_MAX per call", (long long)n);
    if (flags) return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n > 0 && (!points || !out)) return set_err(RTG_ERR_INVALID, "null buffer");
    if (const char* e = rtg::signed_distance_dir(dir, v)) return set_err(RTG_ERR_INVALID, "%s", e);
    return closest_args(s, points, n, flags, out);
}

int rtg_signed_distance_points_device(rtg_scene* s, const rtg_point* d_points, int64_t n, const float dir[3],
                                      uint32_t flags, rtg_nearest* d_out, void* stream) {
    float v[3];
    int rc = signed_distance_args(s, d_points, n, dir, flags, d_out, v);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_signed_distance(s->ds, s->point_xf.ptr(), s->closest_feat, d_points, (int)n, v, d_out,
                                        (hipStream_t)stream));
    return RTG_OK;
}

int rtg_signed_distance_points(rtg_scene* s, const rtg_point* points, int64_t n, const float dir[3], uint32_t flags,
                               rtg_nearest* out) {
    float v[3];
    int rc = signed_distance_args(s, points, n, dir, flags, out, v);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_POINTS, N * sizeof(rtg_point), points, nullptr},
                                                {Q_NEAREST, N * sizeof(rtg_nearest), nullptr, out}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_signed_distance(s->ds, s->point_xf.ptr(), s->closest_feat, (rtg_point*)s->q[Q_POINTS].p, (int)n,
                                        v, (rtg_nearest*)s->q[Q_NEAREST].p, s->stream));
    return unstage(s, bufs);
}

// the camera record and row range of a camera-ray batch
static int camera_rays_args(const rtg_scene* s, const rtg_render_opts* o, const void* rays, rtg::DevCamera& C,
                            int& row_begin, int& row_end) {
    if (!s || !o || !rays) return set_err(RTG_ERR_INVALID, "null argument");
    const rtg_camera* c = nullptr;
    if (int rc = scene_camera(s, o->camera, true, c)) return rc;
    dev_camera(*c, C);
    clamp_rows(o, c->height, row_begin, row_end);
    if (row_begin >= row_end) return set_err(RTG_ERR_INVALID, "empty row range");
    if ((int64_t)c->width * c->height > INT32_MAX) return set_err(RTG_ERR_INVALID, "image of more than INT32_MAX pixels");
    return RTG_OK;
}

int rtg_camera_rays_device(rtg_scene* s, const rtg_render_opts* o, rtg_ray* d_rays, void* stream) {
    rtg::DevCamera C;
    int rb, re;
    int rc = camera_rays_args(s, o, d_rays, C, rb, re);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_camera_rays(C, rb, re, o->sample_begin < 0 ? 0 : o->sample_begin, o->seed, d_rays,
                                    (hipStream_t)stream));
    return RTG_OK;
}

int rtg_camera_rays(rtg_scene* s, const rtg_render_opts* o, rtg_ray* rays) {
    rtg::DevCamera C;
    int rb, re;
    int rc = camera_rays_args(s, o, rays, C, rb, re);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const std::initializer_list<Staged> bufs = {{Q_RAYS, (size_t)(re - rb) * C.width * sizeof(rtg_ray), nullptr, rays}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_camera_rays(C, rb, re, o->sample_begin < 0 ? 0 : o->sample_begin, o->seed,
                                    (rtg_ray*)s->q[Q_RAYS].p, s->stream));
    return unstage(s, bufs);
}

// ---- surface queries (rtg_surface.hip)
// checked in an order that names the argument at fault where the scene is not needed to see it
static int surface_args(const rtg_scene* s, const void* rays, int64_t n, uint32_t flags, const void* out) {
    if (flags & RTG_QUERY_ANY_HIT)
        return set_err(RTG_ERR_INVALID, "surface queries are closest-hit: RTG_QUERY_ANY_HIT in flags 0x%x", flags);
    if (flags & ~(uint32_t)RTG_QUERY_COHERENT) return set_err(RTG_ERR_INVALID, "unknown query flags 0x%x", flags);
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld rays: at most INT32_MAX per call", (long long)n);
    if (n > 0 && (!rays || !out)) return set_err(RTG_ERR_INVALID, "null buffer");
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    return RTG_OK;
}

int rtg_surface_rays_device(rtg_scene* s, const rtg_ray* d_rays, int64_t n, uint32_t flags, rtg_surface* d_out,
                            void* stream) {
    int rc = surface_args(s, d_rays, n, flags, d_out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_surface(s->ds, s->shade_sk, s->feat, d_rays, (int)n, flags, d_out, (hipStream_t)stream));
    return RTG_OK;
}

int rtg_surface_rays(rtg_scene* s, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_surface* out) {
    int rc = surface_args(s, rays, n, flags, out);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_RAYS, N * sizeof(rtg_ray), rays, nullptr},
                                                {Q_SURFACE, N * sizeof(rtg_surface), nullptr, out}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_surface(s->ds, s->shade_sk, s->feat, (rtg_ray*)s->q[Q_RAYS].p, (int)n, flags,
                                (rtg_surface*)s->q[Q_SURFACE].p, s->stream));
    return unstage(s, bufs);
}

// ---- radiance queries (rtg_radiance.hip)
// the camera record and kernel parameters of a radiance batch; host_ids: pixel ids in host memory
static int radiance_args(const rtg_scene* s, const rtg_radiance_opts* o, const void* rays, const int32_t* host_ids,
                         int64_t n, const void* rgbt, rtg::DevCamera& C, rtg::RadianceParams& P) {
    if (!o) return set_err(RTG_ERR_INVALID, "null options");
    if (n < 0 || n > INT32_MAX) return set_err(RTG_ERR_INVALID, "%lld rays: at most INT32_MAX per call", (long long)n);
    if (o->flags & ~(uint32_t)RTG_RADIANCE_CAMERA_EYE) return set_err(RTG_ERR_INVALID, "unknown radiance flags 0x%x", o->flags);
    if (o->first_pixel < 0) return set_err(RTG_ERR_INVALID, "negative first_pixel %d", o->first_pixel);
    if (n > 0 && (!rays || !rgbt)) return set_err(RTG_ERR_INVALID, "null buffer");
    if (!s) return set_err(RTG_ERR_INVALID, "null scene");
    const rtg_camera* c = nullptr;
    if (int rc = scene_camera(s, o->camera, true, c)) return rc;
    if (host_ids)
        for (int64_t i = 0; i < n; ++i)
            if (host_ids[i] < 0) return set_err(RTG_ERR_INVALID, "negative pixel id %d at ray %lld", host_ids[i], (long long)i);
    // the frame stack's depth: rtg_scene_create's own bound, kept with the kernel that relies on it
    if (s->max_depth > rtg::max_supported_depth())
        return set_err(RTG_ERR_UNSUPPORTED, "MaxRecursionDepth %d > %d", s->max_depth, rtg::max_supported_depth());
    dev_camera(*c, C);
    std::memset(&P, 0, sizeof(P));
    P.n = (int)n;
    P.first_pixel = o->first_pixel;
    P.sample_begin = o->sample_begin < 0 ? 0 : o->sample_begin;
    P.sample_count = o->sample_count <= 0 ? 1 : o->sample_count;
    P.camera_eye = (o->flags & RTG_RADIANCE_CAMERA_EYE) ? 1 : 0;
    P.seed = o->seed;
    return RTG_OK;
}

int rtg_radiance_rays_device(rtg_scene* s, const rtg_radiance_opts* o, const rtg_ray* d_rays, const int32_t* d_pixel_ids,
                             int64_t n, float* d_rgbt, void* stream) {
    rtg::DevCamera C;
    rtg::RadianceParams P;
    int rc = radiance_args(s, o, d_rays, nullptr, n, d_rgbt, C, P);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(rtg::launch_radiance(s->ds, C, P, s->shade_sk, s->feat, d_rays, d_pixel_ids, d_rgbt, (hipStream_t)stream));
    return RTG_OK;
}

int rtg_radiance_rays(rtg_scene* s, const rtg_radiance_opts* o, const rtg_ray* rays, const int32_t* pixel_ids, int64_t n,
                      float* rgbt) {
    rtg::DevCamera C;
    rtg::RadianceParams P;
    int rc = radiance_args(s, o, rays, pixel_ids, n, rgbt, C, P);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t N = (size_t)n;
    const std::initializer_list<Staged> bufs = {{Q_RAYS, N * sizeof(rtg_ray), rays, nullptr},
                           {Q_RADIANCE, N * 4 * sizeof(float), nullptr, rgbt},
                           {Q_PIXEL_IDS, pixel_ids ? N * sizeof(int32_t) : 0, pixel_ids, nullptr}};
    if ((rc = stage(s, bufs))) return rc;
    HIP_TRY(rtg::launch_radiance(s->ds, C, P, s->shade_sk, s->feat, (rtg_ray*)s->q[Q_RAYS].p,
                                 pixel_ids ? (int32_t*)s->q[Q_PIXEL_IDS].p : nullptr, (float*)s->q[Q_RADIANCE].p,
                                 s->stream));
    return unstage(s, bufs);
}

int rtg_desc_trace_rays(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags, rtg_hit* hits,
                        float* normals) {
    std::string err;
    int rc;
    try {
        rc = rtg::host_trace_rays(d, rays, n, flags, hits, normals, err);
    } catch (const std::exception& e) {
        return set_err(RTG_ERR_NOMEM, "rtg_desc_trace_rays: %s", e.what());
    }
    return rc == RTG_OK ? RTG_OK : set_err(rc, "%s", err.c_str());
}

int rtg_desc_trace_rays_multi(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, int32_t k, uint32_t flags,
                              rtg_hit* hits, int32_t* counts) {
    std::string err;
    int rc;
    try {
        rc = rtg::host_trace_rays_multi(d, rays, n, k, flags, hits, counts, err);
    } catch (const std::exception& e) {
        return set_err(RTG_ERR_NOMEM, "rtg_desc_trace_rays_multi: %s", e.what());
    }
    return rc == RTG_OK ? RTG_OK : set_err(rc, "%s", err.c_str());
}

int rtg_desc_closest_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, uint32_t flags,
                            rtg_nearest* out) {
    std::string err;
    int rc;
    try {
        rc = rtg::host_closest_points(d, points, n, flags, out, err);
    } catch (const std::exception& e) {
        return set_err(RTG_ERR_NOMEM, "rtg_desc_closest_points: %s", e.what());
    }
    return rc == RTG_OK ? RTG_OK : set_err(rc, "%s", err.c_str());
}

int rtg_desc_count_crossings(const rtg_scene_desc* d, const rtg_ray* rays, int64_t n, uint32_t flags,
                             rtg_crossings* out) {
    std::string err;
    int rc;
    try {
        rc = rtg::host_count_crossings(d, rays, n, flags, out, err);
    } catch (const std::exception& e) {
        return set_err(RTG_ERR_NOMEM, "rtg_desc_count_crossings: %s", e.what());
    }
    return rc == RTG_OK ? RTG_OK : set_err(rc, "%s", err.c_str());
}

int rtg_desc_signed_distance_points(const rtg_scene_desc* d, const rtg_point* points, int64_t n, const float dir[3],
                                    uint32_t flags, rtg_nearest* out) {
    std::string err;
    int rc;
    try {
        rc = rtg::host_signed_distance_points(d, points, n, dir, flags, out, err);
    } catch (const std::exception& e) {
        return set_err(RTG_ERR_NOMEM, "rtg_desc_signed_distance_points: %s", e.what());
    }
    return rc == RTG_OK ? RTG_OK : set_err(rc, "%s", err.c_str());
}

int rtg_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return set_err(RTG_ERR_INVALID, "bad arguments");
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return RTG_OK;
}

int rtg_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return RTG_OK;
}

int rtg_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return set_err(RTG_ERR_INVALID, "bad arguments");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return RTG_OK;
}

int rtg_host_unregister(void* p) {
    if (!p) return set_err(RTG_ERR_INVALID, "null argument");
    HIP_TRY(hipHostUnregister(p));
    return RTG_OK;
}

int rtg_tonemap_device(const float* d_hdr, int32_t w, int32_t h, const rtg_tonemap_params* tp, uint8_t* d_ldr,
                       int32_t device, void* stream) {
    if (!d_hdr || !d_ldr || !tp || w <= 0 || h <= 0) return set_err(RTG_ERR_INVALID, "bad tonemap arguments");
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    void* scratch = nullptr;
    HIP_TRY(hipMallocAsync(&scratch, rtg::tonemap_scratch_bytes((long long)w * h), st));
    hipError_t e = rtg::launch_tonemap(d_hdr, w, h, tp->key, tp->burn_percent, tp->saturation, tp->gamma, d_ldr, scratch, st);
    hipError_t e2 = hipFreeAsync(scratch, st);
    HIP_TRY(e);
    HIP_TRY(e2);
    return RTG_OK;
}

int rtg_tonemap(const float* hdr, int32_t w, int32_t h, const rtg_tonemap_params* tp, uint8_t* ldr, int32_t device) {
    if (!hdr || !ldr || !tp || w <= 0 || h <= 0) return set_err(RTG_ERR_INVALID, "bad tonemap arguments");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)w * h * 3;
    DevBuf<float> dh;
    DevBuf<uint8_t> dl;
    HIP_TRY(dh.alloc(n));
    if (dl.alloc(n) != hipSuccess) return set_err(RTG_ERR_NOMEM, "device allocation failed");
    if (hipMemcpy(dh.p, hdr, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return set_err(RTG_ERR_HIP, "copy failed");
    if (int rc = rtg_tonemap_device(dh.p, w, h, tp, dl.p, device, nullptr)) return rc;
    if (hipMemcpy(ldr, dl.p, n, hipMemcpyDeviceToHost) != hipSuccess) return set_err(RTG_ERR_HIP, "copy failed");
    return RTG_OK;
}

int rtg_tonemap_log_average(const float* hdr, int32_t w, int32_t h, int32_t mode, double* avg_out, int32_t device) {
    if (!hdr || !avg_out || w <= 0 || h <= 0 || mode > 3) return set_err(RTG_ERR_INVALID, "bad log-average arguments");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)w * h;
    DevBuf<float> dh;
    DevBuf<char> scratch;
    HIP_TRY(dh.alloc(3 * n));
    if (scratch.alloc(rtg::tonemap_scratch_bytes((long long)n)) != hipSuccess)
        return set_err(RTG_ERR_NOMEM, "device allocation failed");
    if (hipMemcpy(dh.p, hdr, 3 * n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return set_err(RTG_ERR_HIP, "copy failed");
    rtg::launch_log_average(dh.p, (long long)n, mode, 0, scratch.p, nullptr);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(avg_out, scratch.p + rtg::tonemap_avg_offset(), sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(RTG_ERR_HIP, "log-average failed");
    return RTG_OK;
}

int rtg_resolve_accum(const float* accum, int32_t w, int32_t h, float* hdr, uint8_t* ldr) {
    if (!accum || w <= 0 || h <= 0) return set_err(RTG_ERR_INVALID, "bad accumulation buffer");
    for (size_t p = 0; p < (size_t)w * h; ++p) {
        const float* a = accum + 4 * p;
        for (int k = 0; k < 3; ++k) {
            float c = a[k] / a[3];
            if (hdr) hdr[3 * p + k] = c;
            if (ldr) {
                int i = (c > -2147483904.0f && c < 2147483648.0f) ? (int)c : (int)0x80000000;
                ldr[3 * p + k] = (uint8_t)(i < 0 ? 0 : (i > 255 ? 255 : i));
            }
        }
    }
    return RTG_OK;
}

int rtg_scene_stats(rtg_scene* s, rtg_stats* out) {
    if (!s || !out) return set_err(RTG_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    for (rtg_scene* r : with_replicas(s)) {
        HIP_TRY(hipSetDevice(r->device));
        rtg::DevCounters c;
        HIP_TRY(hipEventSynchronize(r->done));
        HIP_TRY(hipMemcpy(&c, r->counters.p, sizeof(c), hipMemcpyDeviceToHost));
        out->camera_rays += c.camera_rays;
        out->secondary_rays += c.secondary_rays;
        out->shadow_rays += c.shadow_rays;
        out->node_visits += c.node_visits;
        out->tri_tests += c.tri_tests;
        out->sphere_tests += c.sphere_tests;
        out->object_tests += c.object_tests;
        out->shadow_node_visits += c.shadow_node_visits;
        out->shadow_tri_tests += c.shadow_tri_tests;
        out->shadow_wide_visits += c.shadow_wide_visits;
        out->shadow_fallbacks += c.shadow_fallbacks;
        out->extend_wide_visits += c.extend_wide_visits;
        out->extend_fallbacks += c.extend_fallbacks;
    }
    return RTG_OK;
}

int rtg_scene_reset_stats(rtg_scene* s) {
    if (!s) return set_err(RTG_ERR_INVALID, "null argument");
    for (rtg_scene* r : with_replicas(s)) {
        HIP_TRY(hipSetDevice(r->device));
        HIP_TRY(hipEventSynchronize(r->done));
        // on the scene's (non-blocking) stream, complete before return: ordered before the
        // next render whichever stream that one runs on
        HIP_TRY(hipMemsetAsync(r->counters.p, 0, sizeof(rtg::DevCounters), r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));
    }
    return RTG_OK;
}

int rtg_scene_timings(rtg_scene* s, float* ms, const char** names, int32_t cap, int32_t* count) {
    // stage names per layout (rtg_kernels.hpp LAYOUT_*)
    static const char* kNames[7][rtg::MAX_STAGES] = {{"k_primary", "k_shade", "k_shadow", "k_resolve"},
                                                     {"k_primary", "k_shade", "k_shadow"},
                                                     {"k_primary", "k_shade_shadow"},
                                                     {"tree_levels", "tree_resolve"},
                                                     {"k_render"},
                                                     {"path_iterations"},
                                                     {"k_frame"}};
    static const int kCount[7] = {rtg::WAVE_STAGES, 3, 2, rtg::TREE_STAGES, rtg::MEGA_STAGES, rtg::PATH_STAGES, 1};
    if (!s || !count) return set_err(RTG_ERR_INVALID, "null argument");
    if (s->timed_layout < 0) return set_err(RTG_ERR_INVALID, "no render was issued with RTG_RENDER_TIMING");
    HIP_TRY(hipSetDevice(s->device));
    const int n = kCount[s->timed_layout];
    HIP_TRY(hipEventSynchronize(s->ev[n]));
    const char* const* nm = kNames[s->timed_layout];
    for (int k = 0; k < n && k < cap; ++k) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, s->ev[k], s->ev[k + 1]));
        if (ms) ms[k] = t;
        if (names) names[k] = nm[k];
    }
    *count = n;
    return RTG_OK;
}

int rtg_scene_timed_samples(const rtg_scene* s, int32_t* samples) {
    if (!s || !samples) return set_err(RTG_ERR_INVALID, "null argument");
    if (s->timed_layout < 0) return set_err(RTG_ERR_INVALID, "no render was issued with RTG_RENDER_TIMING");
    *samples = s->timed_samples;
    return RTG_OK;
}

int rtg_write_png(const char* path, int32_t w, int32_t h, const uint8_t* rgb) {
    std::string err;
    if (!path || !rgb || w <= 0 || h <= 0) return set_err(RTG_ERR_INVALID, "bad arguments");
    if (!rtg::write_png(path, w, h, rgb, err)) return set_err(RTG_ERR_IO, "%s", err.c_str());
    return RTG_OK;
}

int rtg_write_hdr(const char* path, int32_t w, int32_t h, const float* rgb) {
    std::string err;
    if (!path || !rgb || w <= 0 || h <= 0) return set_err(RTG_ERR_INVALID, "bad arguments");
    if (!rtg::write_hdr(path, w, h, rgb, err)) return set_err(RTG_ERR_IO, "%s", err.c_str());
    return RTG_OK;
}

}  // extern "C"

extern "C" int rtg_desc_anyhit_check(const rtg_scene_desc* d, int32_t mode, int64_t* out, int32_t n_out) {
    if (!d || !out || n_out < 8 || mode < 0 || mode > 2) return set_err(RTG_ERR_INVALID, "bad argument");
    if (d->num_faces > 0 && d->num_nodes == 0) return set_err(RTG_ERR_INVALID, "description without a BVH");
    try {
        std::string err;
        int rc = rtg::validate_desc(d, err);
        rtg::TableOptions opt;
        opt.ahb_mode = (rtg::AhbMode)mode;
        rtg::SceneTables T;
        if (!rc) rc = rtg::build_scene_tables(d, opt, nullptr, T, err);
        if (rc) return set_err(rc, "%s", err.c_str());
        const bool ok = T.ahb_ok;
        long long bad = 0;
        for (int m = 0; m < d->num_meshes && ok; ++m)
            bad += rtg::ahb_validate(T.anodes, T.ahtris, T.aroot[m], T.nodes, T.node_ext, T.mesh_begin[m], T.mesh_end[m],
                                     T.tris.data());
        const int64_t v[8] = {T.ahb.nodes, T.ahb.entries, T.ahb.max_depth, T.ahb.leaf_prims, T.ahb.face_prims,
                              T.ahb.exact_faces, bad, ok ? 1 : 0};
        for (int k = 0; k < 8; ++k) out[k] = v[k];
    } catch (const std::bad_alloc&) {
        return set_err(RTG_ERR_NOMEM, "out of memory");
    }
    return RTG_OK;
}
