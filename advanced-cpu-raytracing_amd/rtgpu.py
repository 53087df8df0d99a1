"""ctypes binding of the rtgpu C-ABI (include/rtgpu.h).

Mirrors the reference's render interface for Python callers (tests, bench.py):

* ``HostScene(xml)``          -- ``DorkTracer::Scene::loadFromXml`` (src/parser.cpp:26-577)
* ``DeviceScene(host, dev)``  -- ``Raytracer::Raytracer(Scene&)`` (src/raytracer.cpp:7-16),
                                 a device-resident replica on HIP device ``dev``
* ``DeviceScene.render(cam)`` -- the per-camera block of ``main()`` (src/main.cpp:142-196):
                                 every pixel through ``RenderPixel`` (raytracer.hpp:19),
                                 returning the float image (main.cpp:114-116) and the
                                 ``clamp((int)c)`` LDR image (main.cpp:121)

The product path is librtgpu.so only; importing this module fails loudly when the
library has not been built.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RTGPU_LIB: an alternative in-tree build of the same library (A/B kernel experiments)
LIB_PATH = os.environ.get("RTGPU_LIB") or os.path.join(HERE, "librtgpu.so")

RTG_RENDER_COUNT_STATS = 1
RTG_RENDER_ACCUM_ONLY = 2
RTG_RENDER_FUSED = 4
RTG_RENDER_TIMING = 8
RTG_RENDER_TREE = 16
RTG_RENDER_EXACT_SHADOW = 32
RTG_RENDER_ORDERED = 64
RTG_RENDER_SAMPLE_PASSES = 128
RTG_LOAD_DEVICE_BVH = 1
RTG_QUERY_ANY_HIT = 1
RTG_QUERY_COHERENT = 2
RTG_MULTIHIT_MAX = 8
RTG_RADIANCE_CAMERA_EYE = 1
# rtg_ray (32 B) and rtg_hit (16 B) as NumPy structured dtypes
RAY_DTYPE = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("tmax", "<f4"),
                      ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("time", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("object", "<i4"), ("face", "<i4"), ("pad", "<i4")])
# rtg_surface (64 B): hit, shading normal + u, geometric normal + v, diffuse coefficient
SURFACE_DTYPE = np.dtype([("t", "<f4"), ("object", "<i4"), ("face", "<i4"), ("material", "<i4"),
                          ("n", "<f4", (3,)), ("u", "<f4"), ("ng", "<f4", (3,)), ("v", "<f4"),
                          ("kd", "<f4", (3,)), ("pad", "<f4")])
# rtg_point (16 B) and rtg_nearest (32 B) of the closest-point queries
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("max_dist", "<f4")])
NEAREST_DTYPE = np.dtype([("dist", "<f4"), ("object", "<i4"), ("face", "<i4"), ("pad0", "<i4"),
                          ("p", "<f4", (3,)), ("pad1", "<f4")])
# rtg_crossings (8 B) of the crossing-count queries
CROSSINGS_DTYPE = np.dtype([("count", "<i4"), ("entering", "<i4")])
# the direction rtg_signed_distance_points* walks along when given none (rtgpu.h)
SDF_DEFAULT_DIRECTION = (0.8213, 0.4402, 0.3628)
RTG_CAMERA_SIZE = 392   # sizeof(rtg_camera), checked against the C compiler by tests/test_abi.py


class RTGError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtgpu error {code}: {msg}")
        self.code = code


class TonemapParams(ctypes.Structure):
    _fields_ = [("key", ctypes.c_float), ("burn_percent", ctypes.c_float), ("saturation", ctypes.c_float),
                ("gamma", ctypes.c_float)]


class _Camera(ctypes.Structure):
    """Head of rtg_camera (include/rtgpu.h) up to the tonemapper parameters."""
    _fields_ = [("f3", ctypes.c_float * 15), ("ext", ctypes.c_float * 5), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("spp", ctypes.c_int32), ("focus_distance", ctypes.c_float),
                ("aperture", ctypes.c_float), ("has_tonemapper", ctypes.c_int32), ("tm_key", ctypes.c_float),
                ("tm_burn", ctypes.c_float), ("tm_saturation", ctypes.c_float), ("tm_gamma", ctypes.c_float)]


class CameraView(ctypes.Structure):
    """rtg_camera_view (72 B): what a <Camera> element states about the view."""
    _fields_ = [("position", ctypes.c_float * 3), ("gaze", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("look_at", ctypes.c_int32), ("near_plane", ctypes.c_float * 4), ("fov_y", ctypes.c_float),
                ("near_dist", ctypes.c_float), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class Camera:
    """One rtg_camera by value (RTG_CAMERA_SIZE bytes): what HostScene.camera_record() and
    camera_setup() return and DeviceScene.set_camera() takes."""

    def __init__(self, raw: bytes = b""):
        self.buf = ctypes.create_string_buffer(bytes(raw).ljust(RTG_CAMERA_SIZE, b"\0"), RTG_CAMERA_SIZE)

    @property
    def head(self) -> "_Camera":
        return _Camera.from_buffer(self.buf)

    @property
    def width(self) -> int:
        return self.head.width

    @property
    def height(self) -> int:
        return self.head.height

    def view_bytes(self) -> bytes:
        """The fields rtg_camera_setup fills: position .. q, the extents and near distance, the size."""
        return self.buf.raw[:88]

    def copy(self) -> "Camera":
        return Camera(self.buf.raw)


def camera_setup(position, gaze, up, near_dist, width, height, near_plane=None, fov_y=None, base: Camera = None) -> Camera:
    """rtg_camera_setup (host only): the camera of a view.  ``fov_y`` (degrees) selects the lookAt
    form, where ``gaze`` is the gaze point; otherwise ``gaze`` is a direction and ``near_plane`` =
    (left, right, bottom, top).  ``base``: the camera whose other fields (samples, lens,
    tonemapper, renderer flags) the result keeps; default a one-sample camera."""
    v = CameraView()
    v.position[:], v.gaze[:], v.up[:] = position, gaze, up
    v.look_at = 1 if fov_y is not None else 0
    if near_plane is not None:
        v.near_plane[:] = near_plane
    v.fov_y = fov_y if fov_y is not None else 0.0
    v.near_dist, v.width, v.height = near_dist, width, height
    cam = base.copy() if base is not None else Camera()
    if base is None:
        cam.head.spp = 1
    _check(lib().rtg_camera_setup(ctypes.byref(v), ctypes.addressof(cam.buf)))
    return cam


class _DescHead(ctypes.Structure):
    """Head of rtg_scene_desc (include/rtgpu.h) up to the camera list."""
    _fields_ = [("background", ctypes.c_int32 * 3), ("shadow_epsilon", ctypes.c_float),
                ("max_recursion_depth", ctypes.c_int32), ("bg_texture", ctypes.c_int32),
                ("ambient_light", ctypes.c_float * 3), ("cameras", ctypes.c_void_p), ("num_cameras", ctypes.c_int32)]


class RenderOpts(ctypes.Structure):
    _fields_ = [
        ("camera", ctypes.c_int32),
        ("sample_begin", ctypes.c_int32),
        ("sample_count", ctypes.c_int32),
        ("row_begin", ctypes.c_int32),
        ("row_end", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("part_index", ctypes.c_int32),
        ("part_count", ctypes.c_int32),
    ]


class RadianceOpts(ctypes.Structure):
    """rtg_radiance_opts (32 B)."""
    _fields_ = [
        ("camera", ctypes.c_int32),
        ("sample_begin", ctypes.c_int32),
        ("sample_count", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
        ("first_pixel", ctypes.c_int32),
        ("pad0", ctypes.c_int32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "camera_rays", "secondary_rays", "shadow_rays", "node_visits", "tri_tests",
        "sphere_tests", "object_tests", "shadow_node_visits", "shadow_tri_tests", "shadow_wide_visits",
        "shadow_fallbacks", "extend_wide_visits", "extend_fallbacks")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# every symbol include/rtgpu.h declares
EXPORTED = [
    "rtg_host_scene_load_xml", "rtg_host_scene_load_xml_ex", "rtg_host_scene_desc", "rtg_host_scene_free",
    "rtg_scene_export_bvh",
    "rtg_desc_camera_info", "rtg_desc_counts", "rtg_desc_anyhit_check", "rtg_scene_create", "rtg_scene_destroy",
    "rtg_device_count", "rtg_render", "rtg_render_device", "rtg_resolve_accum",
    "rtg_scene_stats", "rtg_scene_reset_stats", "rtg_scene_timings", "rtg_scene_timed_samples", "rtg_tonemap_device", "rtg_tonemap",
    "rtg_tonemap_log_average",
    "rtg_write_png", "rtg_write_hdr",
    "rtg_last_error", "rtg_abi_version",
    "rtg_scene_create_multi", "rtg_scene_num_devices", "rtg_part_runs", "rtg_copy_part_to_host",
    "rtg_host_alloc", "rtg_host_free", "rtg_host_register", "rtg_host_unregister",
    "rtg_trace_rays_device", "rtg_trace_rays", "rtg_camera_rays_device", "rtg_camera_rays", "rtg_desc_trace_rays",
    "rtg_trace_rays_multi_device", "rtg_trace_rays_multi", "rtg_desc_trace_rays_multi",
    "rtg_closest_points_device", "rtg_closest_points", "rtg_desc_closest_points",
    "rtg_count_crossings_device", "rtg_count_crossings", "rtg_desc_count_crossings",
    "rtg_signed_distance_points_device", "rtg_signed_distance_points", "rtg_desc_signed_distance_points",
    "rtg_radiance_rays_device", "rtg_radiance_rays",
    "rtg_surface_rays_device", "rtg_surface_rays",
    "rtg_scene_update", "rtg_scene_set_camera", "rtg_scene_num_cameras", "rtg_camera_setup",
    "rtg_scene_clone", "rtg_scene_shares_geometry",
]

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RTGError(-1, f"{LIB_PATH} not built: run `make -C {HERE}` (or __graft_entry__.build())")
    # One HIP runtime per process: torch's ROCm wheel ships its own libamdhip64.so.7.  If
    # torch is loaded first, librtgpu's NEEDED libamdhip64.so.7 binds to that same copy
    # (shared streams, events, allocations); loaded the other way round, two runtimes
    # end up in the process and torch's fails to initialise.  So load torch first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, P = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER
    L.rtg_last_error.restype = ctypes.c_char_p
    L.rtg_abi_version.restype = ctypes.c_int
    L.rtg_host_scene_load_xml.argtypes = [ctypes.c_char_p, P(vp)]
    L.rtg_host_scene_load_xml_ex.argtypes = [ctypes.c_char_p, ctypes.c_uint32, P(vp)]
    L.rtg_scene_export_bvh.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, P(ctypes.c_int64),
                                       P(ctypes.c_int64)]
    L.rtg_host_scene_desc.argtypes = [vp]
    L.rtg_host_scene_desc.restype = vp
    L.rtg_host_scene_free.argtypes = [vp]
    L.rtg_host_scene_free.restype = None
    L.rtg_desc_camera_info.argtypes = [vp, ctypes.c_int, P(i32), P(i32), P(i32), P(i32)]
    L.rtg_desc_counts.argtypes = [vp] + [P(ctypes.c_int64)] * 4
    L.rtg_desc_anyhit_check.argtypes = [vp, i32, P(ctypes.c_int64), i32]
    L.rtg_scene_create.argtypes = [vp, ctypes.c_int, P(vp)]
    L.rtg_scene_destroy.argtypes = [vp]
    L.rtg_scene_destroy.restype = None
    L.rtg_device_count.argtypes = [P(i32)]
    L.rtg_render.argtypes = [vp, P(RenderOpts), vp, vp]
    L.rtg_render_device.argtypes = [vp, P(RenderOpts), vp, vp, vp, vp]
    L.rtg_resolve_accum.argtypes = [vp, i32, i32, vp, vp]
    L.rtg_scene_stats.argtypes = [vp, P(Stats)]
    L.rtg_scene_reset_stats.argtypes = [vp]
    L.rtg_scene_timings.argtypes = [vp, P(ctypes.c_float), P(ctypes.c_char_p), i32, P(i32)]
    L.rtg_scene_timed_samples.argtypes = [vp, P(i32)]
    L.rtg_tonemap_device.argtypes = [vp, i32, i32, P(TonemapParams), vp, i32, vp]
    L.rtg_tonemap.argtypes = [vp, i32, i32, P(TonemapParams), vp, i32]
    L.rtg_tonemap_log_average.argtypes = [vp, i32, i32, i32, P(ctypes.c_double), i32]
    L.rtg_write_png.argtypes = [ctypes.c_char_p, i32, i32, vp]
    L.rtg_write_hdr.argtypes = [ctypes.c_char_p, i32, i32, vp]
    L.rtg_scene_create_multi.argtypes = [vp, P(i32), i32, P(vp)]
    L.rtg_scene_num_devices.argtypes = [vp, P(i32)]
    L.rtg_part_runs.argtypes = [i32, i32, i32, i32, vp, i32, P(i32)]
    L.rtg_copy_part_to_host.argtypes = [vp, P(RenderOpts), vp, vp, vp, vp, vp]
    L.rtg_host_alloc.argtypes = [ctypes.c_size_t, P(vp)]
    L.rtg_host_free.argtypes = [vp]
    L.rtg_host_register.argtypes = [vp, ctypes.c_size_t]
    L.rtg_host_unregister.argtypes = [vp]
    L.rtg_trace_rays_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp, vp]
    L.rtg_trace_rays.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp]
    L.rtg_camera_rays_device.argtypes = [vp, P(RenderOpts), vp, vp]
    L.rtg_camera_rays.argtypes = [vp, P(RenderOpts), vp]
    L.rtg_desc_trace_rays.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp]
    L.rtg_trace_rays_multi_device.argtypes = [vp, vp, ctypes.c_int64, i32, ctypes.c_uint32, vp, vp, vp]
    L.rtg_trace_rays_multi.argtypes = [vp, vp, ctypes.c_int64, i32, ctypes.c_uint32, vp, vp]
    L.rtg_desc_trace_rays_multi.argtypes = [vp, vp, ctypes.c_int64, i32, ctypes.c_uint32, vp, vp]
    L.rtg_closest_points_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp]
    L.rtg_closest_points.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp]
    L.rtg_desc_closest_points.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp]
    L.rtg_count_crossings_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp]
    L.rtg_count_crossings.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp]
    L.rtg_desc_count_crossings.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp]
    L.rtg_signed_distance_points_device.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_uint32, vp, vp]
    L.rtg_signed_distance_points.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_uint32, vp]
    L.rtg_desc_signed_distance_points.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_uint32, vp]
    L.rtg_radiance_rays_device.argtypes =[vp, P(RadianceOpts), vp, vp, ctypes.c_int64, vp, vp]
    L.rtg_radiance_rays.argtypes = [vp, P(RadianceOpts), vp, vp, ctypes.c_int64, vp]
    L.rtg_surface_rays_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp, vp]
    L.rtg_surface_rays.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_uint32, vp]
    L.rtg_scene_update.argtypes = [vp, vp, vp]
    L.rtg_scene_set_camera.argtypes = [vp, i32, vp]
    L.rtg_scene_num_cameras.argtypes = [vp, P(i32)]
    L.rtg_camera_setup.argtypes = [P(CameraView), vp]
    L.rtg_scene_clone.argtypes = [vp, P(vp)]
    L.rtg_scene_shares_geometry.argtypes = [vp, vp, P(i32)]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise RTGError(rc, lib().rtg_last_error().decode(errors="replace"))


def make_rays(origins, directions, tmax=np.inf, time=0.0) -> np.ndarray:
    """(n, 3) origins and directions (+ scalar or (n,) tmax / time) -> RAY_DTYPE array."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = o[:, 0], o[:, 1], o[:, 2]
    rays["dx"], rays["dy"], rays["dz"] = d[:, 0], d[:, 1], d[:, 2]
    rays["tmax"] = tmax
    rays["time"] = time
    return rays


def _query_flags(any_hit: bool, coherent: bool) -> int:
    return (RTG_QUERY_ANY_HIT if any_hit else 0) | (RTG_QUERY_COHERENT if coherent else 0)


def _query(fn, handle, rays, any_hit, coherent, normals):
    """Shared body of HostScene.trace / DeviceScene.trace: hits, or (hits, normals (n, 4))."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = rays.size
    hits = np.zeros(n, HIT_DTYPE)
    nrm = np.zeros((n, 4), np.float32) if normals else None
    _check(fn(handle, rays.ctypes.data, n, _query_flags(any_hit, coherent), hits.ctypes.data,
              nrm.ctypes.data if normals else None))
    return (hits, nrm) if normals else hits


def _query_multi(fn, handle, rays, k, coherent, counts):
    """Shared body of HostScene.trace_multi / DeviceScene.trace_multi: (n, k) hits, or (hits, counts)."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    n = rays.size
    k = int(k)
    hits = np.zeros((n, max(k, 0)), HIT_DTYPE)
    cnt = np.zeros(n, np.int32) if counts else None
    _check(fn(handle, rays.ctypes.data, n, k, _query_flags(False, coherent), hits.ctypes.data,
              cnt.ctypes.data if counts else None))
    return (hits, cnt) if counts else hits


def make_points(xyz, max_dist=np.inf) -> np.ndarray:
    """(n, 3) points (+ scalar or (n,) max_dist) -> POINT_DTYPE array."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    pts = np.zeros(len(p), POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = p[:, 0], p[:, 1], p[:, 2]
    pts["max_dist"] = max_dist
    return pts


def _query_closest(fn, handle, points):
    """Shared body of HostScene.closest / DeviceScene.closest."""
    points = np.ascontiguousarray(points, POINT_DTYPE)
    out = np.zeros(points.size, NEAREST_DTYPE)
    _check(fn(handle, points.ctypes.data, points.size, 0, out.ctypes.data))
    return out


def _query_crossings(fn, handle, rays, coherent):
    """Shared body of HostScene.crossings / DeviceScene.crossings."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    out = np.zeros(rays.size, CROSSINGS_DTYPE)
    _check(fn(handle, rays.ctypes.data, rays.size, _query_flags(False, coherent), out.ctypes.data))
    return out


def _direction(direction):
    """None (the library's default), or three float32 the call keeps alive."""
    return None if direction is None else np.ascontiguousarray(direction, np.float32).reshape(3)


def _query_signed_distance(fn, handle, points, direction):
    """Shared body of HostScene.signed_distance / DeviceScene.signed_distance."""
    points = np.ascontiguousarray(points, POINT_DTYPE)
    out = np.zeros(points.size, NEAREST_DTYPE)
    d = _direction(direction)
    _check(fn(handle, points.ctypes.data, points.size, None if d is None else d.ctypes.data, 0, out.ctypes.data))
    return out


def device_count() -> int:
    n = ctypes.c_int32()
    _check(lib().rtg_device_count(ctypes.byref(n)))
    return n.value


class HostScene:
    """Parsed + flattened scene (rtg_host_scene).  Paths inside the XML resolve like the
    reference's: PLY relative to the current directory, images as ``inputs/<name>``."""

    def __init__(self, xml_path: str, device_bvh: bool = False):
        """device_bvh: RTG_LOAD_DEVICE_BVH -- no host BVH build; DeviceScene builds it on the GPU."""
        h = ctypes.c_void_p()
        _check(lib().rtg_host_scene_load_xml_ex(os.fsencode(xml_path), RTG_LOAD_DEVICE_BVH if device_bvh else 0,
                                                ctypes.byref(h)))
        self._h = h
        self.desc = lib().rtg_host_scene_desc(h)

    def camera(self, idx: int = 0) -> dict:
        w, h, s, t = (ctypes.c_int32() for _ in range(4))
        _check(lib().rtg_desc_camera_info(self.desc, idx, ctypes.byref(w), ctypes.byref(h),
                                          ctypes.byref(s), ctypes.byref(t)))
        return {"width": w.value, "height": h.value, "spp": s.value, "tonemapped": bool(t.value)}

    def tonemap_params(self, idx: int = 0):
        """(key, burn %, saturation, gamma) of camera idx's <Tonemap> (tonemapper.h:18-25), or
        None for a camera without one."""
        head = _DescHead.from_address(self.desc)
        if not 0 <= idx < head.num_cameras:
            raise RTGError(-1, "camera index out of range")
        cam = _Camera.from_address(head.cameras + idx * RTG_CAMERA_SIZE)
        if not cam.has_tonemapper:
            return None
        return (cam.tm_key, cam.tm_burn, cam.tm_saturation, cam.tm_gamma)

    def camera_record(self, idx: int = 0) -> Camera:
        """Camera idx's rtg_camera by value (for DeviceScene.set_camera, or as camera_setup's base)."""
        head = _DescHead.from_address(self.desc)
        if not 0 <= idx < head.num_cameras:
            raise RTGError(-1, "camera index out of range")
        return Camera(ctypes.string_at(head.cameras + idx * RTG_CAMERA_SIZE, RTG_CAMERA_SIZE))

    def counts(self) -> dict:
        v = [ctypes.c_int64() for _ in range(4)]
        _check(lib().rtg_desc_counts(self.desc, *[ctypes.byref(x) for x in v]))
        return dict(zip(("objects", "faces", "nodes", "lights"), (x.value for x in v)))

    def anyhit_check(self, mode: int = 1) -> dict:
        """Host-only build + structural check of the shadow rays' any-hit trees
        (rtg_desc_anyhit_check; mode 0 reference collapse, 1 SAH over leaves (default), 2 split)."""
        out = (ctypes.c_int64 * 8)()
        _check(lib().rtg_desc_anyhit_check(self.desc, mode, out, 8))
        keys = ("nodes", "entries", "depth", "leaf_prims", "face_prims", "exact_faces", "violations", "built")
        return dict(zip(keys, (int(x) for x in out)))

    def trace(self, rays, any_hit: bool = False, coherent: bool = False, normals: bool = False):
        """Ray queries on the host, no device (rtg_desc_trace_rays: the reference's object loop
        restated plainly -- the yardstick of DeviceScene.trace).  rays: RAY_DTYPE array.  Returns
        the HIT_DTYPE array, or (hits, normals (n, 4) float32) with ``normals=True``."""
        return _query(lib().rtg_desc_trace_rays, self.desc, rays, any_hit, coherent, normals)

    def trace_multi(self, rays, k: int, coherent: bool = False, counts: bool = False):
        """The k nearest hits along each ray on the host, no device (rtg_desc_trace_rays_multi: the
        yardstick of DeviceScene.trace_multi).  Returns the (n, k) HIT_DTYPE array, or
        (hits, counts (n,) int32) with ``counts=True``."""
        return _query_multi(lib().rtg_desc_trace_rays_multi, self.desc, rays, k, coherent, counts)

    def closest(self, points):
        """The nearest surface point to each POINT_DTYPE point on the host, no device
        (rtg_desc_closest_points: the walk that defines the query, the yardstick of
        DeviceScene.closest).  Returns the NEAREST_DTYPE array."""
        return _query_closest(lib().rtg_desc_closest_points, self.desc, points)

    def crossings(self, rays):
        """How many surfaces each ray meets with 0 < t < tmax, and at how many of them it enters, on
        the host, no device (rtg_desc_count_crossings: the walk that defines the query, the
        yardstick of DeviceScene.crossings).  Returns the CROSSINGS_DTYPE array."""
        return _query_crossings(lib().rtg_desc_count_crossings, self.desc, rays, False)

    def signed_distance(self, points, direction=None):
        """closest() with the distance signed by the parity of the surfaces crossed from the point
        along ``direction`` (three floats; None: the library's default), on the host, no device
        (rtg_desc_signed_distance_points: the yardstick of DeviceScene.signed_distance).  ``pad0``
        carries the crossing count."""
        return _query_signed_distance(lib().rtg_desc_signed_distance_points, self.desc, points, direction)

    def num_cameras(self) -> int:
        n = 0
        while True:
            try:
                self.camera(n)
            except RTGError:
                return n
            n += 1

    def close(self):
        if getattr(self, "_h", None):
            lib().rtg_host_scene_free(self._h)
            self._h = None
            self.desc = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: ctypes may already be torn down
            pass


class DeviceScene:
    """Device-resident scene replica (rtg_scene) on HIP device ``device``, or -- with
    ``devices=[d0, d1, ...]`` -- one replica per listed device (rtg_scene_create_multi),
    among which ``render()`` deals the frame's parts (multigpu.py)."""

    def __init__(self, host: HostScene, device: int = 0, devices=None):
        s = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int32 * len(devices))(*devices)
            _check(lib().rtg_scene_create_multi(host.desc, arr, len(devices), ctypes.byref(s)))
            device = devices[0]
        else:
            _check(lib().rtg_scene_create(host.desc, device, ctypes.byref(s)))
        self._s = s
        self.host = host
        self.device = device
        self.devices = list(devices) if devices else [device]
        self._cams = {}     # cameras set by set_camera since the last update: index -> size

    def _camera(self, idx: int) -> dict:
        """Width and height of the scene's camera idx: set_camera's, else the description's."""
        return self._cams[idx] if idx in self._cams else self.host.camera(idx)

    def update(self, host: HostScene, stream: int = 0):
        """rtg_scene_update: every non-geometric part of the scene -- cameras, lights, materials,
        textures' records, object transforms, the global scalars -- replaced in place by
        ``host``'s, over the geometry as uploaded; afterwards every render and query answers bit
        for bit as a scene freshly created from ``host``.  ``host`` must describe the same
        geometry (meshes, face and node ranges, object kinds, images' sizes, mesh lights'
        objects), else RTGError -1 and nothing changes; -6 for a map that needs a table the scene
        was created without, or split any-hit trees.  The copies are enqueued on ``stream``
        (0 = default): work enqueued there before sees the old scene, work after it the new one."""
        _check(lib().rtg_scene_update(self._s, host.desc, stream or None))
        self.host = host
        self._cams = {}

    def set_camera(self, index: int, cam: Camera):
        """rtg_scene_set_camera: replace camera ``index`` (``index == num_cameras()`` appends) by
        ``cam`` (HostScene.camera_record / camera_setup).  No device memory is touched."""
        _check(lib().rtg_scene_set_camera(self._s, index, ctypes.addressof(cam.buf)))
        self._cams[index] = {"width": cam.width, "height": cam.height, "spp": cam.head.spp,
                             "tonemapped": bool(cam.head.has_tonemapper)}

    def num_cameras(self) -> int:
        n = ctypes.c_int32()
        _check(lib().rtg_scene_num_cameras(self._s, ctypes.byref(n)))
        return n.value

    def clone(self) -> "DeviceScene":
        """rtg_scene_clone: a second scene on the same device that shares this one's geometry
        buffers and owns what update() writes -- one clone per frame in flight.  Either may be
        closed first."""
        s = ctypes.c_void_p()
        _check(lib().rtg_scene_clone(self._s, ctypes.byref(s)))
        c = DeviceScene.__new__(DeviceScene)
        c._s, c.host, c.device, c.devices, c._cams = s, self.host, self.device, [self.device], dict(self._cams)
        return c

    def shares_geometry(self, other: "DeviceScene") -> bool:
        yes = ctypes.c_int32()
        _check(lib().rtg_scene_shares_geometry(self._s, other._s, ctypes.byref(yes)))
        return bool(yes.value)

    @staticmethod
    def opts(camera=0, sample_begin=0, sample_count=-1, rows=(0, 0), flags=0, seed=0x5EED, part=(0, 1)) -> RenderOpts:
        return RenderOpts(camera, sample_begin, sample_count, rows[0], rows[1], flags, seed, part[0], part[1])

    def render(self, camera: int = 0, rows=(0, 0), flags: int = 0, seed: int = 0x5EED, part=(0, 1), out=None):
        """Host-buffer render of one camera -> (hdr float32 HxWx3, ldr uint8 HxWx3).  With
        ``part=(i, n)`` only part i's rows are rendered and written (zeros elsewhere, or
        what ``out=(hdr, ldr)`` already holds)."""
        c = self._camera(camera)
        if out is None:
            hdr = np.zeros((c["height"], c["width"], 3), np.float32)
            ldr = np.zeros((c["height"], c["width"], 3), np.uint8)
        else:
            hdr, ldr = out
        o = self.opts(camera, 0, -1, rows, flags, seed, part)
        _check(lib().rtg_render(self._s, ctypes.byref(o), hdr.ctypes.data if hdr is not None else None,
                                ldr.ctypes.data if ldr is not None else None))
        return hdr, ldr

    def render_device(self, hdr_ptr: int, ldr_ptr: int, stream: int = 0, camera: int = 0, flags: int = 0,
                      seed: int = 0x5EED, accum_ptr: int = 0, sample_begin: int = 0, sample_count: int = -1,
                      rows=(0, 0), part=(0, 1)):
        """Asynchronous render into device buffers (e.g. torch tensor data_ptr()s) on ``stream``;
        ``part=(i, n)``: part i of n of the frame (multigpu.py)."""
        o = self.opts(camera, sample_begin, sample_count, rows, flags, seed, part)
        _check(lib().rtg_render_device(self._s, ctypes.byref(o), hdr_ptr or None, ldr_ptr or None,
                                       accum_ptr or None, stream or None))

    def copy_part_to_host(self, d_hdr: int, d_ldr: int, h_hdr: int, h_ldr: int, stream: int = 0, camera: int = 0,
                          rows=(0, 0), part=(0, 1)):
        """Enqueue the DMA of part ``part``'s rows from full-frame device buffers to the same
        offsets of full-frame host buffers (the host framebuffer gather)."""
        o = self.opts(camera, 0, -1, rows, 0, 0, part)
        _check(lib().rtg_copy_part_to_host(self._s, ctypes.byref(o), d_hdr or None, d_ldr or None, h_hdr or None,
                                           h_ldr or None, stream or None))

    def trace(self, rays, any_hit: bool = False, coherent: bool = False, normals: bool = False):
        """Ray queries on host arrays (rtg_trace_rays; synchronous).  rays: RAY_DTYPE array.
        Closest hit: t / object / face per ray (a miss: object = face = -1, t = tmax); with
        ``any_hit`` occlusion (object 0 / -1; emissive meshes skipped, time ignored).
        ``coherent`` is a performance hint (64 consecutive rays are similar), never a different
        answer.  Returns the HIT_DTYPE array, or (hits, normals (n, 4) float32) with
        ``normals=True`` (world-space unit geometric normals; zeros for a miss)."""
        return _query(lib().rtg_trace_rays, self._s, rays, any_hit, coherent, normals)

    def trace_device(self, rays_ptr: int, n: int, hits_ptr: int, normals_ptr: int = 0, stream: int = 0,
                     flags: int = 0):
        """Asynchronous ray queries on device buffers (e.g. torch tensor data_ptr()s: n x 32 B
        rays, n x 16 B hits, optionally n x 4 float32 normals) on ``stream``; flags RTG_QUERY_*."""
        _check(lib().rtg_trace_rays_device(self._s, rays_ptr or None, n, flags, hits_ptr or None,
                                           normals_ptr or None, stream or None))

    def trace_multi(self, rays, k: int, coherent: bool = False, counts: bool = False):
        """The k nearest hits along each ray, in order, on host arrays (rtg_trace_rays_multi;
        synchronous): an (n, k) HIT_DTYPE array -- filled slots first in ascending t, unfilled ones
        the miss record -- or (hits, counts (n,) int32) with ``counts=True``.  A sphere gives both
        of its roots (face -1, then -2).  k in [1, RTG_MULTIHIT_MAX]; k = 1 is trace()."""
        return _query_multi(lib().rtg_trace_rays_multi, self._s, rays, k, coherent, counts)

    def trace_multi_device(self, rays_ptr: int, n: int, k: int, hits_ptr: int, counts_ptr: int = 0, stream: int = 0,
                           flags: int = 0):
        """Asynchronous multi-hit queries on device buffers (n x 32 B rays, n x k x 16 B hits
        ray-major, optionally n int32 counts) on ``stream``; flags RTG_QUERY_COHERENT or 0."""
        _check(lib().rtg_trace_rays_multi_device(self._s, rays_ptr or None, n, k, flags, hits_ptr or None,
                                                 counts_ptr or None, stream or None))

    def closest(self, points):
        """The nearest point of the scene's surface to each POINT_DTYPE point (make_points), on host
        arrays (rtg_closest_points; synchronous): a NEAREST_DTYPE array with the world-space
        distance, the object and global face (-1: a sphere) and the closest point ``p``.  Nothing
        strictly nearer than ``max_dist``, or a point that is not finite: dist = max_dist,
        object = face = -1, p = 0."""
        return _query_closest(lib().rtg_closest_points, self._s, points)

    def closest_device(self, points_ptr: int, n: int, out_ptr: int, stream: int = 0):
        """Asynchronous closest-point queries on device buffers (n x 16 B points, n x 32 B results)
        on ``stream`` (rtg_closest_points_device)."""
        _check(lib().rtg_closest_points_device(self._s, points_ptr or None, n, 0, out_ptr or None, stream or None))

    def crossings(self, rays, coherent: bool = False):
        """How many surfaces each RAY_DTYPE ray meets with 0 < t < tmax -- every one, with no bound
        on their number -- and at how many of them it goes against the geometric normal, on host
        arrays (rtg_count_crossings; synchronous): a CROSSINGS_DTYPE array.  ``count & 1`` is the
        parity test, ``count - entering`` the leaving hits.  ``coherent`` is accepted and ignored.
        Bit for bit HostScene.crossings."""
        return _query_crossings(lib().rtg_count_crossings, self._s, rays, coherent)

    def crossings_device(self, rays_ptr: int, n: int, out_ptr: int, stream: int = 0, coherent: bool = False):
        """Asynchronous crossing counts on device buffers (n x 32 B rays, n x 8 B results) on
        ``stream`` (rtg_count_crossings_device)."""
        _check(lib().rtg_count_crossings_device(self._s, rays_ptr or None, n, _query_flags(False, coherent),
                                                out_ptr or None, stream or None))

    def signed_distance(self, points, direction=None):
        """closest() and, in the same launch, one unbounded crossing walk from each point along
        ``direction`` (three floats; None: the library's default, which lies in no coordinate or
        diagonal plane), on host arrays (rtg_signed_distance_points; synchronous).  The
        NEAREST_DTYPE record is closest()'s with the crossing count in ``pad0`` and, on a hit with an
        odd count, a negative ``dist`` (-0.0 on the surface).  Inside means inside an odd number of
        closed surfaces; on an open surface choose a direction that leaves through it (a height
        field: (0, 0, 1) answers "below the terrain").  Bit for bit HostScene.signed_distance."""
        return _query_signed_distance(lib().rtg_signed_distance_points, self._s, points, direction)

    def signed_distance_device(self, points_ptr: int, n: int, out_ptr: int, direction=None, stream: int = 0):
        """Asynchronous signed-distance queries on device buffers (n x 16 B points, n x 32 B
        results) on ``stream`` (rtg_signed_distance_points_device); ``direction`` is host data."""
        d = _direction(direction)
        _check(lib().rtg_signed_distance_points_device(self._s, points_ptr or None, n,
                                                       None if d is None else d.ctypes.data, 0, out_ptr or None,
                                                       stream or None))

    def camera_rays(self, camera: int = 0, rows=(0, 0), sample: int = 0, seed: int = 0x5EED) -> np.ndarray:
        """The rays render() traces for ``camera`` at sample index ``sample`` and ``seed``, rows
        ``rows`` in pixel order (rtg_camera_rays): RAY_DTYPE array, tmax = inf, time = the
        motion-blur draw."""
        c = self._camera(camera)
        r0 = max(rows[0], 0)
        r1 = c["height"] if rows[1] <= 0 or rows[1] > c["height"] else rows[1]
        rays = np.zeros(max(r1 - r0, 0) * c["width"], RAY_DTYPE)
        o = self.opts(camera, sample, 1, rows, 0, seed)
        _check(lib().rtg_camera_rays(self._s, ctypes.byref(o), rays.ctypes.data))
        return rays

    def camera_rays_device(self, rays_ptr: int, camera: int = 0, rows=(0, 0), sample: int = 0, seed: int = 0x5EED,
                           stream: int = 0):
        """camera_rays() into a device buffer (width x rows x 32 B) on ``stream``; asynchronous."""
        o = self.opts(camera, sample, 1, rows, 0, seed)
        _check(lib().rtg_camera_rays_device(self._s, ctypes.byref(o), rays_ptr or None, stream or None))

    @staticmethod
    def radiance_opts(camera=0, sample=0, samples=1, seed=0x5EED, first_pixel=0, camera_eye=False) -> RadianceOpts:
        return RadianceOpts(camera, sample, samples, RTG_RADIANCE_CAMERA_EYE if camera_eye else 0, seed, first_pixel, 0)

    def radiance(self, rays, camera: int = 0, sample: int = 0, samples: int = 1, seed: int = 0x5EED, pixel_ids=None,
                 first_pixel: int = 0, camera_eye: bool = False) -> np.ndarray:
        """The colour the renderer computes along caller rays (rtg_radiance_rays; synchronous):
        (n, 4) float32 -- unclamped rgb and the primary hit's t (tmax on a miss).  rays:
        RAY_DTYPE array.  Ray i plays pixel ``pixel_ids[i]`` (or ``first_pixel + i``) of
        ``camera``, which supplies the renderer flags and the image size of the background
        texture and nothing else; sample ``s`` of it uses render()'s random numbers for that
        pixel, sample and ``seed``.  ``samples`` > 1: the plain float mean of samples ``sample``
        .. ``sample + samples - 1``, summed in ascending order.  Primary hits are shaded as seen
        from the ray's origin, or from the camera's position with ``camera_eye`` (as render()
        shades its depth-of-field rays): ``radiance(camera_rays(seed=s), seed=s,
        camera_eye=True)`` is render()'s image of a one-sample camera bit for bit."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        n = rays.size
        ids = None if pixel_ids is None else np.ascontiguousarray(pixel_ids, np.int32)
        if ids is not None and ids.size != n:
            raise ValueError(f"{ids.size} pixel ids for {n} rays")
        out = np.zeros((n, 4), np.float32)
        o = self.radiance_opts(camera, sample, samples, seed, first_pixel, camera_eye)
        _check(lib().rtg_radiance_rays(self._s, ctypes.byref(o), rays.ctypes.data,
                                       ids.ctypes.data if ids is not None else None, n, out.ctypes.data))
        return out

    def radiance_device(self, rays_ptr: int, n: int, out_ptr: int, ids_ptr: int = 0, stream: int = 0, camera: int = 0,
                        sample: int = 0, samples: int = 1, seed: int = 0x5EED, first_pixel: int = 0,
                        camera_eye: bool = False):
        """Asynchronous radiance() on device buffers (e.g. torch tensor data_ptr()s: n x 32 B rays,
        n x 4 float32 out, optionally n int32 pixel ids) on ``stream``; allocates nothing."""
        o = self.radiance_opts(camera, sample, samples, seed, first_pixel, camera_eye)
        _check(lib().rtg_radiance_rays_device(self._s, ctypes.byref(o), rays_ptr or None, ids_ptr or None, n,
                                              out_ptr or None, stream or None))

    def surface(self, rays, coherent: bool = False) -> np.ndarray:
        """What render() knows about the point each ray hits (rtg_surface_rays; synchronous):
        SURFACE_DTYPE array.  ``t / object / face`` are trace()'s closest hit and ``ng`` its
        geometric normal; ``n`` is the shading normal (normal and bump maps applied, not flipped
        towards the ray), ``u, v`` the texture coordinates, ``material`` the object's material index
        and ``kd`` the diffuse coefficient after replace_kd / blend_kd / Perlin textures (reported
        for every hit, also where the render never reads it: emissive and replace_all objects).  A
        miss: t = tmax, object = face = material = -1, zeros elsewhere.  ``coherent`` is a
        performance hint, never a different answer."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(rays.size, SURFACE_DTYPE)
        _check(lib().rtg_surface_rays(self._s, rays.ctypes.data, rays.size, _query_flags(False, coherent),
                                      out.ctypes.data))
        return out

    def surface_device(self, rays_ptr: int, n: int, out_ptr: int, stream: int = 0, coherent: bool = False):
        """Asynchronous surface() on device buffers (e.g. torch tensor data_ptr()s: n x 32 B rays,
        n x 64 B out) on ``stream``; allocates nothing."""
        _check(lib().rtg_surface_rays_device(self._s, rays_ptr or None, n, _query_flags(False, coherent),
                                             out_ptr or None, stream or None))

    def export_bvh(self):
        """(nodes (N, 8) float32, tris (F, 12) float32): the device's walk records."""
        nn, nf = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().rtg_scene_export_bvh(self._s, None, 0, None, 0, ctypes.byref(nn), ctypes.byref(nf)))
        nodes = np.zeros((nn.value, 8), np.float32)
        tris = np.zeros((nf.value, 12), np.float32)
        _check(lib().rtg_scene_export_bvh(self._s, nodes.ctypes.data, nn.value, tris.ctypes.data, nf.value,
                                          ctypes.byref(nn), ctypes.byref(nf)))
        return nodes, tris

    def stats(self) -> dict:
        st = Stats()
        _check(lib().rtg_scene_stats(self._s, ctypes.byref(st)))
        return st.as_dict()

    def reset_stats(self):
        _check(lib().rtg_scene_reset_stats(self._s))

    def timings(self) -> dict:
        """{kernel: ms} of the last render issued with RTG_RENDER_TIMING (synchronises)."""
        ms = (ctypes.c_float * 8)()
        names = (ctypes.c_char_p * 8)()
        n = ctypes.c_int32()
        _check(lib().rtg_scene_timings(self._s, ms, names, 8, ctypes.byref(n)))
        return {names[k].decode(): float(ms[k]) for k in range(n.value)}

    def timed_samples(self) -> int:
        """Samples per pixel the stages of timings() covered (the last pass of a multi-sample
        render carries several, RTG_RENDER_SAMPLE_PASSES)."""
        n = ctypes.c_int32()
        _check(lib().rtg_scene_timed_samples(self._s, ctypes.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_s", None):
            lib().rtg_scene_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedArray:
    """Page-locked host array (rtg_host_alloc): the frame buffer of the drop-in host path
    (the CLI allocates its frames the same way), so the device-to-host copy is one DMA."""

    def __init__(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = ctypes.c_void_p()
        _check(lib().rtg_host_alloc(nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self.array = np.frombuffer((ctypes.c_char * nbytes).from_address(self.ptr), dtype).reshape(shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib().rtg_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resolve_accum(accum: np.ndarray):
    """(sum w*c, sum w) per pixel -> (hdr, ldr); host side (samples split across devices)."""
    h, w, _ = accum.shape
    accum = np.ascontiguousarray(accum, np.float32)
    hdr = np.zeros((h, w, 3), np.float32)
    ldr = np.zeros((h, w, 3), np.uint8)
    _check(lib().rtg_resolve_accum(accum.ctypes.data, w, h, hdr.ctypes.data, ldr.ctypes.data))
    return hdr, ldr


def tonemap(hdr: np.ndarray, key=0.18, burn=1.0, saturation=1.0, gamma=2.2, device: int = 0) -> np.ndarray:
    """Photographic tonemapper (Tonemapper::Tonemap, tonemapper.h:28-60) on the GPU."""
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w, _ = hdr.shape
    ldr = np.zeros((h, w, 3), np.uint8)
    p = TonemapParams(key, burn, saturation, gamma)
    _check(lib().rtg_tonemap(hdr.ctypes.data, w, h, ctypes.byref(p), ldr.ctypes.data, device))
    return ldr


def tonemap_log_average(hdr: np.ndarray, mode: int = -1, device: int = 0) -> float:
    """Tonemapper::avgLuminance (tonemapper.h:35-48) on the GPU; mode as rtg_tonemap_log_average."""
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w, _ = hdr.shape
    out = ctypes.c_double()
    _check(lib().rtg_tonemap_log_average(hdr.ctypes.data, w, h, mode, ctypes.byref(out), device))
    return out.value


def write_png(path: str, ldr: np.ndarray):
    ldr = np.ascontiguousarray(ldr, np.uint8)
    _check(lib().rtg_write_png(os.fsencode(path), ldr.shape[1], ldr.shape[0], ldr.ctypes.data))
