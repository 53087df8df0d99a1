"""Helpers of the ray-query tests (test_query_host.py, test_gpu_query.py): NumPy views of a scene
description, the pixel-centre camera rays in NumPy, and an independent float64 brute force."""
import ctypes

import numpy as np

import rtgpu

# rtg_object / rtg_face / rtg_mesh of include/rtgpu.h (packed == natural layout here)
OBJ_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("mesh", "<i4"), ("flags", "<i4"), ("tex", "<i4", 5),
                      ("id", "<i4"), ("inv_transform", "<f8", 16), ("inv_transpose", "<f8", 16),
                      ("base_inv_transpose", "<f8", 16), ("transform", "<f8", 16), ("bbox_min", "<f4", 3),
                      ("bbox_max", "<f4", 3), ("motion_blur", "<f4", 3), ("center", "<f4", 3), ("radius", "<f4"),
                      ("pad0", "<i4")])
FACE_DTYPE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("n", "<f4", 3), ("uv", "<f4", 6),
                       ("area", "<f8")])
MESH_DTYPE = np.dtype([("face_offset", "<i4"), ("face_count", "<i4"), ("node_offset", "<i4"), ("node_count", "<i4"),
                       ("has_uv", "<i4"), ("id", "<i4"), ("surface_area", "<f8")])
assert (OBJ_DTYPE.itemsize, FACE_DTYPE.itemsize, MESH_DTYPE.itemsize) == (608, 80, 32)

RTG_OBJ_MESH, RTG_OBJ_INSTANCE, RTG_OBJ_SPHERE = 0, 1, 2
RTG_OBJF_SHADOW_SKIP = 1


class Desc(ctypes.Structure):
    """rtg_scene_desc (include/rtgpu.h)."""
    _list = ("cameras", "materials", "brdfs", "point_lights", "area_lights", "dir_lights", "spot_lights",
             "env_lights", "textures", "images", "objects", "meshes")
    _fields_ = ([("background", ctypes.c_int32 * 3), ("shadow_epsilon", ctypes.c_float),
                 ("max_recursion_depth", ctypes.c_int32), ("bg_texture", ctypes.c_int32),
                 ("ambient_light", ctypes.c_float * 3)] +
                [f for n in _list for f in ((n, ctypes.c_void_p), ("num_" + n, ctypes.c_int32))] +
                [("faces", ctypes.c_void_p), ("num_faces", ctypes.c_int64), ("nodes", ctypes.c_void_p),
                 ("num_nodes", ctypes.c_int64), ("mesh_lights", ctypes.c_void_p), ("num_mesh_lights", ctypes.c_int32),
                 ("pad0", ctypes.c_int32)])


def _array(ptr, n, dtype):
    if not n:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (n * dtype.itemsize)).from_address(ptr), dtype).copy()


def scene_arrays(hs):
    """(background int[3], objects, meshes, faces) of a HostScene as NumPy copies."""
    d = Desc.from_address(hs.desc)
    return (np.array(d.background[:], np.int32), _array(d.objects, d.num_objects, OBJ_DTYPE),
            _array(d.meshes, d.num_meshes, MESH_DTYPE), _array(d.faces, d.num_faces, FACE_DTYPE))


def camera_record(hs, idx=0):
    """Camera idx of the description: position, gaze, up, right, q (float32[3]) and the plane."""
    head = rtgpu._DescHead.from_address(hs.desc)
    assert 0 <= idx < head.num_cameras
    cam = rtgpu._Camera.from_address(head.cameras + idx * rtgpu.RTG_CAMERA_SIZE)
    f3 = np.array(cam.f3[:], np.float32).reshape(5, 3)
    ext = np.array(cam.ext[:], np.float32)
    return {"position": f3[0], "gaze": f3[1], "up": f3[2], "right": f3[3], "q": f3[4], "left": ext[0],
            "right_ext": ext[1], "bottom": ext[2], "top": ext[3], "near": ext[4], "width": cam.width,
            "height": cam.height, "aperture": cam.aperture}


def numpy_camera_rays(cam):
    """GenerateRay through the pixel centre (raytracer.cpp:661-699, camera.cpp:74-80) without
    depth of field, operation by operation in float32 / float64 as the reference: RAY_DTYPE array
    in pixel order, tmax = inf, time = 0."""
    f32 = np.float32
    w, h = cam["width"], cam["height"]
    su = ((np.arange(w) + 0.5) * np.float64(f32(cam["right_ext"]) - f32(cam["left"])) / w).astype(f32)
    sv = ((np.arange(h) + 0.5) * np.float64(f32(cam["top"]) - f32(cam["bottom"])) / h).astype(f32)
    su = np.broadcast_to(su[None, :], (h, w)).reshape(-1)
    sv = np.broadcast_to(sv[:, None], (h, w)).reshape(-1)
    q, right, up, pos = (cam[k].astype(f32) for k in ("q", "right", "up", "position"))
    nsv = -sv
    d = [((q[k] + right[k] * su) + up[k] * nsv) - pos[k] for k in range(3)]
    assert all(c.dtype == f32 for c in d)
    length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    rays = np.zeros(w * h, rtgpu.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = pos
    rays["dx"], rays["dy"], rays["dz"] = d[0] / length, d[1] / length, d[2] / length
    rays["tmax"] = np.inf
    return rays


def origins(rays):
    return np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)


def directions(rays):
    return np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)


def brute_force(objs, meshes, faces, o, d, edge=1e-5):
    """Closest hit of every ray against every face and every sphere in float64, no BVH
    (identity transforms only).  Returns (t, object, grazing): t = inf / object = -1 for a miss;
    grazing marks rays whose barycentrics on some face are within `edge` of one of its edges, or
    whose discriminant on some sphere is within edge * b^2 of zero."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    n = len(o)
    best_t = np.full(n, np.inf)
    best_k = np.full(n, -1)
    grazing = np.zeros(n, bool)
    ident = np.eye(4).reshape(-1)
    for k, ob in enumerate(objs):
        assert np.array_equal(ob["inv_transform"], ident), "brute force handles identity transforms only"
        if ob["kind"] == RTG_OBJ_SPHERE:
            c, r = ob["center"].astype(np.float64), float(ob["radius"])
            oc = o - c
            a = (d * d).sum(1)
            b = 2.0 * (d * oc).sum(1)
            cc = (oc * oc).sum(1) - r * r
            disc = b * b - 4.0 * a * cc
            grazing |= np.abs(disc) < edge * b * b
            sq = np.sqrt(np.maximum(disc, 0.0))
            t_lo, t_hi = (-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)
            t = np.where(t_lo > 0.0, t_lo, t_hi)
            ok = (disc >= 0.0) & (t > 0.0)
        else:
            m = meshes[ob["mesh"]]
            t = np.full(n, np.inf)
            ok = np.zeros(n, bool)
            for F in faces[m["face_offset"]:m["face_offset"] + m["face_count"]]:
                v0, v1, v2 = (F[x].astype(np.float64) for x in ("v0", "v1", "v2"))
                e1, e2 = v1 - v0, v2 - v0
                p = np.cross(d, e2)
                det = p @ e1
                with np.errstate(divide="ignore", invalid="ignore"):
                    s = o - v0
                    beta = (s * p).sum(1) / det
                    qv = np.cross(s, e1)
                    gamma = (d * qv).sum(1) / det
                    tf = (qv @ e2) / det
                third = 1.0 - beta - gamma
                inside = (det != 0.0) & (beta >= 0.0) & (gamma >= 0.0) & (third >= 0.0) & (tf > 0.0)
                near = (det != 0.0) & (tf > 0.0) & (beta > -edge) & (gamma > -edge) & (third > -edge) & \
                    (np.minimum(np.minimum(np.abs(beta), np.abs(gamma)), np.abs(third)) < edge)
                grazing |= near
                better = inside & (tf < t)
                t = np.where(better, tf, t)
                ok |= inside
        better = ok & (t < best_t)
        best_t = np.where(better, t, best_t)
        best_k = np.where(better, k, best_k)
    return best_t, best_k, grazing
