"""Crossing counts and signed distances on the host (rtg_desc_count_crossings,
rtg_desc_signed_distance_points: the walks that define the queries and the yardsticks of the device
kernels, test_gpu_crossings.py).  Checked against the analytic layered scene, the multi-hit walk's
own counts (wherever it holds fewer than 8 hits the two walks accepted the same set), a float64
brute force that returns every hit, the closest-point walk byte for byte, and the analytic inside
of a scene of closed shapes (sdf_scenes.py).

Figures of the seeds used here, printed by the tests: of the layered scene's 4 096 slanted rays
one is grazing (0.00024) and of the two-spheres cone none; of the closed-shapes scene's 4 000
points none has a grazing ray along the default direction (the expected share is of order 1e-4)
and every sign is the analytic one, 623 points being inside; the caps are 1 %.

The height field of closest_util.write_grid carries its heights along y, so "below the
interpolated surface" is asked along (0, 1, 0), the direction that leaves through it.  Along
(0, 0, 1) a ray runs inside the slab of heights and leaves through the field's edge z = 4: its
parity is "the point and the exit lie on different sides of the surface", which is asserted too.
"""
import os

import numpy as np
import pytest

import bvh_cases as bc
import closest_util as cu
import multihit_scenes as ms
import oracle_bind as ob
import query_util as qu
import rtgpu
import sdf_scenes as sd
import walk_cases as wc
from test_multihit_host import NAMES as MULTI_NAMES
from test_multihit_host import _scene as multi_scene
from test_query_host import _cone_rays

SCENES = os.path.join(ob.GOLDEN, "scenes")


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def test_layered_analytic(tmp_path):
    hs = ms.load_layered(tmp_path)
    xy = ms.axis_points(64, seed=11)
    # down from z = 0: 13 sheet hits against +z normals and the three near roots enter
    c = hs.crossings(ms.axis_rays(xy))
    assert np.all(c["count"] == 19) and np.all(c["entering"] == 16)
    # up from below the spheres: only the three near roots enter
    c = hs.crossings(ms.axis_rays(xy, z0=-30.0, down=False))
    assert np.all(c["count"] == 19) and np.all(c["entering"] == 3)
    # from the spheres' centre heading down: three far roots, all leaving
    c = hs.crossings(ms.axis_rays(xy, z0=ms.SPHERE_Z))
    assert np.all(c["count"] == 3) and np.all(c["entering"] == 0)
    # a finite tmax; the duplicated sheet counts twice
    assert np.all(hs.crossings(ms.axis_rays(xy, tmax=3.5))["count"] == 3)
    c = hs.crossings(ms.axis_rays(xy, tmax=5.5))
    assert np.all(c["count"] == 6) and np.all(c["entering"] == 6)
    # tmax equal to a hit's own t drops that hit and its tie (strict <)
    hits8 = hs.trace_multi(ms.axis_rays(xy), 8)
    for j, left in ((2, 2), (4, 4), (5, 4), (6, 6)):
        r = ms.axis_rays(xy)
        r["tmax"] = hits8["t"][:, j]
        assert np.all(hs.crossings(r)["count"] == left), j
    assert hs.crossings(np.zeros(0, rtgpu.RAY_DTYPE)).shape == (0,)


def _against_multi(name, label, hs, rays, seen):
    c = hs.crossings(rays)
    _, cnt = hs.trace_multi(rays, 8, counts=True)
    below = cnt < 8
    bad = np.flatnonzero(below & (c["count"] != cnt))
    assert bad.size == 0, (name, label, bad[:8], c[bad[:8]], cnt[bad[:8]], rays[bad[:8]])
    assert np.all(c["count"][~below] >= 8), (name, label)
    assert np.all(c["entering"] >= 0) and np.all(c["entering"] <= c["count"]), (name, label)
    seen[0] += int(below.sum())
    seen[1] += int((~below).sum())
    seen[2] = max(seen[2], int(c["count"].max()))


def test_counts_equal_multihit_on_its_scenes(tmp_path_factory):
    """Every scene and ray set of test_multihit_host.py: count == the k = 8 count where that is
    below 8, >= 8 elsewhere; both occur."""
    seen = [0, 0, 0]
    for name in MULTI_NAMES:
        hs, sets = multi_scene(name, tmp_path_factory)
        for label, rays in sets.items():
            _against_multi(name, label, hs, rays, seen)
    print("rays holding < 8 hits", seen[0], "holding 8", seen[1], "largest count", seen[2])
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 8


def test_counts_equal_multihit_on_the_adversarial_meshes(tmp_path_factory):
    """Every case of bvh_cases with the edge, aimed and light rays of walk_cases.ray_sets."""
    seen = [0, 0, 0]
    with np.errstate(all="ignore"):
        for name in bc.NAMES:
            hs = wc.load(tmp_path_factory.mktemp(name), name)
            rays, _ = wc.ray_sets(hs, name)
            _against_multi(name, "all", hs, rays, seen)
    print("rays holding < 8 hits", seen[0], "holding 8", seen[1], "largest count", seen[2])
    assert seen[0] > 0 and seen[1] > 0 and seen[2] >= 300      # copies_300: every copy counted


def _brute_check(name, hs, rays):
    """count == the float64 brute force's number of hits for every ray that is not grazing (at most
    1 % are), and entering == the number of them with a positive determinant of (d, e2, e1) --
    the ray against (v1 - v0) x (v2 - v0) -- plus the spheres' near roots."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    o, d = qu.origins(rays).astype(np.float64), qu.directions(rays).astype(np.float64)
    ref, grazing = ms.brute_force_all(objs, meshes, faces, o, d)
    got = hs.crossings(rays)
    n_ref = np.array([len(lst) for lst in ref])
    print(name, "rays", rays.size, "grazing", int(grazing.sum()), "share %.5f" % grazing.mean(), "largest count", int(n_ref.max()))
    assert grazing.mean() <= 0.01
    ok = ~grazing
    bad = np.flatnonzero(ok & (got["count"] != n_ref))
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], n_ref[bad[:8]])
    # entering, from the brute force's own quantities: a face is entered where d . ((v1 - v0) x
    # (v2 - v0)) < 0 (its det = (d x e2) . e1 = -d . (e1 x e2) is positive); a sphere at its near
    # root (-b - sqrt(disc)) / 2a
    enter = np.zeros(rays.size, int)
    for k, obj in enumerate(objs):
        if obj["kind"] == qu.RTG_OBJ_SPHERE:
            c, r = obj["center"].astype(np.float64), float(obj["radius"])
            oc = o - c
            a, b = (d * d).sum(1), 2.0 * (d * oc).sum(1)
            disc = b * b - 4.0 * a * ((oc * oc).sum(1) - r * r)
            near = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)
            enter += ((disc > 0.0) & (near > 0.0)).astype(int)
            continue
        m = meshes[obj["mesh"]]
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
            inside = (det != 0.0) & (beta >= 0.0) & (gamma >= 0.0) & (1.0 - beta - gamma >= 0.0) & (tf > 0.0)
            # the stored normal agrees with the winding (asserted: the sign convention of `entering`)
            assert np.dot(F["n"].astype(np.float64), np.cross(e1, e2)) > 0.0
            enter += (inside & (det > 0.0)).astype(int)
    bad = np.flatnonzero(ok & (got["entering"] != enter))
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], enter[bad[:8]])
    return got, grazing


def test_brute_force_layered(tmp_path_factory):
    hs, _ = multi_scene("layered", tmp_path_factory)
    got, grazing = _brute_check("layered", hs, ms.slanted_rays(4096, seed=20253))
    assert (got["count"][~grazing] > 8).any()


def test_brute_force_two_spheres(tmp_path_factory):
    hs, _ = multi_scene("two_spheres", tmp_path_factory)
    got, _ = _brute_check("two_spheres", hs, _cone_rays(qu.camera_record(hs), 4096, seed=20250))
    assert set(np.unique(got["count"])) == {0, 2} and set(np.unique(got["entering"])) == {0, 1}


# ---- signed distance

@pytest.fixture(scope="module")
def closed(tmp_path_factory):
    hs = sd.load_closed(tmp_path_factory.mktemp("closed"))
    xyz = sd.closed_points(hs, 4000, seed=20280)
    pts = rtgpu.make_points(xyz)
    pts.setflags(write=False)
    return hs, xyz, pts


def test_signed_distance_is_closest_with_a_sign(closed):
    hs, xyz, pts = closed
    got = hs.signed_distance(pts)
    want = hs.closest(pts)
    assert (want["object"] >= 0).all()
    assert np.array_equal(np.abs(got["dist"]).view(np.uint32), want["dist"].view(np.uint32))
    for f in ("object", "face", "p", "pad1"):
        assert got[f].tobytes() == want[f].tobytes(), f
    # pad0 is the crossing count of the ray from the point along the default direction
    rays = rtgpu.make_rays(xyz, np.tile(sd.DEFAULT_DIR, (len(xyz), 1)))
    assert np.array_equal(got["pad0"], hs.crossings(rays)["count"])
    assert np.array_equal(np.signbit(got["dist"]), (got["pad0"] & 1) == 1)
    assert got.tobytes() == hs.signed_distance(pts, direction=sd.DEFAULT_DIR).tobytes()


def test_sign_is_the_analytic_inside(closed):
    hs, xyz, pts = closed
    got = hs.signed_distance(pts)
    inside, _ = sd.closed_inside(hs, xyz)
    grazing, n64 = sd.grazing(hs, xyz, np.tile(sd.DEFAULT_DIR.astype(np.float64), (len(xyz), 1)))
    neg = np.signbit(got["dist"])
    print("closed shapes: points", len(xyz), "grazing", int(grazing.sum()), "share %.5f" % grazing.mean(),
          "inside", int(inside.sum()), "sign mismatches among all points", int((neg != inside).sum()))
    assert grazing.mean() <= 0.01
    ok = ~grazing
    bad = np.flatnonzero(ok & (neg != inside))
    assert bad.size == 0, (bad[:8], xyz[bad[:8]], got[bad[:8]])
    assert np.array_equal(got["pad0"][ok], n64[ok])
    for k in range(4):                           # both signs on every object
        on = ok & (got["object"] == k)
        assert (neg[on]).any() and (~neg[on]).any(), k
    # the shell's cavity is outside: inside two surfaces
    cavity = np.abs(xyz.astype(np.float64) - sd.SHELL_CENTRE).max(1) < 1.0
    assert cavity.sum() > 10 and not neg[cavity & ok].any()


def _grid_points(grid, n, seed):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-3.99, 3.99, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-3.99, 3.99, n)], 1).astype(np.float32)
    return xyz, grid.height(xyz[:, 0], xyz[:, 2])


def test_below_the_height_field(tmp_path):
    """Along the field's up axis the sign is "below the interpolated surface", for every point at
    least 1e-3 of the height range from it."""
    hs = cu.load(cu.write_grid(tmp_path))
    grid = sd.Grid()
    xyz, h = _grid_points(grid, 4000, seed=20281)
    clear = np.abs(xyz[:, 1].astype(np.float64) - h) >= 1e-3 * grid.range
    below = xyz[:, 1].astype(np.float64) < h
    got = hs.signed_distance(rtgpu.make_points(xyz), direction=(0, 1, 0))
    neg = np.signbit(got["dist"])
    print("height field: points", len(xyz), "clear of the surface", int(clear.sum()), "below", int(below[clear].sum()))
    assert clear.sum() > 3900 and below[clear].sum() > 500 and (~below[clear]).sum() > 500
    assert np.array_equal(neg[clear], below[clear])
    assert np.array_equal(got["pad0"][clear], below[clear].astype(np.int32))
    assert np.array_equal(np.abs(got["dist"]).view(np.uint32), hs.closest(rtgpu.make_points(xyz))["dist"].view(np.uint32))


def test_height_field_along_z(tmp_path):
    """dir = (0, 0, 1) on the same field: the ray stays at its height and leaves through the edge
    z = 4, so the count is odd exactly when the point and the exit lie on different sides of the
    surface (both at least 1e-3 of the height range from it)."""
    hs = cu.load(cu.write_grid(tmp_path))
    grid = sd.Grid()
    xyz, h = _grid_points(grid, 4000, seed=20282)
    y = xyz[:, 1].astype(np.float64)
    h_exit = grid.height(xyz[:, 0], np.full(len(xyz), 4.0))
    clear = (np.abs(y - h) >= 1e-3 * grid.range) & (np.abs(y - h_exit) >= 1e-3 * grid.range)
    want = (y < h) != (y < h_exit)
    got = hs.signed_distance(rtgpu.make_points(xyz), direction=(0, 0, 1))
    grazing, _ = sd.grazing(hs, xyz, np.tile(np.array([0.0, 0.0, 1.0]), (len(xyz), 1)))
    ok = clear & ~grazing
    print("height field along z: clear", int(clear.sum()), "grazing", int(grazing.sum()), "odd", int(want[ok].sum()),
          "largest count", int(got["pad0"].max()))
    assert grazing.mean() <= 0.01 and want[ok].sum() > 200 and got["pad0"].max() > 2
    assert np.array_equal(np.signbit(got["dist"])[ok], want[ok])


# ---- arguments

def test_argument_errors(tmp_path):
    L = rtgpu.lib()
    for sym in ("rtg_count_crossings_device", "rtg_count_crossings", "rtg_desc_count_crossings",
                "rtg_signed_distance_points_device", "rtg_signed_distance_points", "rtg_desc_signed_distance_points"):
        assert hasattr(L, sym) and sym in rtgpu.EXPORTED
    assert L.rtg_abi_version() == 6 and rtgpu.CROSSINGS_DTYPE.itemsize == 8
    hs = rtgpu.HostScene("simple.xml")
    rays = rtgpu.make_rays([[0, 0, 0]], [[0, 0, -1]])
    out = np.zeros(1, rtgpu.CROSSINGS_DTYPE)
    f = L.rtg_desc_count_crossings

    def err():
        return L.rtg_last_error().decode()

    assert f(hs.desc, None, 0, 0, None) == 0                                               # n = 0
    assert f(hs.desc, None, 1, 0, out.ctypes.data) == -1 and "null" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 0, None) == -1 and "null" in err()
    assert f(None, rays.ctypes.data, 1, 0, out.ctypes.data) == -1 and "null" in err()
    assert f(hs.desc, rays.ctypes.data, 1 << 31, 0, out.ctypes.data) == -1 and "ray count" in err()
    assert f(hs.desc, rays.ctypes.data, -1, 0, out.ctypes.data) == -1
    assert f(hs.desc, rays.ctypes.data, 1, rtgpu.RTG_QUERY_ANY_HIT, out.ctypes.data) == -1 and "RTG_QUERY_ANY_HIT" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 4, out.ctypes.data) == -1 and "unknown query flags" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 0, out.ctypes.data) == 0 and out["count"][0] >= 1
    first = out.copy()
    assert f(hs.desc, rays.ctypes.data, 1, rtgpu.RTG_QUERY_COHERENT, out.ctypes.data) == 0 and out.tobytes() == first.tobytes()
    nb = rtgpu.HostScene("simple.xml", device_bvh=True)
    with pytest.raises(rtgpu.RTGError) as e:
        nb.crossings(rays)
    assert e.value.code == -1 and "RTG_LOAD_DEVICE_BVH" in str(e.value)
    # NaN and non-positive tmax, a NaN direction: whatever the comparisons give, and no crash
    odd = np.concatenate([rays] * 5)
    odd["tmax"][:4] = [0.0, -1.0, np.nan, np.inf]
    odd["dx"][4] = np.nan
    c = hs.crossings(odd)
    assert c.shape == (5,) and np.all(c["count"][:3] == 0) and c["count"][3] == first["count"][0]

    # signed distance
    g = L.rtg_desc_signed_distance_points
    pts = rtgpu.make_points(np.zeros((2, 3), np.float32))
    res = np.zeros(2, rtgpu.NEAREST_DTYPE)
    v = np.array([0, 0, 1], np.float32)
    assert g(hs.desc, None, 0, None, 0, None) == 0
    assert g(hs.desc, None, 2, None, 0, res.ctypes.data) == -1 and "null" in err()
    assert g(hs.desc, pts.ctypes.data, 2, None, 0, None) == -1 and "null" in err()
    assert g(None, pts.ctypes.data, 2, None, 0, res.ctypes.data) == -1 and "null" in err()
    assert g(hs.desc, pts.ctypes.data, 1 << 31, None, 0, res.ctypes.data) == -1 and "point count" in err()
    for flags in (1, 2, 1 << 31):
        assert g(hs.desc, pts.ctypes.data, 2, None, flags, res.ctypes.data) == -1 and "flags" in err()
    for bad in ([np.nan, 0, 1], [0, np.inf, 0], [0, 0, 0], [-0.0, 0, 0]):
        b = np.array(bad, np.float32)
        assert g(hs.desc, pts.ctypes.data, 2, b.ctypes.data, 0, res.ctypes.data) == -1 and "dir" in err(), bad
        assert g(hs.desc, None, 0, b.ctypes.data, 0, None) == -1, bad                      # before the n == 0 rule
    assert g(hs.desc, pts.ctypes.data, 2, v.ctypes.data, 0, res.ctypes.data) == 0
    with pytest.raises(rtgpu.RTGError) as e:
        nb.signed_distance(pts)
    assert e.value.code == -1 and "RTG_LOAD_DEVICE_BVH" in str(e.value)
    # an ellipsoid scene: refused for every n, after the argument errors
    el = cu.load(cu.write_moved(tmp_path, "ellipsoid", sphere_scaling="s1"))
    canary = np.full(2 * 8, 0xA5A5A5A5, np.uint32)
    assert g(el.desc, pts.ctypes.data, 2, None, 0, canary.ctypes.data) == -6 and "object 2" in err()
    assert (canary == 0xA5A5A5A5).all()
    assert g(el.desc, None, 0, None, 0, None) == -6
    assert g(el.desc, pts.ctypes.data, 2, None, 1, canary.ctypes.data) == -1
    assert el.crossings(rays).shape == (1,)                                                # crossings take the scene


def test_miss_record_and_points_that_are_not_finite(closed):
    hs, xyz, pts = closed
    far = hs.closest(pts)["dist"]
    p = pts.copy()
    p["max_dist"] = far * np.float32(0.5)                     # every point misses
    p["max_dist"][7] = np.nan
    p["x"][3] = np.nan
    p["y"][4] = np.inf
    p["z"][5] = -np.inf
    got = hs.signed_distance(p)
    want = hs.closest(p)
    assert np.all(got["object"] == -1) and np.all(got["face"] == -1) and np.all(got["p"] == 0)
    # dist keeps max_dist's own bits whatever the count; pad0 carries the count all the same
    assert np.array_equal(got["dist"].view(np.uint32), p["max_dist"].view(np.uint32))
    counts = hs.signed_distance(pts)["pad0"]
    fin = np.ones(len(p), bool)
    fin[[3, 4, 5]] = False
    assert np.array_equal(got["pad0"][fin], counts[fin]) and (counts[fin] & 1).any()
    assert np.all(got["pad0"][~fin] == 0)
    for f in ("dist", "object", "face", "p", "pad1"):
        assert got[f].tobytes() == want[f].tobytes(), f
