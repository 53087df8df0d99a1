"""Closest-point queries on the host (rtg_desc_closest_points: the walk that defines the query and
the yardstick of the device kernel, test_gpu_closest.py) against a float64 brute force over every
face and sphere: the distance, the primitive named and the point returned, with and without a
radius, on the six traversal-set rooms, a height field and a scene of composite transforms; the
adversarial meshes of bvh_cases; the argument errors; the placement side table by behaviour.

Accuracy bound: |dist - d64| <= 2^-20 S (16 ulp of S), S the largest world-coordinate magnitude
among the scene's vertices and the point."""
import ctypes

import numpy as np
import pytest

import bvh_cases as bc
import closest_util as cu
import query_util as qu
import rtgpu
import variant_scenes as zoo
import walk_cases as wc

ROOM_FEATS = (0, 1, 7, 8, 9, 15)          # the traversal sets of rtg_variants.hpp
SCENES = ["room_%d" % f for f in ROOM_FEATS] + ["grid", "moved"]


def write_scene(name, directory):
    if name.startswith("room_"):
        return zoo.room(directory, name, **zoo._feat_switches(int(name[5:])))
    return {"grid": cu.write_grid, "moved": cu.write_moved}[name](directory, name)


class Run:
    """One scene: the host walk's answers for its points (unbounded), with the brute force's."""

    def __init__(self, name, directory):
        self.name = name
        self.hs = cu.load(write_scene(name, directory))
        self.world = cu.World(self.hs)
        self.xyz = cu.points_for(self.world, seed=20260 + len(name))
        self.d64 = cu.brute_force(self.world, self.xyz)
        self.tol = cu.TOL * cu.scale_of(self.world, self.xyz)
        self.got = self.hs.closest(rtgpu.make_points(self.xyz))


_RUNS = {}


@pytest.fixture(params=SCENES)
def run(request, tmp_path_factory):
    name = request.param
    if name not in _RUNS:
        _RUNS[name] = Run(name, tmp_path_factory.mktemp("closest_" + name))
    return _RUNS[name]


def test_distance_against_brute_force(run):
    """Every point: |dist - d64| <= 2^-20 S."""
    got = run.got
    assert (got["object"] >= 0).all() and np.isfinite(got["dist"]).all()
    err = np.abs(got["dist"].astype(np.float64) - run.d64)
    ratio = err / run.tol
    worst = int(np.argmax(ratio))
    print(run.name, "points", len(err), "worst |dist - d64| / (2^-20 S): %.3f" % ratio[worst], "at", run.xyz[worst],
          "dist", got["dist"][worst], "d64", run.d64[worst])
    assert (err <= run.tol).all(), (run.name, worst, ratio[worst], got[worst], run.d64[worst])
    assert (got["pad0"] == 0).all() and (cu.u32(got)[:, 7] == 0).all()


def test_primitive_and_point(run):
    """The primitive named is (within the bound) a nearest one; the point returned lies on it and
    at `dist` from the query point."""
    got, xyz = run.got, run.xyz.astype(np.float64)
    _, objs, _, _ = qu.scene_arrays(run.hs)
    sphere = objs["kind"][got["object"]] == qu.RTG_OBJ_SPHERE
    assert ((got["face"] == -1) == sphere).all()
    d_prim = cu.primitive_distance(run.world, xyz, got["object"], got["face"])
    assert (np.abs(d_prim - run.d64) <= run.tol).all(), run.name
    c = got["p"].astype(np.float64)
    tol_c = cu.TOL * np.maximum(cu.scale_of(run.world, c), cu.scale_of(run.world, xyz))
    on = cu.primitive_distance(run.world, c, got["object"], got["face"])
    assert (on <= tol_c).all(), (run.name, float((on / tol_c).max()))
    away = np.linalg.norm(c - xyz, axis=1)
    assert (np.abs(away - got["dist"]) <= tol_c).all(), (run.name, float((np.abs(away - got["dist"]) / tol_c).max()))


def test_finite_radius(run):
    """max_dist: a miss wherever d64 > max_dist + tol, the unbounded answer within tol wherever
    d64 < max_dist - tol; the miss record is (max_dist, -1, -1, zeros)."""
    rng = np.random.default_rng(5)
    radius = (run.d64 * rng.choice([0.5, 0.999, 1.001, 2.0], len(run.d64))).astype(np.float32)
    radius[::7] = np.float32(np.median(run.d64))
    got = run.hs.closest(rtgpu.make_points(run.xyz, radius))
    must_miss = run.d64 > radius + run.tol
    must_hit = run.d64 < radius - run.tol
    assert must_miss.sum() > 100 and must_hit.sum() > 100
    miss = got["object"] < 0
    assert miss[must_miss].all() and not miss[must_hit].any(), run.name
    assert (np.abs(got["dist"][must_hit] - run.d64[must_hit]) <= run.tol[must_hit]).all()
    assert (got["dist"][~miss] < radius[~miss]).all(), "a hit is strictly nearer than max_dist"
    m = got[miss]
    assert (m["dist"] == radius[miss]).all() and (m["face"] == -1).all() and not m["p"].any()
    assert (cu.u32(m)[:, 3:] == 0).all()
    # only max_dist's square enters: 0 and NaN admit nothing, -r admits what r admits and a miss
    # reports -r itself
    zero = run.hs.closest(rtgpu.make_points(run.xyz[:64], 0.0))
    assert (zero["object"] == -1).all() and (zero["dist"] == 0).all()
    nan = run.hs.closest(rtgpu.make_points(run.xyz[:64], np.nan))
    assert (nan["object"] == -1).all() and np.isnan(nan["dist"]).all() and not nan["p"].any()
    neg = run.hs.closest(rtgpu.make_points(run.xyz, -radius))
    assert np.array_equal(neg["object"], got["object"]) and np.array_equal(neg["face"], got["face"])
    assert np.array_equal(neg["p"], got["p"])
    assert np.array_equal(neg["dist"][~miss], got["dist"][~miss]) and (neg["dist"][miss] == -radius[miss]).all()


def test_points_that_are_not_finite(run):
    xyz = run.xyz[:12].copy()
    xyz[0, 0] = np.nan
    xyz[1, 1] = np.inf
    xyz[2, 2] = -np.inf
    xyz[3] = np.nan
    for max_dist in (np.inf, 2.5):
        got = run.hs.closest(rtgpu.make_points(xyz, max_dist))
        bad = got[:4]
        assert (bad["object"] == -1).all() and (bad["face"] == -1).all() and (bad["dist"] == np.float32(max_dist)).all()
        assert not bad["p"].any() and (cu.u32(bad)[:, 3:] == 0).all()
        assert (got["object"][4:] >= 0).sum() >= (8 if max_dist == np.inf else 0)


@pytest.mark.parametrize("name", bc.NAMES)
def test_adversarial_meshes_return(name, tmp_path):
    """Slivers, coincident copies, deep chains, huge and subnormal coordinates: the walk returns,
    answers every finite point of an unbounded query, and repeats itself byte for byte."""
    hs = wc.load(tmp_path, name)
    world = cu.World(hs)
    with np.errstate(all="ignore"):
        xyz = cu.points_for(world, seed=3, total=1500, max_faces=64)
    xyz = xyz[np.isfinite(xyz).all(1)]
    pts = rtgpu.make_points(xyz)
    a = hs.closest(pts)
    b = hs.closest(pts)
    assert a.tobytes() == b.tobytes()
    _, _, meshes, faces = qu.scene_arrays(hs)
    held = a["object"] >= 0
    assert (a["face"][held] >= 0).all() and (a["face"][held] < len(faces)).all()
    assert (a["dist"][held] >= 0).all()
    if name not in bc.UNHITTABLE:
        assert held.all(), (name, int((~held).sum()))


# ---------------------------------------------------------------------------
def _err():
    return rtgpu.lib().rtg_last_error().decode()


def test_argument_errors(tmp_path):
    L = rtgpu.lib()
    hs = cu.load(cu.write_grid(tmp_path))
    pts = rtgpu.make_points(np.zeros((4, 3), np.float32))
    out = np.zeros(4, rtgpu.NEAREST_DTYPE)
    f = L.rtg_desc_closest_points
    assert f(hs.desc, pts.ctypes.data, 4, 0, out.ctypes.data) == 0
    for flags in (1, 2, 0x80000000):
        assert f(hs.desc, pts.ctypes.data, 4, flags, out.ctypes.data) == -1 and "flags" in _err()
    assert f(hs.desc, pts.ctypes.data, -1, 0, out.ctypes.data) == -1
    assert f(hs.desc, pts.ctypes.data, 1 << 31, 0, out.ctypes.data) == -1
    assert f(hs.desc, None, 4, 0, out.ctypes.data) == -1 and "null" in _err()
    assert f(hs.desc, pts.ctypes.data, 4, 0, None) == -1 and "null" in _err()
    assert f(None, pts.ctypes.data, 4, 0, out.ctypes.data) == -1 and "null" in _err()
    assert f(hs.desc, None, 0, 0, None) == 0                                       # n = 0: no buffer touched
    assert hs.closest(np.zeros(0, rtgpu.POINT_DTYPE)).shape == (0,)


def test_device_bvh_description_is_refused(tmp_path):
    path = cu.write_grid(tmp_path)
    hs = cu.load(path, device_bvh=True)
    pts = rtgpu.make_points(np.zeros((2, 3), np.float32))
    rays = rtgpu.make_rays(np.zeros((2, 3)), np.ones((2, 3)))
    with pytest.raises(rtgpu.RTGError) as ray_err:
        hs.trace(rays)
    with pytest.raises(rtgpu.RTGError) as err:
        hs.closest(pts)
    assert str(err.value) == str(ray_err.value) and "RTG_LOAD_DEVICE_BVH" in str(err.value)


def test_ellipsoid_is_unsupported(tmp_path):
    """A sphere under a non-uniform scale: RTG_ERR_UNSUPPORTED naming the object, output untouched."""
    hs = cu.load(cu.write_moved(tmp_path, "ellipsoid", sphere_scaling="s1"))
    pts = rtgpu.make_points(np.zeros((3, 3), np.float32))
    out = np.full(3 * 8, 0xA5A5A5A5, np.uint32)
    rc = rtgpu.lib().rtg_desc_closest_points(hs.desc, pts.ctypes.data, 3, 0, out.ctypes.data)
    assert rc == -6 and "object 2" in _err() and "sphere" in _err()
    assert (out == 0xA5A5A5A5).all()
    assert rtgpu.lib().rtg_desc_closest_points(hs.desc, None, 0, 0, None) == -6


# ---------------------------------------------------------------------------
# The placement side table, by behaviour
# ---------------------------------------------------------------------------
def _set_transform(hs, index, M):
    """Overwrite object `index`'s transform / inv_transform in the description (test only)."""
    d = qu.Desc.from_address(hs.desc)
    base = d.objects + index * qu.OBJ_DTYPE.itemsize
    for field, mat in (("transform", M), ("inv_transform", np.linalg.inv(M))):
        off = qu.OBJ_DTYPE.fields[field][1]
        ctypes.memmove(base + off, np.ascontiguousarray(mat, np.float64).ctypes.data, 128)


def test_identity_objects_do_no_transform_arithmetic(tmp_path_factory):
    """IDENTITY and lip2 == 1 by behaviour.  The returned distance of an identity mesh is exactly
    sqrtf(dot(p - c, p - c)) in float32 of the returned point -- no transform rounding in between --
    and the ground mesh of the plain room answers with the same bytes in the room that also holds a
    transformed mesh and an instance (the general walk, which reads the side table per object)."""
    plain = cu.load(write_scene("room_0", tmp_path_factory.mktemp("plain")))
    general = cu.load(write_scene("room_7", tmp_path_factory.mktemp("general")))
    xyz = cu.points_for(cu.World(plain), seed=9)
    pts = rtgpu.make_points(xyz)
    a, b = plain.closest(pts), general.closest(pts)
    both = (a["object"] == 0) & (b["object"] == 0)
    assert both.sum() > 500
    cu.same(a[both], b[both], "the identity ground mesh, plain room against general room")
    for got in (a, b[both]):
        d = np.stack([got["p"][:, k] for k in range(3)], 1)
        d = (xyz if got is a else xyz[both]).astype(np.float32) - d
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32 and np.array_equal(np.sqrt(d2), got["dist"])


def test_similarity_classes(tmp_path):
    """A uniformly scaled and rotated sphere is a sphere of radius r s; a sheared one is refused."""
    hs = cu.load(cu.write_moved(tmp_path))
    _, objs, _, _ = qu.scene_arrays(hs)
    k = 2
    assert objs["kind"][k] == qu.RTG_OBJ_SPHERE and not np.array_equal(objs["transform"][k], np.eye(4).reshape(-1))
    M = objs["transform"][k].reshape(4, 4)
    centre = M[:3, 3] + M[:3, :3] @ objs["center"][k]
    s = abs(np.linalg.det(M[:3, :3])) ** (1 / 3)
    assert abs(s - 1.7) < 1e-6
    # points straight above the scaled sphere, nearer to it than to anything else
    xyz = centre + np.array([[0, 1, 0]]) * np.linspace(0.1, 4.0, 40)[:, None]
    got = hs.closest(rtgpu.make_points(xyz))
    near = got["object"] == k
    assert near.sum() >= 20
    want = np.abs(np.linalg.norm(xyz - centre, axis=1) - 0.75 * s)
    assert (np.abs(got["dist"][near] - want[near]) <= cu.TOL * 8).all()
    shear = np.eye(4)
    shear[0, 1] = 0.3
    _set_transform(hs, k, shear)
    with pytest.raises(rtgpu.RTGError) as err:
        hs.closest(rtgpu.make_points(xyz))
    assert err.value.args and "object 2" in str(err.value)
    # a pure rotation plus translation of the identity sphere is still a similarity
    rot = np.eye(4)
    rot[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    rot[:3, 3] = [1, 2, 3]
    _set_transform(hs, k, rot)
    assert (hs.closest(rtgpu.make_points(xyz))["object"] >= 0).all()
