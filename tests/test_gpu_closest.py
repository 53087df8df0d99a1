"""Closest-point queries on the device (rtg_closest_points*; rtg_closest.hip) against the host walk
(rtg_desc_closest_points, checked on its own against a float64 brute force in test_closest_host.py):
all 32 bytes of every record, on every traversal variant -- the six rooms, the height field, the
composite transforms -- and on the adversarial meshes of bvh_cases (slivers, coincident copies, deep
chains, huge and subnormal coordinates: what no tolerance covers, bit identity does); partial
blocks and waves, a single point, no point; device buffers on a torch stream; a device-built BVH;
update and clone; and consistency with the ray queries."""
import numpy as np
import pytest

import bvh_cases as bc
import closest_util as cu
import rtgpu
import walk_cases as wc
from test_closest_host import SCENES, write_scene

pytestmark = pytest.mark.gpu

N = 4099                                   # 16 blocks and 3 lanes: a partial last block and wave


def _points(hs, seed, n=N):
    """n points of closest_util.points_for in a seeded shuffle (incoherent lanes), four of them not
    finite; max_dist = inf."""
    world = cu.World(hs)
    with np.errstate(all="ignore"):
        xyz = cu.points_for(world, seed, total=n + 600)
    rng = np.random.default_rng(seed)
    xyz = xyz[rng.permutation(len(xyz))[:n]]
    assert len(xyz) == n
    xyz[5, 0] = np.nan
    xyz[70, 1] = np.inf
    xyz[300, 2] = -np.inf
    xyz[n - 1] = np.nan
    return world, rtgpu.make_points(xyz)


def _with_radii(pts, unbounded, seed):
    """Half of the points with a radius around their own distance (hits and misses), a few with 0,
    a negative one and NaN."""
    rng = np.random.default_rng(seed)
    out = pts.copy()
    d = np.where(np.isfinite(unbounded["dist"]), unbounded["dist"], 1.0)
    r = (d * rng.choice([0.5, 1.0, 1.5], len(d))).astype(np.float32)
    pick = rng.random(len(d)) < 0.5
    out["max_dist"][pick] = r[pick]
    out["max_dist"][11] = 0.0
    out["max_dist"][12] = -3.0
    out["max_dist"][13] = np.nan
    return out


def _check_scene(name, hs, ds, seed):
    _, pts = _points(hs, seed)
    want = hs.closest(pts)
    got = ds.closest(pts)
    cu.same(got, want, (name, "unbounded"))
    assert (want["object"] >= 0).sum() > (0 if name in bc.UNHITTABLE else N // 2), name
    bounded = _with_radii(pts, want, seed)
    want_b = hs.closest(bounded)
    cu.same(ds.closest(bounded), want_b, (name, "radii"))
    one = pts[17:18]
    cu.same(ds.closest(one), hs.closest(one), (name, "n = 1"))
    assert ds.closest(pts[:0]).shape == (0,)
    return pts, want, want_b


@pytest.mark.parametrize("name", SCENES)
def test_device_equals_host_walk(name, tmp_path):
    hs = cu.load(write_scene(name, tmp_path))
    ds = rtgpu.DeviceScene(hs, 0)
    _, want, want_b = _check_scene(name, hs, ds, seed=31)
    miss = want_b["object"] < 0
    assert miss.sum() > 200 and (~miss).sum() > 2000, name


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_equals_host_walk_adversarial(name, tmp_path):
    hs = wc.load(tmp_path, name)
    ds = rtgpu.DeviceScene(hs, 0)
    _check_scene(name, hs, ds, seed=32)


@pytest.mark.parametrize("name", ["grid", "moved", "copies_17", "chain"])
def test_device_built_bvh(name, tmp_path):
    """A scene whose BVH was built on the device answers as the host-built one, bit for bit."""
    if name in bc.CASES:
        hs, hs_dev = wc.load(tmp_path, name), wc.load(tmp_path, name, device_bvh=True)
    else:
        path = write_scene(name, tmp_path)
        hs, hs_dev = cu.load(path), cu.load(path, device_bvh=True)
    _, pts = _points(hs, seed=33)
    want = hs.closest(pts)
    cu.same(rtgpu.DeviceScene(hs_dev, 0).closest(pts), want, (name, "device-built BVH"))
    cu.same(rtgpu.DeviceScene(hs, 0).closest(pts), want, (name, "host-built BVH"))


def test_identity_mesh_same_bits_in_every_variant(tmp_path_factory):
    """Identity objects do no transform arithmetic: the ground mesh answers with the same bytes
    from the plain-mesh kernel and from the general one (the room with a transform and an instance)."""
    plain = cu.load(write_scene("room_0", tmp_path_factory.mktemp("plain")))
    general = cu.load(write_scene("room_7", tmp_path_factory.mktemp("general")))
    _, pts = _points(plain, seed=36)
    a = rtgpu.DeviceScene(plain, 0).closest(pts)
    b = rtgpu.DeviceScene(general, 0).closest(pts)
    both = (a["object"] == 0) & (b["object"] == 0)
    assert both.sum() > 500
    cu.same(a[both], b[both], "plain-mesh variant against the general variant")


def test_device_buffers_on_a_torch_stream(tmp_path):
    """closest_device on torch tensors' pointers on a stream of torch's own gives the bytes of the
    host-buffer entry; the word after record n - 1 is untouched; n = 0 touches nothing."""
    import torch
    hs = cu.load(write_scene("moved", tmp_path))
    ds = rtgpu.DeviceScene(hs, 0)
    _, pts = _points(hs, seed=34)
    want = ds.closest(pts)
    cu.same(want, hs.closest(pts), "host-buffer entry")
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.Stream()
        d_pts = torch.from_numpy(pts.view(np.float32).reshape(N, 4).copy()).to(dev)
        d_out = torch.full((N + 1, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ds.closest_device(d_pts.data_ptr(), 0, d_out.data_ptr(), stream=stream.cuda_stream)
        ds.closest_device(0, 0, 0, stream=stream.cuda_stream)
        stream.synchronize()
        assert (d_out.cpu().numpy() == 0x5A5A5A5A).all()
        ds.closest_device(d_pts.data_ptr(), N, d_out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        out = d_out.cpu().numpy()
    assert out[:N].tobytes() == want.tobytes()
    assert (out[N] == 0x5A5A5A5A).all(), "the canary after record n - 1"


def test_update_and_clone(tmp_path):
    """After update() to the other placement: a fresh scene's answers and the host walk's.  A
    clone made before the update still answers for the old placement."""
    hs = cu.load(cu.write_moved(tmp_path, "moved_a", "a"))
    hs2 = cu.load(cu.write_moved(tmp_path, "moved_b", "b"))
    ds = rtgpu.DeviceScene(hs, 0)
    _, pts = _points(hs, seed=35)
    before = hs.closest(pts)
    cu.same(ds.closest(pts), before, "before")
    old = ds.clone()
    ds.update(hs2)
    want = hs2.closest(pts)
    assert want.tobytes() != before.tobytes(), "the other placement changes nothing"
    cu.same(ds.closest(pts), want, "after update")
    cu.same(rtgpu.DeviceScene(hs2, 0).closest(pts), want, "fresh scene")
    cu.same(old.closest(pts), before, "clone made before the update")
    new = ds.clone()
    ds.update(hs)
    cu.same(ds.closest(pts), before, "back")
    cu.same(new.closest(pts), want, "clone of the updated scene, its source moved back")
    ds.close()
    cu.same(old.closest(pts), before, "clone outliving its source")


@pytest.mark.parametrize("name", ["room_15", "grid", "moved"])
def test_consistent_with_rays(name, tmp_path):
    """The hit point of a ray lies on the surface: closest(o + t d).dist <= 4 * 2^-20 S, S the largest
    coordinate magnitude among the scene's vertices and the point (the point on the ray carries
    its own rounding, that of the ray query's t included, hence the 4).  The rays are the camera's
    pixel-centre rays: deterministic.  Worst on one MI355X: 0.36 / 0.08 / 0.86 of the bound on room_15 /
    grid / moved, the last at grazing hits of the identity sphere, where t carries the error."""
    hs = cu.load(write_scene(name, tmp_path))
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()
    hits = ds.trace(rays)
    ok = hits["object"] >= 0
    assert ok.sum() > 500, (name, int(ok.sum()))
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)[ok].astype(np.float64)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)[ok].astype(np.float64)
    xyz = (o + d * hits["t"][ok].astype(np.float64)[:, None]).astype(np.float32)
    got = ds.closest(rtgpu.make_points(xyz))
    S = cu.scale_of(cu.World(hs), xyz)
    ratio = got["dist"] / (4 * cu.TOL * S)
    print(name, "hit points", len(xyz), "worst dist / (4 * 2^-20 S): %.3f" % ratio.max())
    assert (got["dist"] <= 4 * cu.TOL * S).all(), (name, float(ratio.max()))


def test_argument_errors_device(tmp_path):
    L = rtgpu.lib()
    hs = cu.load(write_scene("grid", tmp_path))
    ds = rtgpu.DeviceScene(hs, 0)
    pts = rtgpu.make_points(np.zeros((4, 3), np.float32))
    out = np.zeros(4, rtgpu.NEAREST_DTYPE)
    f, g = L.rtg_closest_points, L.rtg_closest_points_device

    def err():
        return L.rtg_last_error().decode()

    assert f(ds._s, pts.ctypes.data, 4, 0, out.ctypes.data) == 0
    assert f(ds._s, None, 0, 0, None) == 0 and g(ds._s, None, 0, 0, None, None) == 0
    assert f(ds._s, None, 4, 0, out.ctypes.data) == -1 and "null" in err()
    assert f(ds._s, pts.ctypes.data, 4, 0, None) == -1 and "null" in err()
    assert f(None, pts.ctypes.data, 4, 0, out.ctypes.data) == -1 and "null scene" in err()
    assert g(ds._s, None, 4, 0, None, None) == -1
    assert f(ds._s, pts.ctypes.data, 1 << 31, 0, out.ctypes.data) == -1 and "INT32_MAX" in err()
    assert f(ds._s, pts.ctypes.data, -1, 0, out.ctypes.data) == -1
    for flags in (1, 2, 1 << 31):
        assert f(ds._s, pts.ctypes.data, 4, flags, out.ctypes.data) == -1 and "flags" in err()
        assert g(ds._s, pts.ctypes.data, 4, flags, out.ctypes.data, None) == -1


def test_ellipsoid_is_unsupported_on_the_device(tmp_path):
    """The scene renders and traces; closest-point queries refuse it and touch no buffer -- until
    an update makes the sphere a sphere again."""
    hs = cu.load(cu.write_moved(tmp_path, "ellipsoid", sphere_scaling="s1"))
    ds = rtgpu.DeviceScene(hs, 0)
    assert (ds.trace(ds.camera_rays())["object"] >= 0).any()
    pts = rtgpu.make_points(np.zeros((3, 3), np.float32))
    out = np.full(3 * 8, 0xA5A5A5A5, np.uint32)
    L = rtgpu.lib()
    assert L.rtg_closest_points(ds._s, pts.ctypes.data, 3, 0, out.ctypes.data) == -6
    assert "object 2" in L.rtg_last_error().decode()
    assert (out == 0xA5A5A5A5).all()
    assert L.rtg_closest_points_device(ds._s, None, 0, 0, None, None) == -6
    hs2 = cu.load(cu.write_moved(tmp_path, "sphere_again"))
    ds.update(hs2)
    cu.same(ds.closest(pts), hs2.closest(pts), "after the update")
