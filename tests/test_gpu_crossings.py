"""Crossing counts and signed distances on the device (rtg_count_crossings*,
rtg_signed_distance_points*; rtg_crossings.hip) against the host walks (rtg_desc_count_crossings,
rtg_desc_signed_distance_points, checked on their own in test_crossings_host.py): every byte of
every record, on all six traversal sets (the rooms of variant_scenes.py), the layered scene with
its exact ties and 19 hits a ray, the closed shapes, the closest tests' height field and composite
transforms, and the adversarial meshes of bvh_cases; partial waves and blocks, a single ray, none;
tmax infinite, finite, zero, negative and NaN, a NaN direction, points that are not finite; the
multi-hit counts; a device-built BVH; device buffers on a torch stream; update and clone; the
argument errors and the ellipsoid refusal."""
import os

import numpy as np
import pytest

import bvh_cases as bc
import closest_util as cu
import multihit_scenes as ms
import oracle_bind as ob
import rtgpu
import sdf_scenes as sd
import variant_scenes as zoo
import walk_cases as wc
from test_closest_host import ROOM_FEATS, write_scene
from test_gpu_closest import _points
from test_kernel_variants import TRAV_SETS, trav_ladder

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 257, 4099)                 # no multiple of 64 or 256
N = SIZES[-1]
NAMES = ["layered", "closed", "grid", "moved"] + ["room_%d" % f for f in ROOM_FEATS]
UP = (0.0, 1.0, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(os.path.join(ob.GOLDEN, "scenes"))
    yield
    os.chdir(old)


def _host(name, directory, device_bvh=False):
    if name == "layered":
        return rtgpu.HostScene(ms.write_layered(directory), device_bvh=device_bvh)
    if name == "closed":
        return sd.load_closed(directory, device_bvh=device_bvh)
    if name in bc.CASES:
        return wc.load(directory, name, device_bvh=device_bvh)
    return cu.load(write_scene(name, directory), device_bvh=device_bvh)


def _odd(rays):
    """The first rays of a set given every kind of tmax and, one of them, a NaN direction."""
    rays = rays.copy()
    if rays.size >= 64:
        finite = np.isfinite(rays["tmax"])
        rays["tmax"][8:16] = np.where(finite[8:16], rays["tmax"][8:16], 3.0)
        rays["tmax"][16:20] = 0.0
        rays["tmax"][20:24] = -1.0
        rays["tmax"][24:28] = np.nan
        rays["tmax"][28:40] = np.inf
        rays["dy"][40] = np.nan
    return rays


def _rays(hs, seed, n=N):
    """n seeded rays through the scene's box, unbounded and bounded, with a motion-blur time; half
    of them aimed at a vertex of the scene."""
    rng = np.random.default_rng(seed)
    v = cu.World(hs).vertices()
    lo, hi = v.min(0), v.max(0)
    size = np.maximum(hi - lo, 1e-3)
    o = rng.uniform(lo - size / 2, hi + size / 2, (n, 3))
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < 0.5
    d[aim] = v[rng.integers(0, len(v), int(aim.sum()))] - o[aim]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.05, 1.5, n) * np.linalg.norm(size))
    rays = rtgpu.make_rays(o, d, tmax=tmax, time=rng.random(n))
    rays["time"] = np.minimum(rays["time"], np.float32(1.0) - np.float32(2.0 ** -24))
    return _odd(rays)


def _same_c(got, want, what):
    bad = np.flatnonzero((got["count"] != want["count"]) | (got["entering"] != want["entering"]))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _check_crossings(name, hs, ds, sets):
    most = 0
    for label, rays in sets.items():
        want = hs.crossings(rays)
        for n in SIZES:
            if n <= rays.size:
                _same_c(ds.crossings(rays[:n]), want[:n], (name, label, n))
        _same_c(ds.crossings(rays, coherent=True), want, (name, label, "coherent"))
        # the multi-hit walk's own counts
        _, cnt = ds.trace_multi(rays, 8, counts=True)
        below = cnt < 8
        assert np.array_equal(want["count"][below], cnt[below]) and np.all(want["count"][~below] >= 8), (name, label)
        most = max(most, int(want["count"].max()))
    assert ds.crossings(np.zeros(0, rtgpu.RAY_DTYPE)).shape == (0,)
    return most


def _check_signed(name, hs, ds, pts, directions=(None, UP)):
    first = None
    for direction in directions:
        want = hs.signed_distance(pts, direction)
        for n in SIZES:
            cu.same(ds.signed_distance(pts[:n], direction), want[:n], (name, direction, n))
        first = want if first is None else first
    assert ds.signed_distance(pts[:0]).shape == (0,)
    return first


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_walk(name, tmp_path):
    hs = _host(name, tmp_path)
    ds = rtgpu.DeviceScene(hs, 0)
    sets = {"random": _rays(hs, seed=41), "camera": _odd(ds.camera_rays())}
    if name == "layered":
        sets["axis"] = ms.axis_rays(ms.axis_points(257, seed=12))
        sets["slanted"] = _odd(ms.slanted_rays(4096, seed=20253))
    most = _check_crossings(name, hs, ds, sets)
    print(name, "largest count", most)
    assert most >= (19 if name == "layered" else 1), name
    _, pts = _points(hs, seed=42)
    want = _check_signed(name, hs, ds, pts)
    if name == "closed":
        xyz = sd.closed_points(hs, N, seed=43)
        got = ds.signed_distance(rtgpu.make_points(xyz))
        cu.same(got, hs.signed_distance(rtgpu.make_points(xyz)), (name, "uniform points"))
        neg = np.signbit(got["dist"])
        assert neg.sum() > 300 and (~neg).sum() > 2000
    assert (want["object"] >= 0).sum() > N // 2 and (want["pad0"] > 0).any(), name


def test_the_rooms_cover_every_traversal_set():
    """The six rooms are launched above; their feature bits (variant_scenes.expected_bits, which
    test_variant_zoo_host.py holds the scene tables to) select all six instantiations."""
    feats = {trav_ladder(zoo.expected_bits(zoo._feat_switches(f))[1]) for f in ROOM_FEATS}
    assert feats == TRAV_SETS
    assert all("room_%d" % f in NAMES for f in ROOM_FEATS)


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_equals_host_walk_adversarial(name, tmp_path):
    hs = _host(name, tmp_path)
    ds = rtgpu.DeviceScene(hs, 0)
    with np.errstate(all="ignore"):
        rays, _ = wc.ray_sets(hs, name)
        rays = rays[np.random.default_rng(44).permutation(rays.size)[:N]]
        most = _check_crossings(name, hs, ds, {"walk_cases": rays})
        _, pts = _points(hs, seed=45)
        _check_signed(name, hs, ds, pts, directions=(None,))
    if name.startswith("copies_"):
        assert most == int(name.split("_")[1]), (name, most)      # every coincident copy counted


@pytest.mark.parametrize("name", ["closed", "grid", "moved", "copies_17"])
def test_device_built_bvh(name, tmp_path):
    hs, hs_dev = _host(name, tmp_path), _host(name, tmp_path, device_bvh=True)
    ds = rtgpu.DeviceScene(hs_dev, 0)
    rays = _rays(hs, seed=46)
    _same_c(ds.crossings(rays), hs.crossings(rays), (name, "device-built BVH"))
    _, pts = _points(hs, seed=47)
    cu.same(ds.signed_distance(pts), hs.signed_distance(pts), (name, "device-built BVH"))


def test_device_buffers_on_a_torch_stream(tmp_path):
    """The *_device entry points on torch tensors' pointers on a stream of torch's own give the
    bytes of the synchronous calls; the words after the last record are untouched; n = 0 touches
    nothing."""
    import torch
    hs = _host("closed", tmp_path)
    ds = rtgpu.DeviceScene(hs, 0)
    rays = _rays(hs, seed=48)
    _, pts = _points(hs, seed=49)
    want_c = ds.crossings(rays)
    want_s = ds.signed_distance(pts, UP)
    _same_c(want_c, hs.crossings(rays), "host-buffer entry")
    cu.same(want_s, hs.signed_distance(pts, UP), "host-buffer entry")
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.Stream()
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(N, 8).copy()).to(dev)
        d_pts = torch.from_numpy(pts.view(np.float32).reshape(N, 4).copy()).to(dev)
        d_c = torch.full((N + 1, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_s = torch.full((N + 1, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ds.crossings_device(d_rays.data_ptr(), 0, d_c.data_ptr(), stream=stream.cuda_stream)
        ds.crossings_device(0, 0, 0, stream=stream.cuda_stream)
        ds.signed_distance_device(d_pts.data_ptr(), 0, d_s.data_ptr(), stream=stream.cuda_stream)
        ds.signed_distance_device(0, 0, 0, stream=stream.cuda_stream)
        stream.synchronize()
        assert (d_c.cpu().numpy() == 0x5A5A5A5A).all() and (d_s.cpu().numpy() == 0x5A5A5A5A).all()
        ds.crossings_device(d_rays.data_ptr(), N, d_c.data_ptr(), stream=stream.cuda_stream, coherent=True)
        ds.signed_distance_device(d_pts.data_ptr(), N, d_s.data_ptr(), direction=UP, stream=stream.cuda_stream)
        stream.synchronize()
        out_c, out_s = d_c.cpu().numpy(), d_s.cpu().numpy()
    assert out_c[:N].tobytes() == want_c.tobytes() and out_s[:N].tobytes() == want_s.tobytes()
    assert (out_c[N] == 0x5A5A5A5A).all() and (out_s[N] == 0x5A5A5A5A).all(), "the canaries after record n - 1"


def test_update_and_clone(tmp_path):
    """After update() to the other placement: a fresh scene's answers and the host walk's.  A
    clone made before the update still answers for the old placement."""
    hs = cu.load(cu.write_moved(tmp_path, "moved_a", "a"))
    hs2 = cu.load(cu.write_moved(tmp_path, "moved_b", "b"))
    ds = rtgpu.DeviceScene(hs, 0)
    rays = _rays(hs, seed=50)
    _, pts = _points(hs, seed=51)
    before_c, before_s = hs.crossings(rays), hs.signed_distance(pts)
    _same_c(ds.crossings(rays), before_c, "before")
    cu.same(ds.signed_distance(pts), before_s, "before")
    old = ds.clone()
    ds.update(hs2)
    want_c, want_s = hs2.crossings(rays), hs2.signed_distance(pts)
    assert want_c.tobytes() != before_c.tobytes() and want_s.tobytes() != before_s.tobytes()
    _same_c(ds.crossings(rays), want_c, "after update")
    cu.same(ds.signed_distance(pts), want_s, "after update")
    fresh = rtgpu.DeviceScene(hs2, 0)
    _same_c(fresh.crossings(rays), want_c, "fresh scene")
    cu.same(fresh.signed_distance(pts), want_s, "fresh scene")
    _same_c(old.crossings(rays), before_c, "clone made before the update")
    cu.same(old.signed_distance(pts), before_s, "clone made before the update")
    ds.close()
    cu.same(old.signed_distance(pts), before_s, "clone outliving its source")


def test_argument_errors_device(tmp_path):
    L = rtgpu.lib()
    hs = _host("grid", tmp_path)
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()[:4]
    out = np.zeros(4, rtgpu.CROSSINGS_DTYPE)
    f, g = L.rtg_count_crossings, L.rtg_count_crossings_device

    def err():
        return L.rtg_last_error().decode()

    assert f(ds._s, rays.ctypes.data, 4, 0, out.ctypes.data) == 0
    assert f(ds._s, None, 0, 0, None) == 0 and g(ds._s, None, 0, 0, None, None) == 0
    assert f(ds._s, None, 4, 0, out.ctypes.data) == -1 and "null" in err()
    assert f(ds._s, rays.ctypes.data, 4, 0, None) == -1 and "null" in err()
    assert f(None, rays.ctypes.data, 4, 0, out.ctypes.data) == -1 and "null scene" in err()
    assert g(ds._s, None, 4, 0, None, None) == -1
    assert f(ds._s, rays.ctypes.data, 1 << 31, 0, out.ctypes.data) == -1 and "INT32_MAX" in err()
    assert f(ds._s, rays.ctypes.data, 4, rtgpu.RTG_QUERY_ANY_HIT, out.ctypes.data) == -1 and "RTG_QUERY_ANY_HIT" in err()
    assert f(ds._s, rays.ctypes.data, 4, 8, out.ctypes.data) == -1 and "unknown query flags" in err()
    assert g(ds._s, rays.ctypes.data, 4, 8, out.ctypes.data, None) == -1

    pts = rtgpu.make_points(np.zeros((4, 3), np.float32))
    res = np.zeros(4, rtgpu.NEAREST_DTYPE)
    f, g = L.rtg_signed_distance_points, L.rtg_signed_distance_points_device
    assert f(ds._s, pts.ctypes.data, 4, None, 0, res.ctypes.data) == 0
    assert f(ds._s, None, 0, None, 0, None) == 0 and g(ds._s, None, 0, None, 0, None, None) == 0
    assert f(ds._s, None, 4, None, 0, res.ctypes.data) == -1 and "null" in err()
    assert f(ds._s, pts.ctypes.data, 4, None, 0, None) == -1 and "null" in err()
    assert f(None, pts.ctypes.data, 4, None, 0, res.ctypes.data) == -1 and "null scene" in err()
    assert g(ds._s, None, 4, None, 0, None, None) == -1
    assert f(ds._s, pts.ctypes.data, 1 << 31, None, 0, res.ctypes.data) == -1 and "INT32_MAX" in err()
    for flags in (1, 2, 1 << 31):
        assert f(ds._s, pts.ctypes.data, 4, None, flags, res.ctypes.data) == -1 and "flags" in err()
        assert g(ds._s, pts.ctypes.data, 4, None, flags, res.ctypes.data, None) == -1
    for bad in ([np.nan, 0, 1], [0, -np.inf, 0], [0, 0, 0]):
        b = np.array(bad, np.float32)
        assert f(ds._s, pts.ctypes.data, 4, b.ctypes.data, 0, res.ctypes.data) == -1 and "dir" in err(), bad
        assert g(ds._s, pts.ctypes.data, 4, b.ctypes.data, 0, res.ctypes.data, None) == -1, bad
        assert g(ds._s, None, 0, b.ctypes.data, 0, None, None) == -1, bad


def test_ellipsoid_is_unsupported_on_the_device(tmp_path):
    """Signed distances refuse the scene as closest-point queries do, for every n, and touch no
    buffer; crossing counts take it."""
    hs = cu.load(cu.write_moved(tmp_path, "ellipsoid", sphere_scaling="s1"))
    ds = rtgpu.DeviceScene(hs, 0)
    pts = rtgpu.make_points(np.zeros((3, 3), np.float32))
    out = np.full(3 * 8, 0xA5A5A5A5, np.uint32)
    L = rtgpu.lib()
    assert L.rtg_signed_distance_points(ds._s, pts.ctypes.data, 3, None, 0, out.ctypes.data) == -6
    assert "object 2" in L.rtg_last_error().decode()
    assert (out == 0xA5A5A5A5).all()
    assert L.rtg_signed_distance_points_device(ds._s, None, 0, None, 0, None, None) == -6
    rays = _rays(hs, seed=52)
    _same_c(ds.crossings(rays), hs.crossings(rays), "crossings on the ellipsoid scene")
    hs2 = cu.load(cu.write_moved(tmp_path, "sphere_again"))
    ds.update(hs2)
    cu.same(ds.signed_distance(pts), hs2.signed_distance(pts), "after the update")
