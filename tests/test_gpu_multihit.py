"""Multi-hit ray queries on the device (rtg_trace_rays_multi*; rtg_multihit.hip) against the host
walk (rtg_desc_trace_rays_multi, checked on its own in test_multihit_host.py): hits and counts bit
for bit, on every traversal variant -- plain meshes, spheres, transforms and nested instances,
motion blur, an emissive mesh, large leaves, the layered scene with its exact ties -- for every
list size (k below and equal to each of the kernel's 2, 4 and 8 slots), coherent and incoherent
rays, partial waves and partial blocks, with and without the coherence hint."""
import os

import numpy as np
import pytest

import multihit_scenes as ms
import oracle_bind as ob
import rtgpu
import scene_variants as sv
from test_gpu_query import NAMES as QUERY_NAMES
from test_gpu_query import _load, _ray_sets

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = QUERY_NAMES + ["layered"]
KS = (1, 2, 3, 4, 5, 8)


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def _scene(name, tmp_path):
    if name != "layered":
        return _load(name, tmp_path)
    hs = ms.load_layered(tmp_path)
    return hs, rtgpu.DeviceScene(hs, 0)


def _same(got, want, what):
    """(n, k) hit arrays as raw words (the pad word is zero on both sides)."""
    g, w = (a.view(np.uint32).reshape(a.shape[0], -1) for a in (got, want))
    bad = np.flatnonzero((g != w).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_walk(name, tmp_path):
    hs, ds = _scene(name, tmp_path)
    sets = _ray_sets(ds, np.random.default_rng(20254))
    if name == "layered":
        sets["axis"] = ms.axis_rays(ms.axis_points(257, seed=12))
        sets["slanted"] = ms.slanted_rays(4096, seed=20253)
    held = 0
    for label, rays in sets.items():
        closest = ds.trace(rays)
        for k in KS:
            want, want_cnt = hs.trace_multi(rays, k, counts=True)
            for coherent in (False, True):
                got, cnt = ds.trace_multi(rays, k, coherent=coherent, counts=True)
                _same(got, want, (name, label, k, coherent))
                assert np.array_equal(cnt, want_cnt), (name, label, k, coherent)
                assert ds.trace_multi(rays, k, coherent=coherent).tobytes() == got.tobytes()      # counts = NULL
            if k == 1:
                _same(got, closest.reshape(-1, 1), (name, label, "k = 1 against trace()"))
            held = max(held, int(want_cnt.max()))
        if label in ("camera", "random"):
            print(name, label, "rays", rays.size, "mean hits held of 8:", float(want_cnt.mean()))
    assert held >= (8 if name == "layered" else 1), name


def test_update_and_clone(tmp_path):
    """After update() to a description with objects moved, and on a clone() of it: the host walk
    on the new description."""
    name = "transforms_textures"
    with sv.in_scenes():
        hs = rtgpu.HostScene(sv.golden(name))
        hs2 = rtgpu.HostScene(sv.variant(name, tmp_path, sv.PAIRS[name]))
        ds = rtgpu.DeviceScene(hs, 0)
        rays = ds.camera_rays()
        before = ds.trace_multi(rays, 4)
        _same(before, hs.trace_multi(rays, 4), "before")
        ds.update(hs2)
        rays2 = ds.camera_rays()
        want = hs2.trace_multi(rays2, 4)
        assert want.tobytes() != hs.trace_multi(rays2, 4).tobytes(), "the variant changes nothing"
        _same(ds.trace_multi(rays2, 4), want, "after update")
        c = ds.clone()
        _same(c.trace_multi(rays2, 4), want, "clone")
        ds.update(hs)
        _same(ds.trace_multi(rays, 4), before, "back")
        _same(c.trace_multi(rays2, 4), want, "clone after its source moved back")
        ds.close()
        _same(c.trace_multi(rays2, 8), hs2.trace_multi(rays2, 8), "clone outliving its source")


def test_torch_plumbing():
    """trace_multi_device on torch tensors' pointers on the current stream gives the bytes of the
    host-buffer path; counts_ptr = 0 is accepted."""
    import torch
    hs = rtgpu.HostScene("transforms_textures.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()
    n, k = rays.size, 3
    want, want_cnt = ds.trace_multi(rays, k, counts=True)
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).to(dev)
        d_hits = torch.zeros((n, k, 4), dtype=torch.int32, device=dev)
        d_hits2 = torch.zeros((n, k, 4), dtype=torch.int32, device=dev)
        d_cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
        ds.trace_multi_device(d_rays.data_ptr(), n, k, d_hits.data_ptr(), d_cnt.data_ptr(), stream=stream.cuda_stream)
        ds.trace_multi_device(d_rays.data_ptr(), n, k, d_hits2.data_ptr(), stream=stream.cuda_stream,
                              flags=rtgpu.RTG_QUERY_COHERENT)
        stream.synchronize()
        assert d_hits.cpu().numpy().tobytes() == want.tobytes()
        assert d_hits2.cpu().numpy().tobytes() == want.tobytes()
        assert np.array_equal(d_cnt.cpu().numpy(), want_cnt)


def test_render_unchanged_by_queries():
    """A render, 200 multi-hit queries and a second render give identical images."""
    hs = rtgpu.HostScene("transforms_textures.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    hdr0, ldr0 = ds.render(0)
    rays = ds.camera_rays()[:2048]
    first = ds.trace_multi(rays, 8)
    for i in range(200):
        hits = ds.trace_multi(rays, 1 + i % 8, coherent=bool(i & 8), counts=bool(i & 16))
    assert ds.trace_multi(rays, 8).tobytes() == first.tobytes()
    hdr1, ldr1 = ds.render(0)
    assert hdr0.tobytes() == hdr1.tobytes() and ldr0.tobytes() == ldr1.tobytes()
    assert hits is not None


def test_argument_errors_device():
    L = rtgpu.lib()
    hs = rtgpu.HostScene("simple.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()[:4]
    hits = np.zeros((4, 8), rtgpu.HIT_DTYPE)
    f, g = L.rtg_trace_rays_multi, L.rtg_trace_rays_multi_device

    def err():
        return L.rtg_last_error().decode()

    assert ds.trace_multi(np.zeros(0, rtgpu.RAY_DTYPE), 2).shape == (0, 2)                  # n = 0
    assert g(ds._s, None, 0, 2, 0, None, None, None) == 0
    assert f(ds._s, None, 4, 2, 0, hits.ctypes.data, None) == -1 and "null" in err()
    assert f(ds._s, rays.ctypes.data, 4, 2, 0, None, None) == -1 and "null" in err()
    assert f(None, rays.ctypes.data, 4, 2, 0, hits.ctypes.data, None) == -1 and "null scene" in err()
    assert g(ds._s, None, 4, 2, 0, None, None, None) == -1
    assert f(ds._s, rays.ctypes.data, 1 << 31, 2, 0, hits.ctypes.data, None) == -1 and "INT32_MAX" in err()
    for k in (0, -1, 9):
        assert f(ds._s, rays.ctypes.data, 4, k, 0, hits.ctypes.data, None) == -1 and "k = %d" % k in err()
        assert g(ds._s, rays.ctypes.data, 4, k, 0, hits.ctypes.data, None, None) == -1
    assert f(ds._s, rays.ctypes.data, 4, 2, rtgpu.RTG_QUERY_ANY_HIT, hits.ctypes.data, None) == -1
    assert "RTG_QUERY_ANY_HIT" in err()
    assert f(ds._s, rays.ctypes.data, 4, 2, 8, hits.ctypes.data, None) == -1 and "unknown query flags" in err()
    assert ds.trace_multi(rays, 8).shape == (4, 8)
