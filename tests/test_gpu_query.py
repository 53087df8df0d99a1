"""Ray queries on the device (rtg_trace_rays*, rtg_camera_rays*; rtg_query.hip) against the host
walk (rtg_desc_trace_rays, checked on its own in test_query_host.py): bit for bit, on every
traversal variant the library ships -- plain meshes, spheres, transforms and nested instances,
motion blur, an emissive mesh, large leaves -- for coherent and incoherent rays, partial waves and
partial blocks, with and without the coherence hint."""
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = ["simple", "spheres", "synth_10k", "transforms_textures", "dof_motion", "mesh_light", "defer_gate"]


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def _load(name, tmp_path):
    """(HostScene, DeviceScene); `defer_gate` is generated (large leaves: FEAT_BIGLEAF)."""
    if name != "defer_gate":
        hs = rtgpu.HostScene(name + ".xml")
        return hs, rtgpu.DeviceScene(hs, 0)
    import scenes
    xml = scenes.config_defer_gate(str(tmp_path))
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        hs = rtgpu.HostScene(xml)
        return hs, rtgpu.DeviceScene(hs, 0)
    finally:
        os.chdir(old)


def _ray_sets(ds, rng):
    """The ray sets of one scene, all from one seeded generator."""
    cam = ds.camera_rays()                                  # coherent
    perm = cam[rng.permutation(cam.size)]                   # the same rays, incoherent
    # the scene box: the camera and everything its rays see
    hits = ds.host.trace(cam)
    hit = hits["object"] >= 0
    p = qu.origins(cam)[hit] + qu.directions(cam)[hit] * hits["t"][hit][:, None]
    lo = np.minimum(p.min(0), qu.origins(cam).min(0))
    hi = np.maximum(p.max(0), qu.origins(cam).max(0))
    n = 4096
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    diag = float(np.linalg.norm(hi - lo))
    rnd = rtgpu.make_rays(rng.uniform(lo, hi, (n, 3)), d, tmax=rng.uniform(0.05, 1.0, n) * diag, time=rng.random(n))
    rnd["time"] = np.minimum(rnd["time"], np.float32(1.0) - np.float32(2.0 ** -24))      # [0, 1) in float32
    sets = {"camera": cam, "permuted": perm, "random": rnd}
    for k in (1, 63, 65, 257):                              # partial waves and partial blocks
        sets[f"n{k}"] = perm[:k]
        sets[f"n{k}r"] = rnd[:k]
    return sets


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_walk(name, tmp_path):
    hs, ds = _load(name, tmp_path)
    rng = np.random.default_rng(20251)
    total = 0
    for label, rays in _ray_sets(ds, rng).items():
        h_hits, h_nrm = hs.trace(rays, normals=True)
        h_occ = hs.trace(rays, any_hit=True)["object"]
        for coherent in (False, True):
            hits = ds.trace(rays, coherent=coherent)
            hits2, nrm = ds.trace(rays, coherent=coherent, normals=True)
            occ = ds.trace(rays, any_hit=True, coherent=coherent)["object"]
            # t, object, face as raw bytes (the pad word is zero on both sides)
            bad = np.flatnonzero((hits.view(np.uint32).reshape(-1, 4) != h_hits.view(np.uint32).reshape(-1, 4)).any(1))
            assert bad.size == 0, (name, label, coherent, bad[:8], hits[bad[:8]], h_hits[bad[:8]])
            assert hits2.tobytes() == hits.tobytes(), (name, label, coherent)
            assert np.array_equal(nrm.view(np.uint32), h_nrm.view(np.uint32)), (name, label, coherent)
            assert set(np.unique(occ)) <= {0, -1}
            assert np.array_equal(occ, h_occ), (name, label, coherent, np.flatnonzero(occ != h_occ)[:8])
            total += rays.size
        if label in ("camera", "random"):
            print(name, label, "rays", rays.size, "hits", int((h_hits["object"] >= 0).sum()), "occluded",
                  int((h_occ == 0).sum()))
            assert (h_hits["object"] >= 0).any()
    assert total > 0


def test_camera_rays_pixel_centre():
    """`simple` (no depth of field): camera_rays() equals the NumPy pixel-centre rays bit for
    bit, whatever the sample index and seed; a row range is the matching slice."""
    hs = rtgpu.HostScene("simple.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    cam = qu.camera_record(hs)
    ref = qu.numpy_camera_rays(cam)
    got = ds.camera_rays(sample=3, seed=99)
    for f in ("ox", "oy", "oz", "tmax", "dx", "dy", "dz"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    assert np.all((got["time"] >= 0) & (got["time"] < 1))
    w = cam["width"]
    part = ds.camera_rays(rows=(5, 12), sample=3, seed=99)
    assert part.tobytes() == got[5 * w:12 * w].tobytes()


def test_camera_rays_agree_with_render():
    """`dof_motion` (depth of field, motion blur): camera_rays() then trace() misses exactly
    where a 1-sample fused render at the same seed shows the background."""
    hs = rtgpu.HostScene("dof_motion.xml")
    assert hs.camera(0)["spp"] == 1
    ds = rtgpu.DeviceScene(hs, 0)
    seed = 0xC0FFEE
    rays = ds.camera_rays(seed=seed)
    assert len(np.unique(rays["ox"])) > 1 and len(np.unique(rays["time"])) > 1      # the draws are in
    hits = ds.trace(rays, coherent=True)
    hdr, _ = ds.render(0, flags=rtgpu.RTG_RENDER_FUSED, seed=seed)
    bg = qu.scene_arrays(hs)[0].astype(np.float32)
    is_bg = (hdr == bg[None, None, :]).all(axis=2).reshape(-1)
    miss = hits["object"] < 0
    print("dof_motion pixels", miss.size, "misses", int(miss.sum()), "disagreeing", int((miss != is_bg).sum()))
    assert 0 < miss.sum() < miss.size
    assert np.array_equal(miss, is_bg)


def test_torch_plumbing():
    """trace_device / camera_rays_device on torch tensors' pointers on the current stream give
    the bytes of the host-buffer path."""
    import torch
    hs = rtgpu.HostScene("transforms_textures.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()
    n = rays.size
    want_hits, want_nrm = ds.trace(rays, normals=True)
    want_occ = ds.trace(rays, any_hit=True)
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        d_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        d_hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d_occ = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d_nrm = torch.full((n, 4), 7.0, dtype=torch.float32, device=dev)
        ds.camera_rays_device(d_rays.data_ptr(), stream=stream.cuda_stream)
        ds.trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_nrm.data_ptr(), stream=stream.cuda_stream,
                        flags=rtgpu.RTG_QUERY_COHERENT)
        ds.trace_device(d_rays.data_ptr(), n, d_occ.data_ptr(), stream=stream.cuda_stream,
                        flags=rtgpu.RTG_QUERY_ANY_HIT)
        stream.synchronize()
        assert d_rays.cpu().numpy().tobytes() == rays.tobytes()
        assert d_hits.cpu().numpy().tobytes() == want_hits.tobytes()
        assert d_nrm.cpu().numpy().tobytes() == want_nrm.tobytes()
        assert np.array_equal(d_occ.cpu().numpy()[:, 1], want_occ["object"])


def test_render_unchanged_by_queries():
    """A render, 1 000 queries and a second render give identical images."""
    hs = rtgpu.HostScene("transforms_textures.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    hdr0, ldr0 = ds.render(0)
    rays = ds.camera_rays()[:2048]
    first = ds.trace(rays)
    for k in range(1000):
        hits = ds.trace(rays, any_hit=bool(k & 1), coherent=bool(k & 2), normals=(k % 5 == 0))
    assert ds.trace(rays).tobytes() == first.tobytes()
    hdr1, ldr1 = ds.render(0)
    assert hdr0.tobytes() == hdr1.tobytes() and ldr0.tobytes() == ldr1.tobytes()
    assert hits is not None


def test_argument_errors_device():
    L = rtgpu.lib()
    hs = rtgpu.HostScene("simple.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()[:4]
    hits = np.zeros(4, rtgpu.HIT_DTYPE)
    assert ds.trace(np.zeros(0, rtgpu.RAY_DTYPE)).size == 0                     # n = 0
    assert L.rtg_trace_rays(ds._s, None, 4, 0, hits.ctypes.data, None) == -1
    assert L.rtg_trace_rays(ds._s, rays.ctypes.data, 4, 0, None, None) == -1
    assert L.rtg_trace_rays(ds._s, rays.ctypes.data, 1 << 31, 0, hits.ctypes.data, None) == -1
    assert L.rtg_trace_rays_device(ds._s, None, 4, 0, None, None, None) == -1
    assert L.rtg_trace_rays_device(ds._s, None, 0, 0, None, None, None) == 0
    assert L.rtg_trace_rays(None, rays.ctypes.data, 4, 0, hits.ctypes.data, None) == -1
    assert L.rtg_camera_rays(ds._s, None, None) == -1
    assert ds.trace(rays).size == 4
