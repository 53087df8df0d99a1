"""The device work buffers behind the render paths and the host-buffer queries (csrc/rtg_devmem.hpp
DevBuf / PinnedBuf; csrc/work_layout.hpp): each owner grown, left larger than the next request needs,
and grown again inside one scene.  Every answer is compared bit for bit with one that does not
depend on the buffers' history: a fresh scene's whole-frame render, the fused kernel's, the host
walk's, or the device-buffer entry point's.  The fixtures render at their own small sizes.
"""
import os

import numpy as np
import pytest

import oracle_bind as ob
import rtgpu

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
FUSED, TREE, COUNT = rtgpu.RTG_RENDER_FUSED, rtgpu.RTG_RENDER_TREE, rtgpu.RTG_RENDER_COUNT_STATS

_whole = {}


@pytest.fixture(autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def whole(name, flags=0):
    """(HostScene, the whole-frame render of a scene created for it alone), once per fixture and flags."""
    if (name, flags) not in _whole:
        hs = rtgpu.HostScene(name + ".xml")
        ds = rtgpu.DeviceScene(hs, 0)
        _whole[name, flags] = (hs, ds.render(0, flags=flags))
        ds.close()
    return _whole[name, flags]


def check_sequence(ds, want, steps, what):
    """Each (rows, flags) render of `ds` equals the same rows of `want` = (hdr, ldr)."""
    for rows, flags in steps:
        hdr, ldr = ds.render(0, rows=rows, flags=flags)
        r0, r1 = rows if rows[1] else (0, want[0].shape[0])
        assert np.array_equal(bits(hdr[r0:r1]), bits(want[0][r0:r1])), (what, rows, flags)
        assert np.array_equal(ldr[r0:r1], want[1][r0:r1]), (what, rows, flags)


def grow_shrink_regrow(height, flags=0):
    r = height // 2
    return [((r, r + 1), flags), ((0, 0), flags), ((r - 2, r + 3), flags), ((0, 0), flags | COUNT)]


@pytest.mark.parametrize("name", ["simple", "windmill"])
def test_wavefront_buffers(name):
    """One light (the one-layout payload) and three lights over large leaves (the general layout
    and the deferred-leaf queue): one row, the frame, five rows, the frame counted."""
    hs, want = whole(name)
    ds = rtgpu.DeviceScene(hs, 0)
    check_sequence(ds, want, grow_shrink_regrow(hs.camera(0)["height"]), name)


@pytest.mark.parametrize("streams", [None, "1"])
def test_ray_tree_buffers(streams, monkeypatch):
    """Levels, segments and the twins of the other streams, against the fused kernel."""
    if streams:
        monkeypatch.setenv("RTG_TREE_STREAMS", streams)
    hs, want = whole("spheres_mirror", FUSED)
    ds = rtgpu.DeviceScene(hs, 0)
    check_sequence(ds, want, grow_shrink_regrow(hs.camera(0)["height"], TREE), streams)


@pytest.mark.parametrize("spp", [1, 4])
def test_path_tracer_buffers(spp, tmp_path):
    """A row range, the frame, the row range again, against the fused kernel."""
    xml = tmp_path / "pt_cornell.xml"
    xml.write_text(ob.with_samples(open(os.path.join(SCENES, "pt_cornell.xml")).read(), spp))
    hs = rtgpu.HostScene(str(xml))
    assert hs.camera(0)["spp"] == spp
    fused = rtgpu.DeviceScene(hs, 0)
    want = fused.render(0, flags=FUSED)
    ds = rtgpu.DeviceScene(hs, 0)
    r = hs.camera(0)["height"] // 2
    check_sequence(ds, want, [((r, r + 3), TREE), ((0, 0), TREE), ((r, r + 3), TREE)], spp)


def test_query_scratch():
    """1, 1 000 and 64 rays through one scene's scratch, then the other kinds of query on it."""
    hs, _ = whole("transforms_textures")
    ds = rtgpu.DeviceScene(hs, 0)
    rays = ds.camera_rays()
    assert rays.size >= 1000
    for n in (1, 1000, 64):
        pick = np.ascontiguousarray(rays[:: rays.size // n][:n])
        hits, nrm = ds.trace(pick, normals=True)
        ref, ref_n = hs.trace(pick, normals=True)
        for k in ("t", "object", "face"):
            assert np.array_equal(bits(hits[k]), bits(ref[k])), (n, k)
        assert np.array_equal(bits(nrm), bits(ref_n)), n
    torch = pytest.importorskip("torch")
    pick = np.ascontiguousarray(rays[:: rays.size // 64][:64])
    d_rays = torch.from_numpy(pick.view(np.uint8).copy()).cuda()
    d_surf = torch.zeros(64 * rtgpu.SURFACE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
    d_rad = torch.zeros((64, 4), dtype=torch.float32, device="cuda:0")
    ds.surface_device(d_rays.data_ptr(), 64, d_surf.data_ptr())
    ds.radiance_device(d_rays.data_ptr(), 64, d_rad.data_ptr())
    torch.cuda.synchronize()
    assert ds.surface(pick).tobytes() == d_surf.cpu().numpy().tobytes()
    assert np.array_equal(bits(ds.radiance(pick)), bits(d_rad.cpu().numpy()))
    # and the first kind again, on scratch the others have used since
    assert ds.trace(pick).tobytes() == hs.trace(pick).tobytes()


def _destruction_order(devices):
    hs, want = whole("simple")
    src = rtgpu.DeviceScene(hs, devices=devices) if len(devices) > 1 else rtgpu.DeviceScene(hs, devices[0])
    a = src.render(0)
    assert np.array_equal(bits(a[0]), bits(want[0])) and np.array_equal(a[1], want[1])
    if len(devices) > 1:        # (a multi-device scene cannot be cloned)
        src.close()
        return
    clone = src.clone()
    src.close()
    b = clone.render(0)
    assert np.array_equal(bits(b[0]), bits(want[0])) and np.array_equal(b[1], want[1])
    clone.close()


def test_destruction_order():
    """Create, render, clone, destroy the source, render the clone, destroy it: the device is
    sound afterwards.  With two devices also a multi-device scene, whose replicas free their
    memory on their own devices."""
    torch = pytest.importorskip("torch")
    _destruction_order([0])
    if rtgpu.device_count() >= 2:
        _destruction_order([0, 1])
    for d in range(min(rtgpu.device_count(), 2)):
        torch.cuda.synchronize(d)      # hipDeviceSynchronize: raises on a device error
