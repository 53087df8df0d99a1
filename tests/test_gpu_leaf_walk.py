"""The leaf-exact camera packet walk (rtg_walk.hpp walk_bvh_packet_lx: conservative decisions at
inner nodes, the exact one at leaves) against walks it does not touch: the per-lane fused kernel
(RTG_RENDER_FUSED, k_render), the host walk (HostScene.trace) and the oracle; counting renders keep
the walk that is exact at every node and must report the oracle's counters.  Every render case
asserts through ds.timings() that the kernel under test ran.

  height field   200 triangles at 16x8, 37x21 and 131x67: whole, a row band, three parts
  axis camera    a camera looking down -z with odd width and height: the centre column and row have
                 zero direction components (off the fast path) in waves whose other lanes are on it
  one lane       frames of width 1 (1x21: one column of a tile; 1x1: a single live lane)
  fixtures       simple, spheres, transforms_textures and dof_motion without its <MotionBlur> at their
                 golden sizes (plain, sphere, transform and instance variants of the walk's callers)
  large leaves   C3 at 20 000 triangles, 320x180: the deferring form of the walk
  tmax ties      trace(coherent=True) with tmax at the hit distance and one ulp either side
"""
import os
import re

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu
import scenes

pytestmark = pytest.mark.gpu

REL = 1e-4
SCENES = os.path.join(ob.GOLDEN, "scenes")
WALK_STAGES = ("k_frame", "k_primary")      # the timed stages whose kernels run the packet walk
COUNTERS = ("camera_rays", "shadow_rays", "node_visits", "tri_tests")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _load(xml, cwd):
    old = os.getcwd()
    os.chdir(cwd)               # PLY / image paths are relative
    try:
        hs = rtgpu.HostScene(xml)
        return hs, rtgpu.DeviceScene(hs, 0)
    finally:
        os.chdir(old)


def _field(out_dir, w, h, name=None):
    xml = scenes.synthetic_heightfield(str(out_dir), K=200, width=w, height=h, name=name or f"f{w}x{h}")
    return xml, _load(xml, out_dir)


def _stages(ds, flags=0):
    ds.render(0, flags=rtgpu.RTG_RENDER_TIMING | flags)
    return list(ds.timings())


def _check_scene(hs, ds, seed=77, walk=WALK_STAGES, exact=True):
    """The production render against the fused kernel (bit for bit), the counting render (bit for
    bit, the oracle's counters) and the oracle; returns the production frame."""
    st = _stages(ds)
    assert st and st[0] in walk, st
    assert "k_render" in _stages(ds, rtgpu.RTG_RENDER_FUSED)
    hdr, ldr = ds.render(0, seed=seed)
    fh, fl = ds.render(0, seed=seed, flags=rtgpu.RTG_RENDER_FUSED)
    assert np.array_equal(_bits(hdr), _bits(fh)) and np.array_equal(ldr, fl)
    ds.reset_stats()
    ch, _ = ds.render(0, seed=seed, flags=rtgpu.RTG_RENDER_COUNT_STATS)
    got = ds.stats()
    ohdr, _, ost = ob.render(hs, seed=seed)
    assert np.array_equal(_bits(ch), _bits(hdr))
    print(st, {k: (got[k], ost[k]) for k in COUNTERS})
    for k in COUNTERS:
        # (a scene with sampled rays: test_gpu_parity's allowance, a last-ulp difference can move one ray)
        assert got[k] == ost[k] if exact else abs(got[k] - ost[k]) <= max(4, 0.002 * ost[k]), (k, got[k], ost[k])
    r = ob.compare(hdr, ohdr, REL)
    assert r["n_fail"] == 0, r
    return hdr, ldr


@pytest.mark.parametrize("w,h", [(16, 8), (37, 21), (131, 67)])
def test_height_field_whole_band_and_parts(w, h, tmp_path):
    _, (hs, ds) = _field(tmp_path, w, h)
    assert _stages(ds) == ["k_frame"]
    hdr, ldr = _check_scene(hs, ds, walk=("k_frame",))
    fused, _ = ds.render(0, seed=77, flags=rtgpu.RTG_RENDER_FUSED)
    assert (hdr != 0).any(axis=2).all()                       # every pixel was written
    if h >= 19:
        band, _ = ds.render(0, seed=77, rows=(5, 19))
        assert np.array_equal(_bits(band[5:19]), _bits(fused[5:19]))
        assert not _bits(band[:5]).any() and not _bits(band[19:]).any()
    out = (np.zeros_like(hdr), np.zeros_like(ldr))
    for r in range(3):
        ds.render(0, seed=77, part=(r, 3), out=out)
    assert np.array_equal(_bits(out[0]), _bits(fused)) and np.array_equal(out[1], ldr)


def test_axis_aligned_camera_has_zero_components_in_mixed_waves(tmp_path):
    xml, _ = _field(tmp_path, 37, 21, name="axis")
    s = open(xml).read()
    for tag, val in (("Position", "0 0.5 2"), ("Gaze", "0 0 -1"), ("Up", "0 1 0"), ("NearPlane", "-0.5 0.5 -0.5 0.5"),
                     ("NearDistance", "1")):
        s, n = re.subn(rf"<{tag}>[^<]*</{tag}>", f"<{tag}>{val}</{tag}>", s, count=1)
        assert n == 1, tag
    with open(xml, "w") as f:
        f.write(s)
    hs, ds = _load(xml, tmp_path)
    rays = ds.camera_rays()
    d = qu.directions(rays).reshape(21, 37, 3)
    assert (d[:, 18, 0] == 0).all() and (d[10, :, 1] == 0).all()          # the centre column and row
    assert (d[:, :18, 0] != 0).all() and (d[:10, :, 1] != 0).all()         # ... among lanes on the fast path
    hdr, _ = _check_scene(hs, ds, walk=("k_frame",))
    host = hs.trace(rays)
    got = ds.trace(rays, coherent=True)
    assert (host["object"] >= 0).sum() > len(rays) // 2
    for k in ("object", "face"):
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(_bits(got["t"]), _bits(host["t"]))


@pytest.mark.parametrize("w,h", [(1, 21), (1, 1)])
def test_frame_of_width_one(w, h, tmp_path):
    _, (hs, ds) = _field(tmp_path, w, h)
    hdr, _ = _check_scene(hs, ds)               # (1x21 takes the queued layout: k_primary runs the walk)
    assert hdr.shape == (h, w, 3)


def _fixture_xml(name, tmp_path):
    s = open(os.path.join(SCENES, name + ".xml")).read()
    if name == "dof_motion":
        s, n = re.subn(r"\s*<MotionBlur>[^<]*</MotionBlur>", "", s)
        assert n == 3
    raw = tmp_path / (name + "_raw.xml")
    raw.write_text(s)
    return scenes.with_depth(str(raw), str(tmp_path / (name + "_d0.xml")), 0)


@pytest.mark.parametrize("name", ["simple", "spheres", "transforms_textures", "dof_motion"])
def test_fixtures_at_their_golden_sizes(name, tmp_path):
    hs, ds = _load(_fixture_xml(name, tmp_path), SCENES)
    c = hs.camera(0)
    old = os.getcwd()
    os.chdir(SCENES)
    try:
        ref = rtgpu.HostScene(name + ".xml").camera(0)
        assert (c["width"], c["height"]) == (ref["width"], ref["height"])
        kinds = set(qu.scene_arrays(hs)[1]["kind"].tolist())
        if name in ("transforms_textures", "dof_motion"):
            assert qu.RTG_OBJ_INSTANCE in kinds
        if name != "transforms_textures":
            assert qu.RTG_OBJ_SPHERE in kinds
        _check_scene(hs, ds, seed=1234, exact=ob.manifest()[name]["kind"] == "exact")
    finally:
        os.chdir(old)


def test_large_leaves_through_the_deferring_walk(tmp_path, monkeypatch):
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        xml = scenes.config_c3(str(tmp_path), K=20000, width=320, height=180, spp=1)
        xml0 = scenes.with_depth(xml, str(tmp_path / "d0.xml"), 0)
        hs, ds = _load(xml0, tmp_path)
        monkeypatch.setenv("RTG_DEFER_DIAG", "1")
        ds.reset_stats()
        a, la = ds.render(0, seed=9)
        pending = ds.stats()["extend_wide_visits"]
        monkeypatch.delenv("RTG_DEFER_DIAG")
        assert pending > 0, pending                                        # the walk deferred leaves
        st = _stages(ds)
        assert "k_primary" in st, st
        f, lf = ds.render(0, seed=9, flags=rtgpu.RTG_RENDER_FUSED)
        assert np.array_equal(_bits(a), _bits(f)) and np.array_equal(la, lf)
        ds.reset_stats()
        c, _ = ds.render(0, seed=9, flags=rtgpu.RTG_RENDER_COUNT_STATS)
        got = ds.stats()
        _, _, ost = ob.render(hs, seed=9)
        assert np.array_equal(_bits(c), _bits(a))
        for k in ("camera_rays", "node_visits", "tri_tests"):
            assert got[k] == ost[k], (k, got[k], ost[k])
    finally:
        os.chdir(old)


def test_coherent_trace_with_tmax_at_the_hit_distance(tmp_path):
    _, (hs, ds) = _field(tmp_path, 37, 21)
    rays = ds.camera_rays()
    base = hs.trace(rays)
    hit = base["object"] >= 0
    assert hit.sum() > len(rays) // 2
    t = base["t"][hit]
    tm = np.stack([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))], 1)
    q = np.repeat(rays[hit], 3)
    q["tmax"] = tm.reshape(-1)
    want, got = hs.trace(q), ds.trace(q, coherent=True)
    w3 = want["object"].reshape(-1, 3)
    assert (w3[:, 1] >= 0).mean() > 0.99 and (w3[:, 2] < 0).any()          # past the hit: kept; before it: lost
    for k in ("object", "face"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(_bits(got["t"]), _bits(want["t"]))
