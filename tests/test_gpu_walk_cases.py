"""Every device walk on the adversarial meshes of bvh_cases.py and the walk-only cases of
walk_cases.py (the pinwheels), against yardsticks outside the device: the host walk -- which
test_walk_cases_host.py holds to the reference's recorded answers, to a float64 brute force and to
closed forms on exactly these rays -- for the queries, the CPU oracle for the renders.

Per case, on the host-built scene and on the device-built one (device_bvh=True):

  queries   ds.trace in the six variants of walk_cases.VARIANTS against the host walk's bytes
            (occlusion as the boolean), submitted as test_gpu_edge_rays.py submits: every ray set
            (edge classes A-G, aimed, aimed_short, aimed_long, light, and the pinwheels' axis rays)
            alone, interleaved with the scene's camera rays at one lane and at 32 lanes per 64, and
            partial waves of n = 1, 63, 65, 257.  A set of more than MIX_CAP rays goes whole when
            alone and as a seeded choice of MIX_CAP in the two mixes (one lane per 64 multiplies
            the rays by 64).  ds.trace_multi for k = 1, 2, 8 with and without the coherent hint
            against hs.trace_multi, hits and counts.
  renders   of the case's 64 x 48 scene: default, RTG_FRAME_KERNEL=0, RTG_RENDER_FUSED,
            RTG_RENDER_TREE, RTG_RENDER_EXACT_SHADOW, RTG_AHB=split, RTG_AHB=ref and the
            device-built scene, all identical as uint32 (HDR) and bytes (LDR); the default equal
            to the oracle by test_gpu_parity's criterion; the counted render's camera_rays,
            shadow_rays, node_visits and tri_tests equal to the oracle's.
  pipeline  which one ran, through ds.timings() (stage names as rtg_scene_timings gives them for
            the layout launch_wave_t chose): a scene without a leaf above kBigLeaf = 8 and with
            plain shading is fused, ["k_frame"] (RTG_FRAME_KERNEL=0: ["k_primary",
            "k_shade_shadow"]); with such a leaf (FEAT_BIGLEAF) `fused` is false and the first
            stage is k_primary.  launch_wave_t's deferral of leaves above kDeferLeaf = 16 adds
            kernels inside the k_primary stage and no stage name, so it is observed through the
            pending pixels that k_hitfix counts under RTG_DEFER_DIAG=1, from a camera far enough
            for at most RTG_DEFER_LANES = 16 lanes of a wave to reach the leaf: none for
            copies_8 / 9 / 16, some for copies_17.
  step bound (pinwheels over a floor, walk_cases.load_pinwheel_floor): the counted render's
            shadow_fallbacks is 0 at 8 192 faces and positive, with shadow_wide_visits, at
            49 152, where the axis rays' packets give up after RTG_PK_MAX_STEPS wide nodes; both
            equal the RTG_RENDER_EXACT_SHADOW render bit for bit and the oracle by the parity
            criterion; the floor's patch that the blocker darkens is lit in the open variant and
            dark in the blocked one, pixel by pixel as in the oracle.  The axis occlusion queries
            run in `queries` (they have no counter: the render is what proves the path was taken).

Figures of an MI355X run (all 135 tests pass):

  stage names   copies_8, every spread_<n>, chain, subnormal, several and the pinwheels:
                ["k_frame"] (RTG_FRAME_KERNEL=0: ["k_primary", "k_shade_shadow"]).  copies_9, 16,
                17, 254, 255, 256, 300, nested_256, empty_half (largest leaf 10), huge_empty (12)
                and lattice_uv (its normal map is not plain shading):
                ["k_primary", "k_shade", "k_shadow"], with and without RTG_FRAME_KERNEL=0.
  deferral      pending pixels under RTG_DEFER_DIAG=1 from the far camera (12 pixels hit, 24 with
                the instance): copies_8, 9, 16: 0; copies_17: 16, with the instance 32.
  step bound    (shadow_rays 3 072 each)       wide nodes  shadow_fallbacks  shadow_wide_visits
                pinwheel_8192                       1 366                 0           3 605 256
                pinwheel_8192_blocked               1 087                 0              12 288
                pinwheel_49152                      5 462             2 504          10 339 642
                pinwheel_49152_blocked              5 465                 0              18 432
                (the blocked variants' rays start next to the blocker and meet it in their first
                few nodes; 2 504 is every pixel of the lit patch)
  grazing       the shares of the aimed rays are the host walk's, asserted and listed in
                test_walk_cases_host.py: at most 0.00009 of a case's rays (several).

What the file found on the library as it was: test_multihit[chain] failed for k = 2 on three
class C rays (675, 719, 775 of the case's rays).  Each passes through a vertex shared by dozens of
the chain's faces, which all give the same t; the walk meets two of them and then a nearer face.
k_multihit's list_insert compared the hit it carried up with the next slot again, strictly, so
the earlier of the two tied hits was dropped and the later kept, where hs.trace_multi keeps walk
order.  Fixed in rtg_multihit.hip (everything behind the slot a hit takes moves up unconditionally).

Mutated libraries (one decision each, through RTGPU_LIB), run against this file:

  (a) walk_wide_any_pk's step-bound branch no longer sets `und`: test_step_bound[pinwheel_49152]
      (shadow_fallbacks is 0), test_queries[pinwheel_49152] and [pinwheel_49152_blocked] fail (an
      axis ray that gives up is answered "not occluded"; going down the blocked stack it is occluded).
  (b) the LEAF_EXT branch of walk_bvh_packet_lx takes cnt from the leaf word (255) instead of
      node_ext: test_renders[nested_256] fails (the 256th face is missing from the frame).
      Nothing else does: the queries of a large-leaf scene do not reach this walk
      (test_queries[nested_256] aims eight rays at every face and passes), and on coincident
      copies the first face answers whatever the count.
  (c) walk_bvh_packet's `cnt > kDeferLeaf` turned into `>=`: survived the file's first version
      -- scenes of plain meshes take walk_bvh_packet_lx, which has a comparison of its own, and
      no answer can differ, deferral only moves where a leaf's faces are tested -- and is killed
      by test_copies_at_the_leaf_thresholds[16-instanced], added for it (pending pixels > 0).
"""
import os
import types

import numpy as np
import pytest

import bvh_cases as bc
import edge_rays as er
import oracle_bind as ob
import rtgpu
import walk_cases as wc

pytestmark = pytest.mark.gpu

ALL = bc.NAMES + list(wc.WALK_ONLY)
MIX_CAP = 512
AXIS = 20                                   # the axis rays' label, after walk_cases.SETS
COUNTERS = ("camera_rays", "shadow_rays", "node_visits", "tri_tests")


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_u32(a[0]), _u32(b[0])) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module", params=ALL)
def case(request, tmp_path_factory):
    """The case once for all its tests: both descriptions, both device scenes, the ray sets."""
    name = request.param
    d = tmp_path_factory.mktemp(name)
    hs, hd = wc.load(d, name), wc.load(d, name, device_bvh=True)
    assert hd.counts()["nodes"] == 0
    rays, labels = wc.ray_sets(hs, name)
    if wc.is_walk_only(name):
        axis = wc.axis_rays(wc.pinwheel_size(name))[0]
        rays, labels = np.concatenate([rays, axis]), np.concatenate([labels, np.full(axis.size, AXIS, np.int8)])
    c = types.SimpleNamespace(name=name, dir=d, hs=hs, hd=hd, ds_h=rtgpu.DeviceScene(hs, 0), ds_d=rtgpu.DeviceScene(hd, 0),
                              rays=rays, labels=labels)
    yield c
    c.ds_h.close()
    c.ds_d.close()


def test_queries(case):
    name, labels = case.name, case.labels
    sc = wc.device_pool(case.hs, case.ds_h, case.rays, labels)
    rng = np.random.default_rng(20273)
    names = dict(wc.SET_NAMES)
    names[AXIS] = "axis"
    total = 0
    for c in sorted(set(labels.tolist())):
        idx = np.flatnonzero(labels == c)
        some = idx if idx.size <= MIX_CAP else np.sort(rng.choice(idx, MIX_CAP, replace=False))
        total += wc.compare_device(name, names[c], "alone", sc, idx, case.ds_h)
        total += wc.compare_device(name, names[c], "alone, device-built", sc, idx, case.ds_d)
        total += wc.mixes(name, names[c], sc, some, rng, case.ds_h)
        total += wc.mixes(name, names[c] + ", device-built", sc, some, rng, case.ds_d)
    finite = np.flatnonzero(labels != er.CLASSES["G"])
    perm = rng.permutation(finite)
    for n in (1, 63, 65, 257):
        for ds, which in ((case.ds_h, ""), (case.ds_d, ", device-built")):
            total += wc.compare_device(name, "all", "n = %d%s" % (n, which), sc, perm[:n], ds)
            total += wc.compare_device(name, "all", "n = %d from the end%s" % (n, which), sc, perm[-n:], ds)
    hit = sc["hits"]["object"][:case.rays.size] >= 0
    print(name, "rays", case.rays.size, "host hits", int(hit.sum()), "rays submitted", total)
    if name not in bc.UNHITTABLE:
        assert 0 < hit.sum() < case.rays.size
    if wc.is_walk_only(name):
        # the axis rays' closed form on the device's own answers (walk_cases.axis_rays)
        n = wc.pinwheel_size(name)
        axis, _, kind = wc.axis_rays(n)
        for ds in (case.ds_h, case.ds_d):
            for coherent in (False, True):
                occ = ds.trace(axis, any_hit=True, coherent=coherent)["object"]
                want = np.where(kind != 1, 0, -1) if name.endswith("_blocked") else np.full(axis.size, -1)
                assert np.array_equal(occ, want), (name, coherent)


def test_multihit(case):
    rays = case.rays
    for k in (1, 2, 8):
        want, want_cnt = case.hs.trace_multi(rays, k, counts=True)
        for ds, which in ((case.ds_h, "host-built"), (case.ds_d, "device-built")):
            for coherent in (False, True):
                got, cnt = ds.trace_multi(rays, k, coherent=coherent, counts=True)
                bad = np.flatnonzero((_u32(got).reshape(rays.size, -1) != _u32(want).reshape(rays.size, -1)).any(1))
                assert bad.size == 0, (case.name, which, k, coherent, bad[:8], rays[bad[:4]], got[bad[:4]], want[bad[:4]])
                assert np.array_equal(cnt, want_cnt), (case.name, which, k, coherent)
    if case.name in bc.COINCIDENT:
        n = int(case.name.split("_")[1])
        assert want_cnt.max() == min(n, 8)


def _stages(ds, flags=0):
    ds.render(0, flags=rtgpu.RTG_RENDER_TIMING | flags)
    return list(ds.timings())


def _ahb_render(hs, mode, monkeypatch, flags=0):
    monkeypatch.setenv("RTG_AHB", mode)
    ds = rtgpu.DeviceScene(hs, 0)
    monkeypatch.delenv("RTG_AHB")
    try:
        return ds.render(0, flags=flags)
    finally:
        ds.close()


def _check_oracle(name, hs, ds, base):
    """The parity criterion and the counted render against the oracle; returns the oracle's image."""
    ohdr, _, ost = ob.render(hs)
    r = ob.compare(base[0], ohdr)
    print(name, r)
    assert r["n_fail"] == 0 and r["rel_pass"] == 1.0, (name, r)
    ds.reset_stats()
    counted = ds.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS)
    st = ds.stats()
    assert _same(counted, base), (name, "counted render")
    print(name, {k: st[k] for k in st if st[k]})
    for k in COUNTERS:
        assert st[k] == ost[k], (name, k, st[k], ost[k])
    return ohdr, st


def _check_variants(name, hs, ds, base, monkeypatch):
    monkeypatch.setenv("RTG_FRAME_KERNEL", "0")
    two = ds.render(0)
    two_stages = _stages(ds)
    monkeypatch.delenv("RTG_FRAME_KERNEL")
    assert _same(two, base), (name, "RTG_FRAME_KERNEL=0")
    for flag in ("RTG_RENDER_FUSED", "RTG_RENDER_TREE", "RTG_RENDER_EXACT_SHADOW"):
        assert _same(ds.render(0, flags=getattr(rtgpu, flag)), base), (name, flag)
    for mode in ("split", "ref"):
        assert _same(_ahb_render(hs, mode, monkeypatch), base), (name, "RTG_AHB=" + mode)
    return two_stages


def test_renders(case, monkeypatch):
    name, hs, ds = case.name, case.hs, case.ds_h
    base = ds.render(0)
    assert base[0].shape == (48, 64, 3)
    stages = _stages(ds)
    two_stages = _check_variants(name, hs, ds, base, monkeypatch)
    assert _same(case.ds_d.render(0), base), (name, "device-built")
    ohdr, st = _check_oracle(name, hs, ds, base)
    big = wc.max_leaf(hs)
    print(name, "largest leaf", big, "stages", stages, "with RTG_FRAME_KERNEL=0", two_stages)
    if big > 8:                                       # FEAT_BIGLEAF: launch_wave_t's `fused` is false
        assert stages[0] == "k_primary" and stages == two_stages and "k_shade_shadow" not in stages, stages
    elif name.startswith(("copies_", "spread_", "pinwheel_")):   # plain shading, no instance, one light: fused
        assert stages == ["k_frame"] and two_stages == ["k_primary", "k_shade_shadow"], (stages, two_stages)
    if name in bc.COINCIDENT or wc.is_walk_only(name):
        assert st["shadow_rays"] > 0


@pytest.mark.parametrize("instanced", [False, True], ids=["plain", "instanced"])
@pytest.mark.parametrize("n", [8, 9, 16, 17])
def test_copies_at_the_leaf_thresholds(n, instanced, tmp_path, monkeypatch):
    """kBigLeaf = 8 and kDeferLeaf = 16 from both sides (see `pipeline` above).  The far camera
    sees the 4 x 1 triangle at a pixel of 1/2 x 1/2 (its box: 8 x 2 pixels, a dozen of them hit),
    so at most 16 lanes of a wave reach the root leaf; the deferring render equals the fused
    kernel's and the counted one bit for bit.  Plain meshes take the leaf-exact packet walk
    (walk_bvh_packet_lx); with an instance of the mesh two units up the scene takes the walk that
    is exact at every node (walk_bvh_packet), which has a deferral comparison of its own."""
    name = f"copies_{n}"
    if instanced:
        name += "_instanced"
        bc.write_scene(bc.Case([bc.copies(n)], instance=(0, (0, 2, 0))), str(tmp_path), name)
        old = os.getcwd()
        os.chdir(tmp_path)
        try:
            hs = rtgpu.HostScene(name + ".xml")
        finally:
            os.chdir(old)
    else:
        hs = wc.load(tmp_path, name)
    ds = rtgpu.DeviceScene(hs, 0)
    assert wc.max_leaf(hs) == n
    stages = _stages(ds)
    if n <= 8:
        assert stages == ["k_frame"], stages
    else:
        assert stages[0] == "k_primary" and "k_frame" not in stages, stages
    far = rtgpu.camera_setup((2.0, 0.3, 32.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 2.0, 64, 48,
                             near_plane=(-1.0, 1.0, -0.75, 0.75), base=hs.camera_record(0))
    ds.set_camera(0, far)
    monkeypatch.setenv("RTG_DEFER_DIAG", "1")
    ds.reset_stats()
    img = ds.render(0)
    pending = ds.stats()["extend_wide_visits"]
    monkeypatch.delenv("RTG_DEFER_DIAG")
    hits = ds.trace(ds.camera_rays())
    seen = int((hits["object"] >= 0).sum())
    print(name, "stages", stages, "pixels that hit", seen, "pending pixels", pending)
    assert 0 < seen <= 16 * (2 if instanced else 1)
    assert (pending > 0) == (n > 16), (name, pending)
    assert _same(ds.render(0, flags=rtgpu.RTG_RENDER_FUSED), img)
    assert _same(ds.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS), img)
    bg = np.array([10, 20, 30], np.float32)
    assert int((img[0] != bg).any(2).sum()) == seen


@pytest.fixture(scope="module")
def floor_oracle(tmp_path_factory):
    """The oracle's images of the four floor scenes, computed once: {name: (HostScene, hdr)}."""
    d = tmp_path_factory.mktemp("floors")
    out = {}
    for name in wc.WALK_ONLY:
        hs = wc.load_pinwheel_floor(d, name)
        out[name] = (hs, ob.render(hs)[0])
    return out


@pytest.mark.parametrize("name", wc.WALK_ONLY)
def test_step_bound(name, floor_oracle, monkeypatch):
    n = wc.pinwheel_size(name)
    blocked = name.endswith("_blocked")
    hs, ohdr = floor_oracle[name]
    # the premises, from the host: the wide nodes on the right side of the bound, no large leaf
    nodes = hs.anyhit_check(1)["nodes"]
    assert nodes < 4096 if n == 8192 else nodes > 4096
    assert wc.max_leaf(hs) <= 8
    ds = rtgpu.DeviceScene(hs, 0)
    base = ds.render(0)
    assert _stages(ds) == ["k_frame"]
    assert _same(ds.render(0, flags=rtgpu.RTG_RENDER_EXACT_SHADOW), base)
    r = ob.compare(base[0], ohdr)
    assert r["n_fail"] == 0 and r["rel_pass"] == 1.0, (name, r)
    ds.reset_stats()
    counted = ds.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS)
    st = ds.stats()
    assert _same(counted, base)
    print(name, "wide nodes", nodes, "shadow_rays", st["shadow_rays"], "shadow_fallbacks", st["shadow_fallbacks"],
          "shadow_wide_visits", st["shadow_wide_visits"])
    assert st["shadow_rays"] == 64 * 48 and st["shadow_wide_visits"] > 0
    if n == 8192:
        assert st["shadow_fallbacks"] == 0
    elif not blocked:
        assert st["shadow_fallbacks"] > 0
    # the patch the blocker darkens, from the oracle's two images: lit in the open variant, dark
    # in the blocked one, on the device as in the oracle
    open_o, blocked_o = floor_oracle[f"pinwheel_{n}"][1], floor_oracle[f"pinwheel_{n}_blocked"][1]
    patch = (open_o != blocked_o).any(2)
    assert patch.sum() > 1000 and (~patch).sum() > 100 and np.all(open_o[patch] > blocked_o[patch])
    assert np.array_equal(_u32(open_o[~patch]), _u32(blocked_o[~patch]))
    mine, other = (blocked_o, open_o) if blocked else (open_o, blocked_o)
    assert ob.compare(base[0][patch], mine[patch])["n_fail"] == 0
    assert np.all(base[0][patch] < other[patch]) if blocked else np.all(base[0][patch] > other[patch])
    ds.close()
