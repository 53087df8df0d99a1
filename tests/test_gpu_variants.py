"""Every kernel instantiation csrc/rtg_variants.hpp can choose, run on the device: one case per row of
the zoo's table (tests/variant_scenes.py CELLS; test_variant_zoo_host.py proves on the host that each
row's scene, flags and environment take the row's instantiation).

Per cell, as the instantiation allows:
  oracle parity      the cell's own launch against oracle_bind on the same seed, |d| <= 1e-4 * max(1, |ref|):
                     every pixel (ray) of a deterministic cell, and equal ray and traversal counters where
                     the render is counted; path-tracing cells allow FLIP_CAP of the pixels (rays) outside
                     (device sinf / acosf / atan2f flips) and the stochastic counter rule of test_gpu_parity.py
  special == general RTG_MEGA_GENERAL=1 against unset, uint32 views and LDR bytes (all 16 special cells,
                     k_render and k_radiance)
  counted == uncounted   the two builds of a general instantiation
  tree == fused      RTG_RENDER_TREE against RTG_RENDER_FUSED, bits and counters (ray tracing, depth > 0)
  wavefront == fused the wavefront path tracer against the fused kernel, twice in a row (the step cells)
  device == host     ray queries of every kind against HostScene on the camera rays plus
                     radiance_rays.generate (the traversal sets)
and, beside the table: stack-depth invariance (MAXD 8 against MAXD 32 on identical work) and scene
updates across the 8 / 9 switch.

Each case prints its worst deviation from the oracle (DESIGN.md §5 records them).
"""
import numpy as np
import pytest

import oracle_bind as ob
import radiance_rays as rr
import rtgpu
import variant_scenes as zoo

pytestmark = pytest.mark.gpu

REL = 1e-4
FLIP_CAP = 0.005
SEED = 1234
FUSED, TREE, COUNT, TIMING = zoo.FUSED, zoo.TREE, zoo.COUNT, rtgpu.RTG_RENDER_TIMING
COUNTERS = ("camera_rays", "secondary_rays", "shadow_rays", "node_visits", "tri_tests")
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_scenes():
    yield
    _cache.clear()


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("RTG_MEGA_GENERAL", raising=False)


def _scene(sw, tmp_path_factory):
    """(hs, ds, {}) of a room, once per module run; the dict keeps the oracle's answers."""
    key = zoo.key(sw)
    if key not in _cache:
        hs = rtgpu.HostScene(zoo.room(str(tmp_path_factory.mktemp("zoo")), **sw))
        _cache[key] = (hs, rtgpu.DeviceScene(hs, 0), {})
    return _cache[key]


def _oracle(scene):
    hs, _, memo = scene
    if "render" not in memo:
        hdr, _, st = ob.render(hs, seed=SEED)
        hdr.setflags(write=False)
        memo["render"] = (hdr, st)
    return memo["render"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _outside(got, ref):
    """Pixels (rays) with a channel outside the parity bound; equal bits and a NaN on both sides pass."""
    g, w = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(g - w) <= REL * np.maximum(1.0, np.abs(w))) | rr.same_bits(got, ref)
    return ~ok.all(-1)


def _worst(got, ref):
    g, w = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(g - w) / np.maximum(1.0, np.abs(w)), initial=0.0))


def _parity(cell, what, got, ref, stochastic):
    bad = _outside(got, ref)
    print("ZOO %-34s %-10s worst |d| / max(1, |ref|) %.3g outside %d of %d bit-equal %.4f" % (
        cell.id, what, _worst(got, ref), int(bad.sum()), bad.size, float(rr.same_bits(got, ref).mean())))
    if stochastic:
        assert bad.sum() <= FLIP_CAP * bad.size, (cell.id, what, int(bad.sum()), bad.size)
    else:
        assert not bad.any(), (cell.id, what, int(bad.sum()), np.flatnonzero(bad)[:8])


def _counters(cell, st, ost, stochastic, keys=COUNTERS):
    for k in keys:
        if stochastic:      # a last-ulp difference can move one sampled ray; allow a sliver
            assert abs(st[k] - ost[k]) <= max(4, 0.002 * ost[k]), (cell.id, k, st[k], ost[k])
        else:
            assert st[k] == ost[k], (cell.id, k, st[k], ost[k])


def _render(ds, flags):
    ds.reset_stats()
    hdr, ldr = ds.render(0, flags=flags, seed=SEED)
    return hdr, ldr, ds.stats()


def _same_image(a, b, what):
    assert np.array_equal(_bits(a[0]), _bits(b[0])), (what, ob.compare(a[0], b[0]))
    assert np.array_equal(a[1], b[1]), what


def _ran(ds, flags, name):
    """The pipeline the flags take, by the kernels RTG_RENDER_TIMING names."""
    ds.render(0, flags=flags | TIMING, seed=SEED)
    t = ds.timings()
    if name == "fused":
        assert list(t) == ["k_render"], t
    elif name == "wave":
        assert "k_primary" in t or "k_frame" in t, t
    else:
        assert {"tree": "tree_levels", "path": "path_iterations"}[name] in t, t


def _tree_equals_fused(cell, ds):
    """test_tree_pipeline_equals_fused_kernel's checks."""
    a, b = _render(ds, TREE | COUNT), _render(ds, FUSED | COUNT)
    _same_image(a, b, (cell.id, "tree == fused, counted"))
    for k in COUNTERS + ("sphere_tests",):
        assert a[2][k] == b[2][k], (cell.id, k, a[2][k], b[2][k])
    _same_image(_render(ds, TREE), a, (cell.id, "tree uncounted"))
    _same_image(_render(ds, FUSED), a, (cell.id, "fused uncounted"))
    _ran(ds, TREE, "tree")
    return a


def _query_rays(scene, ds):
    hs, _, memo = scene
    if "rays" not in memo:
        cam = ds.camera_rays(seed=SEED)
        off, ids, _ = rr.generate(hs)
        memo["rays"] = (np.concatenate([cam, off]), np.concatenate([np.arange(cam.size, dtype=np.int32), ids]))
    return memo["rays"]


@pytest.mark.parametrize("cell", zoo.CELLS, ids=[c.id for c in zoo.CELLS])
def test_cell(cell, tmp_path_factory, monkeypatch):
    scene = _scene(cell.switches, tmp_path_factory)
    hs, ds, _ = scene
    s = zoo.resolve(**cell.switches)
    pt = s["renderer"] != "rt"

    def switch(on):
        if on:
            monkeypatch.setenv("RTG_MEGA_GENERAL", "1")
        else:
            monkeypatch.delenv("RTG_MEGA_GENERAL", raising=False)

    if cell.kernel == "k_render":
        ohdr, ost = _oracle(scene)
        switch(bool(cell.env))
        own = _render(ds, cell.flags)
        _ran(ds, cell.flags, "fused")
        switch(False)
        _parity(cell, "render", own[0], ohdr, pt)
        assert np.array_equal(own[1], ob.clamp_ldr(own[0]))
        if cell.flags & COUNT:
            _counters(cell, own[2], ost, pt, COUNTERS if not pt else COUNTERS[:3])
        if zoo.is_special(cell):
            switch(True)
            general = _render(ds, cell.flags)
            switch(False)
            _same_image(general, own, (cell.id, "special == general"))
        if cell.flags & COUNT or cell.env:
            # the general instantiation's other build, and what the scene takes uncounted by itself
            switch(True)
            other = _render(ds, (cell.flags ^ COUNT) if cell.env else (cell.flags & ~COUNT))
            switch(False)
            _same_image(other, own, (cell.id, "counted == uncounted"))
            _same_image(_render(ds, cell.flags & ~COUNT), own, (cell.id, "the scene's own uncounted instantiation"))
        if not pt and s["depth"] > 0:
            _same_image(_tree_equals_fused(cell, ds), own, (cell.id, "tree == the cell's render"))
    elif cell.kernel == "k_radiance":
        rays, ids = _query_rays(scene, ds)
        switch(bool(cell.env))
        got = ds.radiance(rays, pixel_ids=ids, seed=SEED)
        switch(False)
        want, _ = ob.radiance(hs, rays, ids, seed=SEED)
        _parity(cell, "radiance", got[:, :3], want[:, :3], pt)
        host_t = hs.trace(rays)["t"]
        assert np.array_equal(_bits(got[:, 3]), _bits(host_t)) and np.array_equal(_bits(want[:, 3]), _bits(host_t))
        if zoo.is_special(cell):
            switch(True)
            general = ds.radiance(rays, pixel_ids=ids, seed=SEED)
            switch(False)
            assert rr.same_bits(general, got).all(), (cell.id, "special == general")
        if cell.env:
            assert rr.same_bits(ds.radiance(rays, pixel_ids=ids, seed=SEED), got).all(), (cell.id, "general == special")
    elif cell.kernel == "k_path_step":
        ohdr, ost = _oracle(scene)
        fused = _render(ds, FUSED | (cell.flags & COUNT))
        for _ in range(2):          # the first render plans its later passes; the second runs planned
            own = _render(ds, cell.flags)
            _same_image(own, fused, (cell.id, "wavefront == fused"))
        _ran(ds, cell.flags, "path")
        _parity(cell, "path", own[0], ohdr, True)
        if cell.flags & COUNT:
            for k in COUNTERS[:3]:
                assert own[2][k] == fused[2][k], (cell.id, k, own[2][k], fused[2][k])
            _counters(cell, own[2], ost, True, COUNTERS[:3])
    elif cell.kernel == "k_tree_shade":
        ohdr, ost = _oracle(scene)
        own = _tree_equals_fused(cell, ds)
        _parity(cell, "tree", own[0], ohdr, False)
        _counters(cell, own[2], ost, False)
    else:
        pipe = cell.inst[0]
        if pipe in ("wave", "tree", "path"):
            ohdr, ost = _oracle(scene)
            if pipe == "tree":
                own = _tree_equals_fused(cell, ds)
                _counters(cell, own[2], ost, False)
            else:
                own = _render(ds, cell.flags)
                _ran(ds, cell.flags, pipe)
                _same_image(own, _render(ds, FUSED), (cell.id, pipe + " == fused"))
                if pipe == "path":
                    _same_image(_render(ds, cell.flags), own, (cell.id, "planned == first"))
            _parity(cell, pipe, own[0], ohdr, pt)
            return
        rays, _ = _query_rays(scene, ds)
        want = hs.trace(rays)
        if pipe == "query":
            for coherent in (False, True):
                got = ds.trace(rays, coherent=coherent)
                assert got.tobytes() == want.tobytes(), (cell.id, coherent)
        elif pipe == "anyhit":
            occ = hs.trace(rays, any_hit=True)["object"]
            assert (occ >= 0).any() and (occ < 0).any()
            for coherent in (False, True):
                assert np.array_equal(ds.trace(rays, any_hit=True, coherent=coherent)["object"], occ), (cell.id, coherent)
        elif pipe == "multihit":
            hits, counts = ds.trace_multi(rays, 3, counts=True)
            h_hits, h_counts = hs.trace_multi(rays, 3, counts=True)
            assert np.array_equal(counts, h_counts) and hits.tobytes() == h_hits.tobytes(), cell.id
            assert (counts > 1).any() and (counts == 0).any()
        else:
            surf = ds.surface(rays)
            for k in ("t", "object", "face"):
                assert surf[k].tobytes() == want[k].tobytes(), (cell.id, k)
            miss = surf[want["object"] < 0]
            assert miss.size and (miss["material"] == -1).all()
            rest = [n for n in rtgpu.SURFACE_DTYPE.names if n not in ("t", "object", "face", "material")]
            assert all(not np.ascontiguousarray(miss[n]).view(np.uint8).any() for n in rest), cell.id
            hit = surf[want["object"] >= 0]
            assert (hit["material"] >= 0).all()


# scenes whose oracle images at depths 8 and 9 may be equal: the shallow room (they are:
# test_variant_zoo_host.py), and the open metal room
INVARIANT = {"shallow": zoo.SHALLOW, "shallow_bigleaf": dict(zoo.SHALLOW, bigleaf=True, xlight=True), "metal": zoo.OPEN_METAL}


@pytest.mark.parametrize("name", list(INVARIANT))
def test_stack_depth_invariance(name, tmp_path_factory):
    """Where the oracle's images of one scene at depths 8 and 9 are bit-equal, the device's are too, in
    the fused kernel (MAXD 8 against MAXD 32: identical work on two frame stacks), the ray-tree
    pipeline and the radiance queries.  Where they differ nothing is asserted beyond test_cell's parity."""
    scenes = [_scene(dict(INVARIANT[name], depth=d), tmp_path_factory) for d in (8, 9)]
    o8, o9 = (_oracle(sc)[0] for sc in scenes)
    if name.startswith("shallow"):
        assert np.array_equal(_bits(o8), _bits(o9))
    if not np.array_equal(_bits(o8), _bits(o9)):
        print(name, "the oracle's images differ: nothing to assert")
        return
    for flags in (FUSED, TREE, FUSED | COUNT):
        a, b = (_render(sc[1], flags) for sc in scenes)
        _same_image(a, b, (name, flags))
        assert not _outside(a[0], o8).any()
    rays, ids = _query_rays(scenes[0], scenes[0][1])
    r8, r9 = (sc[1].radiance(rays, pixel_ids=ids, seed=SEED) for sc in scenes)
    w8, w9 = (ob.radiance(sc[0], rays, ids, seed=SEED)[0] for sc in scenes)
    if rr.same_bits(w8, w9).all():
        assert rr.same_bits(r8, r9).all()


def test_update_across_the_stack_switch(tmp_path_factory):
    """test_gpu_update.py's contract over a change of instantiation: a scene created at depth 6 (MAXD
    8) and updated to depth 12 (MAXD 32), then back, renders and answers radiance queries bit for bit
    as a scene freshly created from that description."""
    d = tmp_path_factory.mktemp("zoo_update")
    hs = {depth: rtgpu.HostScene(zoo.room(str(d), **dict(zoo.UPDATE, depth=depth))) for depth in (6, 12)}
    fresh = {depth: rtgpu.DeviceScene(h, 0) for depth, h in hs.items()}
    ds = rtgpu.DeviceScene(hs[6], 0)
    rays = np.concatenate([ds.camera_rays(seed=SEED), rr.generate(hs[6])[0]])
    images = {}
    for depth in (12, 6, 12):
        ds.update(hs[depth])
        for flags in (0, FUSED, TREE, FUSED | COUNT):
            a, b = _render(ds, flags), _render(fresh[depth], flags)
            _same_image(a, b, (depth, flags))
            if flags & COUNT:
                assert a[2] == b[2], (depth, a[2], b[2])
        assert rr.same_bits(ds.radiance(rays, seed=SEED), fresh[depth].radiance(rays, seed=SEED)).all(), depth
        images[depth] = a[0]
        ohdr, _, _ = ob.render(hs[depth], seed=SEED)
        assert not _outside(a[0], ohdr).any(), depth
    # the update is seen: levels 7 .. 12 show in the image
    assert not np.array_equal(_bits(images[6]), _bits(images[12]))
