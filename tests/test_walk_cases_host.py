"""The host walks (HostScene.trace, trace_multi: the yardsticks of the device queries) on the
adversarial meshes of bvh_cases.py and the walk-only cases of walk_cases.py, held to three
yardsticks that do not pass through them:

  * the reference's own answers (tests/golden/walk_rays_<case>.npz, make_goldens.py `walk_rays`:
    refdriver rays, run twice) on the edge, aimed and light rays of the recorded cases, compared
    as test_edge_rays_host.py compares (walk_cases.check_host_equals_reference): hit flag, the
    bits of t, the object, the occlusion boolean, no ray left out.  Sets dropped because two runs
    of the reference differed: none (walk_rays_manifest.json lists them);
  * a float64 brute force on the aimed rays of every case outside bvh_cases.UNHITTABLE
    (walk_cases.check_brute_force).  Grazing shares, as asserted (<= 1 %) and printed: no ray at
    all on every case but lattice / lattice_uv (3 of 84 336 rays: 0.00004) and several (9 of
    96 744: 0.00009); the largest error of t is 8.9e-6 relative (several);
  * closed forms: coincident copies through trace_multi, the pinwheels' axis rays.

And trace_multi with k = 1 equals trace byte for byte on every ray set of every case.
"""
import json
import os

import numpy as np
import pytest

import bvh_cases as bc
import edge_rays as er
import multihit_scenes as ms
import oracle_bind as ob
import query_util as qu
import rtgpu
import walk_cases as wc

ALL = bc.NAMES + list(wc.WALK_ONLY)
with open(os.path.join(ob.GOLDEN, "walk_rays_manifest.json")) as _f:
    MANIFEST = json.load(_f)

_cache = {}


def _scene(name, tmp_path_factory):
    """(HostScene, {set: rays}) -- loaded and generated once per module."""
    if name not in _cache:
        hs = wc.load(tmp_path_factory.mktemp(name), name)
        rays, labels = wc.ray_sets(hs, name)
        sets = {"all": rays}
        if wc.is_walk_only(name):
            sets["axis"] = wc.axis_rays(wc.pinwheel_size(name))[0]
        for a in list(sets.values()) + [labels]:
            a.setflags(write=False)
        _cache[name] = (hs, sets, labels)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def load_golden(name):
    z = np.load(os.path.join(ob.GOLDEN, f"walk_rays_{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["rays"] = g["rays"].view(rtgpu.RAY_DTYPE).reshape(-1)
    return g


def test_every_recorded_case_is_recorded_or_named():
    assert set(MANIFEST["cases"]) | set(MANIFEST["dropped"]) == set(wc.RECORDED)
    assert not set(MANIFEST["cases"]) & set(MANIFEST["dropped"])
    assert not set(wc.RECORDED) - set(bc.NAMES) and not set(wc.WALK_ONLY) & set(bc.NAMES)
    for name in MANIFEST["cases"]:
        assert os.path.getsize(os.path.join(ob.GOLDEN, f"walk_rays_{name}.npz")) <= 256 * 1024


@pytest.mark.parametrize("name", wc.RECORDED)
def test_host_equals_reference(name, tmp_path_factory):
    assert name in MANIFEST["cases"], MANIFEST["dropped"].get(name)
    g = load_golden(name)
    hs, sets, labels_all = _scene(name, tmp_path_factory)
    assert str(g["sha256"]) == wc.get(name).vertex_sha256() == MANIFEST["cases"][name]["sha256"], \
        "the case's generator drifted: record the goldens again (make_goldens.py walk_rays)"
    rays, labels = g["rays"], g["labels"]
    assert rays.tobytes() == sets["all"][g["index"]].tobytes() and np.array_equal(labels, labels_all[g["index"]]), \
        "the ray generators drifted: record the goldens again (make_goldens.py walk_rays)"
    present = set(np.unique(labels).tolist())
    dropped = MANIFEST["cases"][name]["dropped_sets"]
    assert present | {wc.SETS[d.split(" ")[0]] for d in dropped} >= set(np.unique(labels_all).tolist())
    hits = hs.trace(rays)
    occ = hs.trace(rays, any_hit=True)["object"]
    ref_hit = g["has_hit"] != 0
    # the reference's own bookkeeping: a miss keeps tmax, a hit names a shape of the lists
    assert np.array_equal(g["t_bits"][~ref_hit], rays["tmax"].view(np.uint32)[~ref_hit])
    assert np.all(g["position"][ref_hit] >= 0) and np.all(g["position"][~ref_hit] == -1)
    print(f"{name}: set  rays  hits  occluded")
    for c in sorted(present):
        s = labels == c
        print(f"{name}:   {wc.SET_NAMES[c]:12s} {int(s.sum()):6d} {int(ref_hit[s].sum()):6d} "
              f"{int((g['occluded'][s] != 0).sum()):6d}")
    if name not in bc.UNHITTABLE:
        assert ref_hit[labels == wc.SETS["aimed"]].any() and not ref_hit[labels == wc.SETS["aimed_short"]].any()
    wc.check_host_equals_reference(name, rays, labels, g, hits, occ, wc.SET_NAMES)


def test_blocked_brute_force_equals_the_plain_ones(tmp_path_factory):
    """walk_cases.brute_force_nearest_two is query_util.brute_force done in blocks of faces: the
    same t, object and grazing flags, and the first two entries of multihit_scenes.brute_force_all."""
    for name in ("tie_split", "empty_half"):
        hs, sets, labels = _scene(name, tmp_path_factory)
        rays = sets["all"][labels == wc.SETS["aimed"]][:512]
        _, objs, meshes, faces = qu.scene_arrays(hs)
        o, d = qu.origins(rays), qu.directions(rays)
        t, k, grazing = qu.brute_force(objs, meshes, faces, o, d)
        every, grazing_all = ms.brute_force_all(objs, meshes, faces, o, d)
        t1, k1, f1, t2, gr = wc.brute_force_nearest_two(objs, meshes, faces, o, d, chunk=7)
        assert np.array_equal(t, t1) and np.array_equal(k, k1) and np.array_equal(grazing, gr)
        assert np.array_equal(grazing_all, gr) and (k >= 0).sum() > 256
        for i, row in enumerate(every):
            assert (row[0][0] if row else np.inf) == t1[i] and (row[1][0] if len(row) > 1 else np.inf) == t2[i]
            if row:
                F = faces[f1[i]]
                assert meshes[objs[k1[i]]["mesh"]]["face_offset"] <= f1[i] and np.isfinite(F["v0"]).all()


@pytest.mark.parametrize("name", [n for n in ALL if n not in bc.UNHITTABLE])
def test_host_passes_brute_force(name, tmp_path_factory):
    hs, sets, labels = _scene(name, tmp_path_factory)
    rays = sets["all"][labels >= wc.SETS["aimed"]]
    rays = rays[labels[labels >= wc.SETS["aimed"]] != wc.SETS["light"]]
    assert rays.size >= 3 * wc.AIMED_MIN
    fig = wc.check_brute_force(name, hs, rays, hs.trace(rays))
    print(name, fig)
    assert fig["hits"] > 0
    if name not in bc.COINCIDENT:
        assert fig["unique_faces"] > 0


@pytest.mark.parametrize("name", bc.COINCIDENT)
def test_coincident_copies_closed_form(name, tmp_path_factory):
    """copies_<n>: every ray that hits meets all n copies at one t.  trace_multi(k) fills
    min(n, k) slots with the faces 0 .. min(n, k) - 1 in that order, every slot the same t bits."""
    n = int(name.split("_")[1])
    hs, sets, labels = _scene(name, tmp_path_factory)
    W, owner = er.world_faces(hs)
    o, d = bc.face_rays(W, owner)
    rays = np.concatenate([rtgpu.make_rays(o, d), sets["all"][labels == wc.SETS["aimed"]]])
    closest = hs.trace(rays)
    assert np.all(closest["object"] == 0) and np.all(closest["face"] == 0)
    for k in (1, 2, 8):
        hits, counts = hs.trace_multi(rays, k, counts=True)
        m = min(n, k)
        assert np.all(counts == m), (name, k, np.unique(counts))
        assert np.all(hits["object"][:, :m] == 0)
        assert np.array_equal(hits["face"][:, :m], np.broadcast_to(np.arange(m), (rays.size, m))), (name, k)
        assert np.all(hits["t"][:, :m].view(np.uint32) == closest["t"].view(np.uint32)[:, None]), (name, k)


@pytest.mark.parametrize("name", wc.WALK_ONLY)
def test_pinwheel_premises_and_axis_rays(name, tmp_path_factory):
    """What the step-bound tests rely on, from the host: the default any-hit tree's wide nodes on
    one side and the other of RTG_PK_MAX_STEPS = 4096, no leaf above kBigLeaf = 8 (so no
    FEAT_BIGLEAF), and the axis rays' closed form: nothing on the open variants; the blocker,
    exactly when tmax is past it, on the blocked ones."""
    n = wc.pinwheel_size(name)
    hs, sets, _ = _scene(name, tmp_path_factory)
    nodes = hs.anyhit_check(1)["nodes"]
    print(name, "wide nodes", nodes, "largest leaf", wc.max_leaf(hs))
    assert nodes < 4096 if n == 8192 else nodes > 4096
    assert wc.max_leaf(hs) <= 8
    rays, up, kind = wc.axis_rays(n)
    assert rays.size == 3 * 256 and up.sum() == (~up).sum()
    hits = hs.trace(rays)
    occ = hs.trace(rays, any_hit=True)["object"]
    if not name.endswith("_blocked"):
        assert np.all(hits["object"] == -1) and np.all(occ == -1)
        return
    face = wc.blocker_face(hs, n)
    past = kind != 1
    assert np.all(hits["object"][past] == 0) and np.all(hits["face"][past] == face) and np.all(occ[past] == 0)
    assert np.all(hits["object"][~past] == -1) and np.all(occ[~past] == -1)
    t = np.abs(wc.pinwheel_blocker_z(n) - qu.origins(rays)[:, 2].astype(np.float64))
    assert np.all(np.abs(hits["t"][past] - t[past]) <= 1e-4 * t[past])


@pytest.mark.parametrize("name", ALL)
def test_k1_equals_closest_hit(name, tmp_path_factory):
    hs, sets, _ = _scene(name, tmp_path_factory)
    for label, rays in sets.items():
        want = hs.trace(rays)
        got = hs.trace_multi(rays, 1)
        assert got.shape == (rays.size, 1)
        assert got.tobytes() == want.tobytes(), (name, label)
