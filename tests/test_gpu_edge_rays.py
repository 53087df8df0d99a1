"""Device ray queries against the host walk on the edge rays of edge_rays.py: the rays on which the
walks' fast decisions are not sure -- zero and signed-zero direction components, origins in box
planes, rays at vertices and along edges, origins on the geometry, tmax at / next to / beyond a
hit, direction components at the ends of the fast range -- put through every walk the renders
use, bit for bit.

  edge_lattice, synth_10k    FEAT 0: the packet walk, the any-hit wide walk
  simple, spheres            FEAT_SPHERE
  transforms_textures        instances
  edge_roof                  an instance over boxes that are thick on every axis: class B in the
                             instance's frame reaches the fused slab test with a local origin
                             coordinate of exactly 0 on a -0 axis (o * rcp(d) = NaN, not inf)
  dof_motion                 motion blur
  mesh_light                 RTG_OBJF_SHADOW_SKIP
  defer_gate (generated)     FEAT_BIGLEAF: the cooperative large leaves, the reference any-hit
                             walk per lane

Each scene's rays come from its golden (tests/golden/edge_rays_<scene>.npz: test_edge_rays_host.py
holds the host walk to the reference's own answers on exactly these rays, so device == reference
follows); `defer_gate` and `synth_10k` generate theirs with the same generator.

The exact fallbacks are voted per wave, so every class is submitted alone, interleaved with the
scene's camera rays at one edge lane per 64 (lane 0 in even waves -- the packet walk takes its
order from the first live lane --, lane 63 in odd ones), and at 32 edge lanes per 64; and as
partial waves and blocks of n = 1, 63, 65, 257 rays.

What the file catches, tried on libraries with one mutated decision in the query kernels each
(through RTGPU_LIB):

  * the fast triangle tests' strict `t < minT` turned into `<=`: both tests below fail on seven
    of the nine scenes;
  * `ray_rcp` reporting `fast` for every ray: test_device_equals_host_on_edge_rays[edge_roof]
    fails (class B, coherent).  Elsewhere a zero direction component makes a slab distance or
    o * rcp(d) infinite, and the infinite slack keeps the lane unsure whatever `fast` says; only
    a local origin coordinate of exactly 0 on that axis gives 0 * inf = NaN instead, which min /
    max drop, so that `fast` is the one term left between the lane and a decision that ignores
    the axis.  edge_roof's class B rays in the instance's frame are made for that, on boxes
    thick enough on the other axes to be sure (edge_lattice's flat boxes never are);
  * the NaN-propagating minimum in box_pass_t's `sure` replaced by an fminf chain: nothing
    fails, here or in test_gpu_query.py.  The reading behind that, not a proof: with a ray off
    the fast range the slack is infinite and every term of the minimum is -inf or NaN, so the
    chain's result is -inf or NaN as well; on the fast range a term can be NaN only through an
    infinite slab distance -- which takes an overflowing o * rcp(d), and then the slack is
    infinite again (class F), or an infinite box face, which no fixture has -- or through
    minT = NaN (tmax = NaN, class E), where the mutant
    lets boxes through that the exact test drops -- but every face test under them compares
    t < NaN and rejects, so the answer is the same miss.  A scene with infinite box faces would
    be needed to tell this mutant from the library by its answers.
"""
import os

import numpy as np
import pytest

import edge_rays as er
import oracle_bind as ob
import query_util as qu
import rtgpu
import walk_cases as wc

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = ["edge_lattice", "edge_roof", "synth_10k", "simple", "spheres", "transforms_textures", "dof_motion",
         "mesh_light", "defer_gate"]
GENERATED = ("synth_10k", "defer_gate")
VARIANTS = wc.VARIANTS               # (label, any_hit, coherent, normals)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)
    _cache.clear()


def _scene(name, tmp_path_factory):
    """The scene once per module: HostScene, DeviceScene, the class labels, and a pool of rays --
    the edge rays followed by the scene's camera rays -- with the host walk's answers on it
    (rays are independent, so any submission's expected bytes are a gather from the pool)."""
    if name in _cache:
        return _cache[name]
    if name == "defer_gate":
        import scenes
        d = tmp_path_factory.mktemp("defer_gate")
        xml = scenes.config_defer_gate(str(d))
        old = os.getcwd()
        os.chdir(d)
        try:
            hs = rtgpu.HostScene(xml)
            ds = rtgpu.DeviceScene(hs, 0)
        finally:
            os.chdir(old)
    else:
        hs = rtgpu.HostScene(name + ".xml")
        ds = rtgpu.DeviceScene(hs, 0)
    if name in GENERATED:
        rays, labels = er.generate(hs)
    else:
        z = np.load(os.path.join(ob.GOLDEN, f"edge_rays_{name}.npz"), allow_pickle=False)
        rays, labels = z["rays"].view(rtgpu.RAY_DTYPE).reshape(-1), z["labels"]
    sc = wc.device_pool(hs, ds, rays, labels)
    _cache[name] = sc
    return sc


# the comparison and the wave mixes are shared with test_gpu_walk_cases.py (walk_cases.py)
_compare = wc.compare_device
_mixes = wc.mixes


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_on_edge_rays(name, tmp_path_factory):
    """Classes A-F, each alone and in the two wave mixes, and n = 1, 63, 65, 257 with an edge ray
    as the first lane: every closest-hit variant equals hs.trace as raw bytes (t, object, face, the
    pad word, the normals' bits), every occlusion variant its boolean."""
    sc = _scene(name, tmp_path_factory)
    labels = sc["labels"]
    rng = np.random.default_rng(20262)
    total = 0
    for cls in "ABCDEF":
        edge = np.flatnonzero(labels == er.CLASSES[cls])
        assert edge.size > 0, (name, cls)
        total += _mixes(name, cls, sc, edge, rng)
    finite = np.flatnonzero(labels != er.CLASSES["G"])
    perm = rng.permutation(finite)
    for n in (1, 63, 65, 257):
        total += _compare(name, "A-F", "n = %d" % n, sc, perm[:n])
        total += _compare(name, "A-F", "n = %d from the end" % n, sc, perm[-n:])
    hit = sc["hits"]["object"][finite] >= 0
    print(name, "edge rays", finite.size, "host hits", int(hit.sum()), "rays submitted", total)
    assert 0 < hit.sum() < finite.size


@pytest.mark.parametrize("name", NAMES)
def test_tmax_tie_on_device(name, tmp_path_factory):
    """Class E on device results alone: a ray whose tmax = nextafter(t, +inf) hits at exactly t
    must miss with tmax = t (IntersectFace's t < minT is strict), on the per-lane walk, the packet
    walk and both occlusion walks; tmax = 0, -0, -1 and NaN miss with tmax's own bits."""
    sc = _scene(name, tmp_path_factory)
    ds = sc["ds"]
    e = sc["pool"][:sc["n_edge"]][sc["labels"] == er.CLASSES["E"]].reshape(-1, 10)
    at, up = e[:, 0], e[:, 1]
    assert np.array_equal(up["tmax"], np.nextafter(at["tmax"], np.float32(np.inf)))
    assert np.array_equal(qu.origins(at), qu.origins(up)) and np.array_equal(qu.directions(at), qu.directions(up))
    flat = e.reshape(-1)
    seen = 0
    for coherent in (False, True):
        hits = ds.trace(flat, coherent=coherent).reshape(-1, 10)
        occ = ds.trace(flat, any_hit=True, coherent=coherent)["object"].reshape(-1, 10)
        ties = (hits["object"][:, 1] >= 0) & (hits["t"][:, 1].view(np.uint32) == at["tmax"].view(np.uint32))
        seen += int(ties.sum())
        bad = np.flatnonzero(ties & ((hits["object"][:, 0] != -1) | (hits["face"][:, 0] != -1)
                                     | (hits["t"][:, 0].view(np.uint32) != at["tmax"].view(np.uint32))))
        assert bad.size == 0, (name, coherent, "tmax = t still hits", e[bad[:4], 0], hits[bad[:4], :2])
        for col in (3, 4, 5, 9):                                 # tmax = 0, -0, -1, NaN
            miss = (hits["object"][:, col] == -1) & (hits["t"][:, col].view(np.uint32) == e["tmax"][:, col].view(np.uint32))
            assert miss.all() and np.all(occ[:, col] == -1), (name, coherent, "tmax column", col)
        # occlusion: occluded below next_up(t) implies something strictly below it; with tmax = t
        # the face at t no longer counts, so the answer can only go from occluded to clear
        assert np.all(occ[:, 0] <= occ[:, 1]), (name, coherent)
    print(name, "class E groups", e.shape[0], "ties seen", seen)
    assert seen > 0


@pytest.mark.parametrize("name", NAMES)
def test_nonfinite_rays(name, tmp_path_factory):
    """Class G -- a NaN or an infinity in one origin or direction component -- in a test of its
    own, alone and in the two wave mixes: the device answers what the host walk (and, through the
    goldens, the reference) answers, and returns.

    Why every loop these rays reach ends for ANY float input -- each is bounded by integers that
    come from the scene's records, never from the ray:

      walk_bvh_seq (the per-lane walk; walk_bvh on scenes without large leaves): the node index
        goes to i + 1 or to the record's skip link, both greater than i (skip = the end of the
        node's pre-order subtree, rtg_api.cpp reference_preorder), until it reaches `end`; the
        float results only choose between the two.  A leaf's face loop runs `cnt` times.
      walk_bvh, cooperative large leaves: the wave loops while some lane is active; an active
        lane's node index grows every step as above and the lane retires at `end`.
        coop_leaf_tests loops over at most 64 events, over the sum of their leaf counts, and a
        binary search over the events.
      walk_bvh_packet: one wave-uniform node index that goes to i + 1 or to the record's skip,
        each above i, until `end`; leaves as above.
      walk_wide_any_pk: an explicit step counter (RTG_PK_MAX_STEPS) and a stack of
        RTG_PK_STACK entries that only pops between descents; a ray whose direction is off the
        fast range, or whose o * rcp(d) is not finite, never walks (it is undecided at once and
        takes the reference walk, trace<true>, i.e. walk_bvh above).
      the reference any-hit walk per lane (trace<true>) is walk_bvh with an early exit.
      trace / trace_any_wide: the object index only grows (a group skip jumps to group_end > k).

    No index, address or loop bound is computed from a ray's floats, so a NaN can change which
    boxes pass but not how far a walk runs.  (walk_closest_pk, the ordered render's walk, is not
    reached by the queries.)"""
    sc = _scene(name, tmp_path_factory)
    edge = np.flatnonzero(sc["labels"] == er.CLASSES["G"])
    assert edge.size >= 54
    o, d = qu.origins(sc["pool"][edge]), qu.directions(sc["pool"][edge])
    assert np.all((~np.isfinite(o)).sum(1) + (~np.isfinite(d)).sum(1) == 1)
    total = _mixes(name, "G", sc, edge, np.random.default_rng(20263))
    print(name, "non-finite rays", edge.size, "rays submitted", total)
