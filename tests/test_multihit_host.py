"""Multi-hit ray queries on the host (rtg_desc_trace_rays_multi, HostScene.trace_multi): the k
nearest hits along a ray, the yardstick of the device query (test_gpu_multihit.py).  Checked
against the closest-hit walk (k = 1, byte for byte -- which carries its pin to the reference over
to the new walk: the committed edge-ray fixtures included), an analytic layered scene
(multihit_scenes.py), a float64 brute force returning every hit, and its own structure.

Brute force, figures of the seeds used here (4 096 rays, k = 8; the cap on excluded rays is 1 %):
printed by the test; a near tie is counted among a ray's first k + 1 float64 hits -- the only ones
that can reach or leave the k slots.  No ray of `two_spheres`' view cone meets both spheres, so a
ray holds two roots or none there: the "a quarter of the rays hold >= 3 hits, some hold all 8"
condition is asserted on the layered scene (all rays hold >= 3, 2 862 hold 8), and on
`two_spheres` that rays with two roots and with none both occur."""
import ctypes
import os

import numpy as np
import pytest

import multihit_scenes as ms
import oracle_bind as ob
import query_util as qu
import rtgpu
from test_edge_rays_host import NAMES as EDGE_NAMES
from test_edge_rays_host import load_golden
from test_query_host import _cone_rays

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = ["simple", "spheres", "two_spheres", "synth_10k", "transforms_textures", "dof_motion", "mesh_light", "layered"]
KS = (1, 2, 3, 4, 5, 8)


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


_cache = {}


def _scene(name, tmp_path_factory):
    """(HostScene, ray sets) -- loaded once; the ray sets: pixel-centre camera rays and 4 096
    seeded random rays with finite tmax and random time."""
    if name not in _cache:
        hs = ms.load_layered(tmp_path_factory.mktemp("layered")) if name == "layered" else rtgpu.HostScene(name + ".xml")
        cam = qu.numpy_camera_rays(qu.camera_record(hs))
        hits = hs.trace(cam)
        hit = hits["object"] >= 0
        p = qu.origins(cam)[hit] + qu.directions(cam)[hit] * hits["t"][hit][:, None]
        lo = np.minimum(p.min(0), qu.origins(cam).min(0))
        hi = np.maximum(p.max(0), qu.origins(cam).max(0))
        rng = np.random.default_rng(20252)
        n = 4096
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        diag = float(np.linalg.norm(hi - lo))
        rnd = rtgpu.make_rays(rng.uniform(lo, hi, (n, 3)), d, tmax=rng.uniform(0.05, 1.0, n) * diag, time=rng.random(n))
        rnd["time"] = np.minimum(rnd["time"], np.float32(1.0) - np.float32(2.0 ** -24))
        sets = {"camera": cam, "random": rnd}
        for a in sets.values():
            a.setflags(write=False)
        _cache[name] = (hs, sets)
    return _cache[name]


def _words(hits):
    return hits.view(np.uint32).reshape(-1, 4)


@pytest.mark.parametrize("name", NAMES)
def test_k1_equals_closest_hit(name, tmp_path_factory):
    hs, sets = _scene(name, tmp_path_factory)
    for label, rays in sets.items():
        want = hs.trace(rays)
        got, cnt = hs.trace_multi(rays, 1, counts=True)
        assert got.shape == (rays.size, 1)
        bad = np.flatnonzero((_words(got) != _words(want)).any(1))
        assert bad.size == 0, (name, label, bad[:8], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(cnt, (want["object"] >= 0).astype(np.int32))
        assert (want["object"] >= 0).any(), (name, label)
        assert hs.trace_multi(rays, 1, coherent=True).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_k1_equals_closest_hit_on_edge_rays(name):
    """Every ray of the committed edge-ray fixtures (the reference's own answers for them are
    what test_edge_rays_host.py holds HostScene.trace to): tmax <= 0, NaN, zero direction
    components, origins in box planes and on faces."""
    rays = load_golden(name)["rays"]
    hs = rtgpu.HostScene(name + ".xml")
    want = hs.trace(rays)
    got = hs.trace_multi(rays, 1)
    bad = np.flatnonzero((_words(got) != _words(want)).any(1))
    assert bad.size == 0, (name, bad[:8], rays[bad[:8]], got[bad[:8]], want[bad[:8]])
    # and the structure of a longer list on the same rays
    _check_structure(hs, rays, name)


def _sheet_of(faces, face):
    return int(round(-float(faces[face]["v0"][2])))


def test_layered_analytic(tmp_path):
    hs = ms.load_layered(tmp_path)
    _, objs, meshes, faces = qu.scene_arrays(hs)
    xy = ms.axis_points(64, seed=11)
    rays = ms.axis_rays(xy)
    want = ms.axis_answer(xy)
    hits8, cnt8 = hs.trace_multi(rays, 8, counts=True)
    assert np.all(cnt8 == 8)
    for i in range(len(xy)):
        for j in range(8):
            t, obj, sheet, _ = want[i][j]
            h = hits8[i, j]
            assert int(h["object"]) == obj and _sheet_of(faces, int(h["face"])) == sheet, (i, j, h, want[i][j])
            assert abs(float(h["t"]) - t) <= 1e-5 * t, (i, j, h, t)
            m = meshes[objs[obj]["mesh"]]
            assert m["face_offset"] <= h["face"] < m["face_offset"] + m["face_count"]
        # the tie at z = -5: object 0, then object 1, identical bits
        assert (int(hits8[i, 4]["object"]), int(hits8[i, 5]["object"])) == (0, 1)
        assert hits8["t"][i, 4].view(np.uint32) == hits8["t"][i, 5].view(np.uint32)
    # the whole list, walked 8 at a time from origins further down: sheets, then the six roots
    for z0, skip in ((0.0, 0), (-5.5, 6), (-10.5, 11)):
        got, cnt = hs.trace_multi(ms.axis_rays(xy, z0=z0), 8, counts=True)
        for i in range(len(xy)):
            tail = want[i][skip:skip + 8]
            assert cnt[i] == len(tail) == 8
            for j, (t, obj, sheet, face) in enumerate(tail):
                h = got[i, j]
                assert int(h["object"]) == obj, (z0, i, j, h)
                assert abs(float(h["t"]) - (t + z0)) <= 1e-5 * (t + z0), (z0, i, j, h, t + z0)
                if sheet:
                    assert _sheet_of(faces, int(h["face"])) == sheet
                else:
                    assert int(h["face"]) == face, (z0, i, j, h)       # -1: the selected root, -2: the other
    # from the spheres' centre plane upwards: the near roots are behind the origin, so the far one
    # is the root the reference selects (-1) and nothing else of the sphere is reported
    up, cnt = hs.trace_multi(ms.axis_rays(xy, z0=ms.SPHERE_Z, down=False), 8, counts=True)
    assert np.all(cnt == 8)
    assert np.all(up["object"][:, :3] == np.array([2, 3, 4])) and np.all(up["face"][:, :3] == -1)
    assert np.all(up["object"][:, 3:] == 0)
    assert [_sheet_of(faces, int(f)) for f in up["face"][0, 3:]] == [12, 11, 10, 9, 8]
    # from inside the inner sphere downwards: three far roots, all selected, and nothing else
    down, cnt = hs.trace_multi(ms.axis_rays(xy, z0=ms.SPHERE_Z), 8, counts=True)
    assert np.all(cnt == 3) and np.all(down["face"][:, :3] == -1) and np.all(down["object"][:, :3] == [2, 3, 4])
    # a finite tmax strictly between sheets 3 and 4, and one equal to a hit's own t (strict <)
    got, cnt = hs.trace_multi(ms.axis_rays(xy, tmax=3.5), 8, counts=True)
    assert np.all(cnt == 3) and got[:, :3].tobytes() == hits8[:, :3].tobytes()
    assert np.all(got["t"][:, 3:] == np.float32(3.5)) and np.all(got["object"][:, 3:] == -1)
    for j, left in ((2, 2), (4, 4), (5, 4), (6, 6)):        # slots 4 and 5 tie: tmax = that t drops both
        r = ms.axis_rays(xy)
        r["tmax"] = hits8["t"][:, j]
        got, cnt = hs.trace_multi(r, 8, counts=True)
        assert np.all(cnt == left), (j, cnt)
        assert got[:, :left].tobytes() == hits8[:, :left].tobytes()


def _brute_check(name, hs, rays, min_three):
    _, objs, meshes, faces = qu.scene_arrays(hs)
    k = 8
    got, cnt = hs.trace_multi(rays, k, counts=True)
    ref, grazing = ms.brute_force_all(objs, meshes, faces, qu.origins(rays), qu.directions(rays))
    near = np.zeros(rays.size, bool)
    for i, lst in enumerate(ref):
        t = np.array([h[0] for h in lst[:k + 1]])
        near[i] = t.size > 1 and bool(np.any(np.diff(t) <= 1e-4 * np.maximum(1.0, t[1:])))
    skip = grazing | near
    n_ref = np.array([min(len(lst), k) for lst in ref])
    print(name, "rays", rays.size, "grazing", int(grazing.sum()), "near ties", int(near.sum()), "excluded",
          int(skip.sum()), "with >= 3 hits", int((n_ref >= 3).sum()), "with 8", int((n_ref == 8).sum()))
    assert skip.mean() <= 0.01
    worst = 0.0
    for i in np.flatnonzero(~skip):
        lst = ref[i][:k]
        assert cnt[i] == len(lst), (name, int(i), rays[i], got[i], lst)
        for j, (t, obj) in enumerate(lst):
            assert int(got["object"][i, j]) == obj, (name, int(i), j, got[i], lst)
            rel = abs(float(got["t"][i, j]) - t) / max(1.0, abs(t))
            worst = max(worst, rel)
            assert rel <= 1e-4, (name, int(i), j, got[i], lst)
    print(name, "max relative t error", worst)
    if min_three:
        assert (n_ref[~skip] >= 3).mean() >= 0.25 and (n_ref[~skip] == 8).any()
    return n_ref


def test_brute_force_two_spheres(tmp_path_factory):
    hs, _ = _scene("two_spheres", tmp_path_factory)
    n_ref = _brute_check("two_spheres", hs, _cone_rays(qu.camera_record(hs), 4096, seed=20250), False)
    assert set(np.unique(n_ref)) == {0, 2}       # no ray of the cone meets both spheres: two roots or none


def test_brute_force_layered(tmp_path_factory):
    hs, _ = _scene("layered", tmp_path_factory)
    _brute_check("layered", hs, ms.slanted_rays(4096, seed=20253), True)


def _check_structure(hs, rays, name):
    full, cnt8 = hs.trace_multi(rays, 8, counts=True)
    t8 = full["t"].astype(np.float64)
    # rays whose held distances are pairwise further apart than 1e-4 relative
    apart = np.ones(rays.size, bool)
    for j in range(7):
        both = cnt8 > j + 1
        with np.errstate(invalid="ignore"):             # (unfilled slots: inf - inf)
            apart &= ~both | (t8[:, j + 1] - t8[:, j] > 1e-4 * np.maximum(1.0, np.abs(t8[:, j + 1])))
    for k in KS:
        got, cnt = hs.trace_multi(rays, k, counts=True)
        assert got.shape == (rays.size, k) and got.strides == (rtgpu.HIT_DTYPE.itemsize * k, rtgpu.HIT_DTYPE.itemsize)
        slot = np.arange(k)[None, :]
        filled = slot < cnt[:, None]
        assert np.array_equal(got["object"] >= 0, filled), name            # filled slots first; counts
        assert np.all(got["pad"] == 0)
        # unfilled slots are exactly the miss record: tmax's own bits, object = face = -1
        tmax_bits = np.broadcast_to(rays["tmax"].view(np.uint32)[:, None], (rays.size, k))
        assert np.array_equal(got["t"].view(np.uint32)[~filled], tmax_bits[~filled]), name
        assert np.all(got["face"][~filled] == -1)
        assert np.all(got["face"][filled] >= -2)
        # ascending within a ray, positive, below tmax
        pair = filled[:, 1:]
        assert np.all(got["t"][:, 1:][pair] >= got["t"][:, :-1][pair]), name
        assert np.all(got["t"][filled] > 0) and np.all(got["t"][filled] < np.broadcast_to(rays["tmax"][:, None], (rays.size, k))[filled])
        # a prefix of the answer for 8
        bad = np.flatnonzero(apart & (_words(got).reshape(rays.size, -1) != _words(full[:, :k]).reshape(rays.size, -1)).any(1))
        assert bad.size == 0, (name, k, bad[:8], got[bad[:4]], full[bad[:4]])
        assert np.array_equal(cnt[apart], np.minimum(cnt8, k)[apart])
    return cnt8


@pytest.mark.parametrize("name", NAMES)
def test_structure(name, tmp_path_factory):
    hs, sets = _scene(name, tmp_path_factory)
    for label, rays in sets.items():
        cnt8 = _check_structure(hs, rays, (name, label))
        print(name, label, "rays", rays.size, "mean hits held of 8:", float(cnt8.mean()))


def test_argument_errors(tmp_path):
    L = rtgpu.lib()
    for sym in ("rtg_trace_rays_multi_device", "rtg_trace_rays_multi", "rtg_desc_trace_rays_multi"):
        assert hasattr(L, sym) and sym in rtgpu.EXPORTED
    assert L.rtg_abi_version() == 6 and rtgpu.RTG_MULTIHIT_MAX == 8
    hs = rtgpu.HostScene("simple.xml")
    rays = rtgpu.make_rays([[0, 0, 0]], [[0, 0, -1]])
    hits = np.zeros((1, 8), rtgpu.HIT_DTYPE)
    cnt = np.zeros(1, np.int32)
    f = L.rtg_desc_trace_rays_multi

    def err():
        return L.rtg_last_error().decode()

    assert f(hs.desc, rays.ctypes.data, 0, 1, 0, hits.ctypes.data, None) == 0            # n = 0
    assert hs.trace_multi(np.zeros(0, rtgpu.RAY_DTYPE), 3).shape == (0, 3)
    assert f(hs.desc, None, 1, 1, 0, hits.ctypes.data, None) == -1 and "null" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 1, 0, None, None) == -1 and "null" in err()
    assert f(None, rays.ctypes.data, 1, 1, 0, hits.ctypes.data, None) == -1 and "null" in err()
    assert f(hs.desc, rays.ctypes.data, 1 << 31, 1, 0, hits.ctypes.data, None) == -1 and "ray count" in err()
    assert f(hs.desc, rays.ctypes.data, -1, 1, 0, hits.ctypes.data, None) == -1
    for k in (0, -1, 9, 1 << 20):
        assert f(hs.desc, rays.ctypes.data, 1, k, 0, hits.ctypes.data, None) == -1 and "k out of range" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 1, rtgpu.RTG_QUERY_ANY_HIT, hits.ctypes.data, None) == -1
    assert "RTG_QUERY_ANY_HIT" in err()
    assert f(hs.desc, rays.ctypes.data, 1, 1, 4, hits.ctypes.data, None) == -1 and "unknown query flags" in err()
    # the good call, with and without counts and the hint
    assert f(hs.desc, rays.ctypes.data, 1, 8, 0, hits.ctypes.data, cnt.ctypes.data) == 0
    assert hits["object"][0, 0] == 0 and hits["t"][0, 0] == 2.0 and cnt[0] >= 1
    assert f(hs.desc, rays.ctypes.data, 1, 8, rtgpu.RTG_QUERY_COHERENT, hits.ctypes.data, None) == 0
    nb = rtgpu.HostScene("simple.xml", device_bvh=True)
    with pytest.raises(rtgpu.RTGError) as e:
        nb.trace_multi(rays, 2)
    assert e.value.code == -1 and "RTG_LOAD_DEVICE_BVH" in str(e.value)
    with pytest.raises(rtgpu.RTGError):
        hs.trace_multi(rays, 9)
    # slot j of ray i is hits[i * k + j]
    assert rtgpu.HIT_DTYPE.itemsize == 16 and ctypes.sizeof(ctypes.c_int32) == 4
    two = np.concatenate([rays, rays])
    assert hs.trace_multi(two, 3).strides == (rtgpu.HIT_DTYPE.itemsize * 3, rtgpu.HIT_DTYPE.itemsize)
