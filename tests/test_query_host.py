"""Ray queries on the host (rtg_desc_trace_rays, HostScene.trace): the reference's
IntersectObjects / CastShadowRay restated over a scene description, no device.  It is the
yardstick of the device queries (test_gpu_query.py), so it is checked here against two independent
sources: the reference's own golden images (which pixels show the background) and a float64
brute force written in NumPy (no BVH, no shared code)."""
import ctypes
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu

SCENES = os.path.join(ob.GOLDEN, "scenes")


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


_cache = {}


def _scene(name):
    """(HostScene, camera record, pixel-centre rays, their closest hits) -- computed once."""
    if name not in _cache:
        hs = rtgpu.HostScene(name + ".xml")
        cam = qu.camera_record(hs)
        rays = qu.numpy_camera_rays(cam)
        hits = hs.trace(rays)
        for a in (rays, hits):
            a.setflags(write=False)
        _cache[name] = (hs, cam, rays, hits)
    return _cache[name]


@pytest.mark.parametrize("name", ["simple", "spheres", "two_spheres", "synth_10k"])
def test_miss_mask_equals_reference_golden(name):
    """1 spp, no depth of field, constant background, ambient light x ambient reflectance >= 20
    on every channel: a pixel of the reference's image equals the background colour exactly
    where its camera ray hits nothing -- every pixel, no exceptions."""
    hs, cam, rays, hits = _scene(name)
    assert cam["aperture"] <= 0.0001
    bg = qu.scene_arrays(hs)[0].astype(np.float32)
    gold = ob.load_golden(name)
    assert gold.shape == (cam["height"], cam["width"], 3)
    gold_bg = (gold == bg[None, None, :]).all(axis=2).reshape(-1)
    miss = hits["object"] < 0
    print(name, "pixels", miss.size, "misses", int(miss.sum()), "disagreeing", int((miss != gold_bg).sum()))
    assert np.array_equal(miss, gold_bg)       # (`spheres` and `synth_10k` fill their frames: no miss)
    # a miss keeps tmax and has no face; a hit has a positive finite distance
    assert np.all(np.isinf(hits["t"][miss])) and np.all(hits["face"][miss] == -1)
    assert np.all((hits["t"][~miss] > 0) & np.isfinite(hits["t"][~miss]))


def _cone_rays(cam, n, seed):
    """n seeded rays from the camera position through uniform points of the image plane."""
    rng = np.random.default_rng(seed)
    u = rng.random(n) * (float(cam["right_ext"]) - float(cam["left"]))
    v = rng.random(n) * (float(cam["top"]) - float(cam["bottom"]))
    p = cam["q"].astype(np.float64)[None] + cam["right"].astype(np.float64)[None] * u[:, None] \
        - cam["up"].astype(np.float64)[None] * v[:, None]
    d = p - cam["position"].astype(np.float64)[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rtgpu.make_rays(np.broadcast_to(cam["position"], (n, 3)), d)


@pytest.mark.parametrize("name", ["simple", "two_spheres"])
def test_against_float64_brute_force(name):
    """4 096 seeded rays into the view cone against all faces and all spheres in float64: hit or
    miss and the object agree on every ray that is not grazing (barycentrics within 1e-5 of an
    edge, sphere discriminant within 1e-5 b^2: at most 1 % of the rays), t within relative 1e-4
    (oracle_bind.compare's tolerance)."""
    hs, cam, _, _ = _scene(name)
    _, objs, meshes, faces = qu.scene_arrays(hs)
    rays = _cone_rays(cam, 4096, seed=20250)
    hits = hs.trace(rays)
    t, k, grazing = qu.brute_force(objs, meshes, faces, qu.origins(rays), qu.directions(rays))
    print(name, "grazing", int(grazing.sum()), "hits", int((k >= 0).sum()))
    assert grazing.mean() <= 0.01
    keep = ~grazing
    assert 0 < (k[keep] >= 0).sum() < keep.sum()
    assert np.array_equal(hits["object"][keep], k[keep])
    hit = keep & (k >= 0)
    rel = np.abs(hits["t"][hit].astype(np.float64) - t[hit]) / np.maximum(1.0, np.abs(t[hit]))
    print(name, "max relative t error", rel.max())
    assert np.all(rel <= 1e-4)
    # faces are global indices into faces[] (BVH order) of the hit object's mesh; -1 for spheres
    for i in np.flatnonzero(hit):
        o = objs[hits["object"][i]]
        if o["kind"] == qu.RTG_OBJ_SPHERE:
            assert hits["face"][i] == -1
        else:
            m = meshes[o["mesh"]]
            assert m["face_offset"] <= hits["face"][i] < m["face_offset"] + m["face_count"]


def test_normals():
    """Unit length everywhere; +-(0,0,1) on the meshes of `simple` (all in the plane z = -2)
    within 1e-6; radial on `two_spheres` within 1e-5; zeros for a miss."""
    for name in ("simple", "two_spheres"):
        hs, cam, rays, hits0 = _scene(name)
        hits, nrm = hs.trace(rays, normals=True)
        assert hits.tobytes() == hits0.tobytes()
        hit = hits["object"] >= 0
        assert np.all(nrm[~hit] == 0) and np.all(nrm[:, 3] == 0)
        assert np.all(np.abs(np.linalg.norm(nrm[hit, :3].astype(np.float64), axis=1) - 1.0) <= 1e-6)
        _, objs, _, _ = qu.scene_arrays(hs)
        sphere = objs["kind"][np.maximum(hits["object"], 0)] == qu.RTG_OBJ_SPHERE
        mesh = hit & ~sphere
        if name == "simple":
            assert mesh.any()
            n = nrm[mesh, :3]
            assert np.all(np.abs(np.abs(n[:, 2]) - 1.0) <= 1e-6) and np.all(np.abs(n[:, :2]) <= 1e-6)
        sp = hit & sphere
        assert sp.any()
        p = qu.origins(rays)[sp].astype(np.float64) + qu.directions(rays)[sp].astype(np.float64) * \
            hits["t"][sp].astype(np.float64)[:, None]
        o = objs[hits["object"][sp]]
        radial = (p - o["center"].astype(np.float64)) / o["radius"].astype(np.float64)[:, None]
        err = np.abs(nrm[sp, :3] - radial).max()
        print(name, "max radial normal error", err)
        assert err <= 1e-5


@pytest.mark.parametrize("name", ["simple", "spheres", "two_spheres", "synth_10k"])
def test_occlusion_equals_closest_hit(name):
    """Scenes without RTG_OBJF_SHADOW_SKIP objects, time 0, random finite tmax (about half of
    the hits cut off): occluded exactly where the closest-hit query finds something."""
    hs, cam, rays0, hits0 = _scene(name)
    _, objs, _, _ = qu.scene_arrays(hs)
    assert not np.any(objs["flags"] & qu.RTG_OBJF_SHADOW_SKIP)
    rng = np.random.default_rng(7)
    t_typ = float(np.median(hits0["t"][hits0["object"] >= 0]))
    rays = rays0.copy()
    rays["tmax"] = np.where(hits0["object"] >= 0, hits0["t"], t_typ) * rng.uniform(0.5, 1.5, rays.size).astype(np.float32)
    assert np.all(np.isfinite(rays["tmax"]))
    closest = hs.trace(rays)
    occ = hs.trace(rays, any_hit=True)
    found = closest["object"] >= 0
    assert 0 < found.sum() < (hits0["object"] >= 0).sum()       # tmax cut some hits off
    assert np.all(closest["t"][found] < rays["tmax"][found])
    assert np.all(closest["t"][~found] == rays["tmax"][~found])
    assert set(np.unique(occ["object"])) <= {0, -1}
    assert np.array_equal(occ["object"] == 0, found)
    # the motion-blur time is ignored by occlusion queries
    rays["time"] = 0.75
    assert np.array_equal(hs.trace(rays, any_hit=True)["object"], occ["object"])


def test_occlusion_skips_emissive_mesh():
    """`mesh_light`: the light quad (y = 1.99, under the ceiling at y = 2) is RTG_OBJF_SHADOW_SKIP.
    Rays from the box's middle straight up: the closest hit is the light, but an occlusion query
    that ends between the light and the ceiling sees nothing; one that reaches the ceiling is
    occluded."""
    hs = rtgpu.HostScene("mesh_light.xml")
    _, objs, _, _ = qu.scene_arrays(hs)
    skip = np.flatnonzero(objs["flags"] & qu.RTG_OBJF_SHADOW_SKIP)
    assert len(skip) == 1
    rng = np.random.default_rng(3)
    n = 256
    o = np.zeros((n, 3), np.float32)
    o[:, 0], o[:, 2] = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
    o[:, 1] = 1.0
    d = np.tile(np.array([0, 1, 0], np.float32), (n, 1))
    short = rtgpu.make_rays(o, d, tmax=0.995)        # ends at y = 1.995
    closest = hs.trace(short)
    assert np.all(closest["object"] == skip[0])
    assert np.allclose(closest["t"], 0.99, atol=1e-5)
    assert np.all(hs.trace(short, any_hit=True)["object"] == -1)
    far = rtgpu.make_rays(o, d, tmax=np.inf)
    assert np.all(hs.trace(far)["object"] == skip[0])
    assert np.all(hs.trace(far, any_hit=True)["object"] == 0)


def test_argument_errors():
    L = rtgpu.lib()
    hs = rtgpu.HostScene("simple.xml")
    rays = rtgpu.make_rays([[0, 0, 0]], [[0, 0, -1]])
    hits = np.zeros(1, rtgpu.HIT_DTYPE)
    # n = 0 is fine, also on empty arrays through the wrapper
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, 0, 0, hits.ctypes.data, None) == 0
    assert hs.trace(np.zeros(0, rtgpu.RAY_DTYPE)).size == 0
    # null buffers, null description, ray count out of range, unknown flags
    assert L.rtg_desc_trace_rays(hs.desc, None, 1, 0, hits.ctypes.data, None) == -1
    assert b"null" in L.rtg_last_error()
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, 1, 0, None, None) == -1
    assert L.rtg_desc_trace_rays(None, rays.ctypes.data, 1, 0, hits.ctypes.data, None) == -1
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, (1 << 31), 0, hits.ctypes.data, None) == -1
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, -1, 0, hits.ctypes.data, None) == -1
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, 1, 4, hits.ctypes.data, None) == -1
    # the good call still works, and a description without nodes is refused
    assert L.rtg_desc_trace_rays(hs.desc, rays.ctypes.data, 1, 0, hits.ctypes.data, None) == 0
    assert hits["object"][0] == 0 and hits["t"][0] == 2.0
    nb = rtgpu.HostScene("simple.xml", device_bvh=True)
    assert nb.counts()["nodes"] == 0
    with pytest.raises(rtgpu.RTGError) as e:
        nb.trace(rays)
    assert e.value.code == -1 and "RTG_LOAD_DEVICE_BVH" in str(e.value)
    assert ctypes.sizeof(ctypes.c_float) * 8 == rtgpu.RAY_DTYPE.itemsize and rtgpu.HIT_DTYPE.itemsize == 16
