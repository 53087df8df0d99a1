"""Surface queries on the device (DeviceScene.surface, rtg_surface_rays*): shading normal, texture
coordinates, material and diffuse coefficient at the closest hit of caller rays.

  identity     t / object / face / ng are DeviceScene.trace's bit for bit, the material is the
               description's, a miss is all zero, the coherent hint changes nothing, and n / kd are ng /
               the material's bits wherever no map / no diffuse texture is in effect
  waves        partial blocks and batches that mix misses, spheres, meshes and instances in every wave
               equal the same rays in one plain call; so does the device-resident entry point
  re-lighting  n, kd and p from surface() predict what the CPU oracle renders of the relit scene
               (surface_rays.py; the relation itself is checked without the device in
               test_surface_abi.py): three lights pin the three components of n, kd pins uv and the
               texture path
  uv           u, v against a float64 recomputation from the description

Rays: the camera's own (DeviceScene.camera_rays) plus radiance_rays.generate's probes, surface origins,
back faces, bounded rays, times and misses."""
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import radiance_rays as rr
import rtgpu
import surface_rays as sr

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
IDENTITY = ["simple", "spheres", "transforms_textures", "bump_normal", "dof_motion", "cornell_dielectric", "edge_roof",
            "synth_10k", "image_tex", "ply_quads"]
RELIT = ["simple", "spheres", "cornell_dielectric", "image_tex", "transforms_textures", "bump_normal"]
# Offsets of the green and blue lights as a share of the default (a third of the median hit distance).
# cornell_dielectric: only 50.6 % of the camera's hits have a diffuse coefficient with a green component
# at all (the others are the red wall and the two bodies), so "half of the hits lit in green" leaves
# room for 0.6 % of shadowed or back-facing points: the lights sit close to the eye there.  The scene
# has no maps, so its normal is pinned bit for bit by the identity test.
LIGHT_SHARE = {"cornell_dielectric": 0.1}
UV_MESH = ["image_tex", "bump_normal", "transforms_textures"]
UV_SPHERE = ["bump_normal", "spheres"]
NORM_TOL = 1e-6             # makeUnit in float32: a few roundings of 2^-24

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)
    _cache.clear()


def _scene(name):
    """(hs, ds, rays, n_cam, surface(rays)) once per module run."""
    if name not in _cache:
        hs = rtgpu.HostScene(name + ".xml")
        ds = rtgpu.DeviceScene(hs, 0)
        cam = ds.camera_rays()
        off, _, _ = rr.generate(hs)
        rays = np.concatenate([cam, off])
        surf = ds.surface(rays)
        for a in (rays, surf):
            a.setflags(write=False)
        _cache[name] = (hs, ds, rays, cam.size, surf)
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 3. identity with the existing queries
@pytest.mark.parametrize("name", IDENTITY)
def test_identity_with_trace(name):
    hs, ds, rays, n_cam, s = _scene(name)
    assert s.dtype == rtgpu.SURFACE_DTYPE and s.size == rays.size
    hits, nrm = ds.trace(rays, normals=True)
    objs = qu.scene_arrays(hs)[1]
    hit = hits["object"] >= 0
    print(name, "rays", rays.size, "camera", n_cam, "hits", int(hit.sum()), "objects hit", np.unique(hits["object"][hit]).size)
    assert hit.sum() > 100 and (~hit).sum() > 10
    assert np.array_equal(_bits(s["t"]), _bits(hits["t"]))
    assert np.array_equal(s["object"], hits["object"]) and np.array_equal(s["face"], hits["face"])
    assert np.array_equal(_bits(s["ng"]), _bits(nrm[:, :3])) and not _bits(nrm[:, 3]).any()
    assert np.array_equal(s["material"][hit], objs["material"][s["object"][hit]])
    assert not _bits(s["pad"]).any()
    # a miss: t = tmax (its bits), -1 three times, +0.0f everywhere else
    m = s[~hit]
    assert np.array_equal(_bits(m["t"]), _bits(rays["tmax"][~hit]))
    assert (m["object"] == -1).all() and (m["face"] == -1).all() and (m["material"] == -1).all()
    assert not np.ascontiguousarray(m).view(np.uint32).reshape(-1, 16)[:, 4:].any()
    # the hint changes nothing
    assert ds.surface(rays, coherent=True).tobytes() == s.tobytes()
    # kd without a diffuse texture: the material's bits; n without a map: ng's bits
    tex = objs["tex"][s["object"][hit]]
    plain_kd = tex[:, sr.TEX_DIFFUSE] < 0
    kd_mat = sr.material_diffuse(hs)[objs["material"][s["object"][hit]]]
    assert plain_kd.any() or name == "image_tex"                   # (every object of image_tex is textured)
    assert np.array_equal(_bits(s["kd"][hit][plain_kd]), _bits(kd_mat[plain_kd]))
    unmapped = (tex[:, sr.TEX_NORMAL] < 0) & (tex[:, sr.TEX_BUMP] < 0)
    assert unmapped.any() or name == "bump_normal"                 # (every object of bump_normal is mapped)
    assert np.array_equal(_bits(s["n"][hit][unmapped]), _bits(s["ng"][hit][unmapped]))
    if name == "dof_motion":
        moving = np.any(objs["motion_blur"][s["object"][hit]] != 0, 1) & (rays["time"][hit] > 0)
        print(name, "hits on moving objects at time > 0:", int(moving.sum()))
        assert moving.sum() > 50 and unmapped[moving].all()
    if name in ("bump_normal",):
        differs = (_bits(s["n"][hit]) != _bits(s["ng"][hit])).any(1)
        assert differs[~unmapped].mean() > 0.5         # the maps are in effect
    if name in ("image_tex", "transforms_textures"):
        assert (_bits(s["kd"][hit][~plain_kd]) != _bits(kd_mat[~plain_kd])).any(1).mean() > 0.5   # so are the textures
    # unit length -- except where the reference's own arithmetic gives NaN: a hit on the very pole of a
    # sphere, where rounding puts |p.y| above r and acos(p.y / r) is NaN (sr.sphere_poles); v is then
    # NaN, and so is the normal of a bumped sphere, in the render as here.  Nowhere else.
    pole = sr.sphere_poles(hs, rays, s)[hit]
    nan = np.isnan(s["n"][hit]).any(1) | np.isnan(s["v"][hit]) | np.isnan(s["u"][hit])
    print(name, "hits within %g of a sphere's pole" % sr.POLE_NAN, int(pole.sum()), "with a NaN among n, u, v", int(nan.sum()))
    assert not (nan & ~pole).any() and pole.sum() <= 1e-3 * hit.sum()
    assert not np.isnan(s["ng"][hit]).any() and not np.isnan(s["kd"][hit]).any()
    ln = np.sqrt((s["n"][hit][~nan].astype(np.float64) ** 2).sum(1))
    lg = np.sqrt((s["ng"][hit].astype(np.float64) ** 2).sum(1))
    print(name, "max | |n| - 1 | %.3g" % np.abs(ln - 1).max(), "max | |ng| - 1 | %.3g" % np.abs(lg - 1).max())
    assert np.abs(ln - 1).max() <= NORM_TOL and np.abs(lg - 1).max() <= NORM_TOL


def test_empty_batch_is_ok():
    hs, ds, rays, n_cam, s = _scene("simple")
    assert ds.surface(rays[:0]).size == 0
    assert rtgpu.lib().rtg_surface_rays(ds._s, None, 0, 0, None) == 0
    assert rtgpu.lib().rtg_surface_rays_device(ds._s, None, 0, rtgpu.RTG_QUERY_COHERENT, None, None) == 0
    with pytest.raises(rtgpu.RTGError) as e:
        rtgpu._check(rtgpu.lib().rtg_surface_rays(ds._s, rays.ctypes.data, 4, rtgpu.RTG_QUERY_ANY_HIT, s.ctypes.data))
    assert e.value.code == -1


# ---- 4. partial waves and mixed lanes
@pytest.mark.parametrize("name", ["transforms_textures", "bump_normal"])
def test_partial_waves_and_mixed_lanes(name):
    hs, ds, rays, n_cam, s = _scene(name)
    objs = qu.scene_arrays(hs)[1]
    # every wave meets a miss, a sphere, a mesh and an instance: 16 lanes each, dealt by a fixed-seed
    # permutation within the wave
    rng = np.random.default_rng(20272)
    kind_of = np.where(s["object"] < 0, 3, objs["kind"][np.maximum(s["object"], 0)])
    pools = [np.flatnonzero(kind_of == k) for k in range(4)]
    assert all(p.size >= 16 for p in pools), [p.size for p in pools]
    waves = 192
    perm = np.stack([np.concatenate([rng.choice(p, 16, replace=False) for p in pools])[rng.permutation(64)]
                     for _ in range(waves)]).reshape(-1)
    mixed = np.ascontiguousarray(rays[perm])
    want = s[perm]
    kind = kind_of[perm].reshape(waves, 64)
    assert all(np.unique(g).size == 4 for g in kind)
    print(name, "waves", waves, "each with misses, spheres, meshes and instances; pools", [p.size for p in pools])
    for coherent in (False, True):
        full = ds.surface(mixed, coherent=coherent)
        assert full.tobytes() == want.tobytes(), (name, coherent)
        for n in (1, 63, 64, 65, 257, 1000):
            for start in (0, 4096 + 37):
                got = ds.surface(mixed[start:start + n], coherent=coherent)
                assert got.tobytes() == want[start:start + n].tobytes(), (name, coherent, n, start)
    import torch                                                  # only the device-resident submission needs it
    dev = torch.device("cuda:0")
    n = 1000 + 65
    with torch.cuda.device(dev):
        stream = torch.cuda.Stream()
        d_rays = torch.from_numpy(mixed[:n].view(np.float32).reshape(-1, 8)).to(dev)
        d_out = torch.full((n, 16), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for coherent in (False, True):
            d_out.fill_(7.0)
            stream.wait_stream(torch.cuda.current_stream())
            ds.surface_device(d_rays.data_ptr(), n, d_out.data_ptr(), stream=stream.cuda_stream, coherent=coherent)
            stream.synchronize()
            assert d_out.cpu().numpy().tobytes() == want[:n].tobytes(), (name, coherent)


# ---- 5. re-lighting against the CPU oracle
@pytest.mark.parametrize("name", RELIT)
def test_relighting_against_oracle(name, tmp_path):
    """Measured maxima (MI355X): see the table there; the bound is sr.REL = 1e-4 relative
    on lit values with at most sr.CAP = 0.1 % of a scene's values per channel outside it or disagreeing
    about lit / not lit."""
    hs, ds, rays, n_cam, s0 = _scene(name)
    cam = rays[:n_cam]
    eye = qu.origins(cam)[0]
    assert (qu.origins(cam) == eye).all()                          # a pinhole camera: one common origin
    hit0 = s0["object"][:n_cam] >= 0
    median_t = float(np.median(s0["t"][:n_cam][hit0]))
    lights = sr.light_setup(eye, median_t)
    share = np.float32(LIGHT_SHARE.get(name, 1.0))
    lights = [((eye + (p - eye) * share).astype(np.float32), i) for p, i in lights]
    path = tmp_path / (name + "_relit.xml")
    path.write_text(sr.relit(open(name + ".xml").read(), lights))
    hr = rtgpu.HostScene(str(path))
    dr = rtgpu.DeviceScene(hr, 0)
    s = dr.surface(cam)
    for f in ("t", "object", "face", "material"):                  # the geometry did not move
        assert np.array_equal(s[f], s0[f][:n_cam]), f
    assert s["n"].tobytes() == s0["n"][:n_cam].tobytes() and s["kd"].tobytes() == s0["kd"][:n_cam].tobytes()
    want, _ = ob.radiance(hr, cam)
    hit = s["object"] >= 0
    formula = sr.shaded_by_formula(hr)[np.maximum(s["object"], 0)]
    use = hit & formula
    print(name, "camera hits", int(hit.sum()), "on replace_all / textured-specular objects (not compared)", int((hit & ~formula).sum()))
    assert use.sum() > 0.6 * hit.sum()
    pred = sr.predict(hr, cam[use], s["t"][use], s["n"][use], s["kd"][use], lights)
    res = sr.compare_relit(want[use, :3], pred)
    print(name, "values per channel", res["m"], "lit", res["lit"], "outside 1e-4", res["outside"], "lit / not lit disagree",
          res["disagree"], "max rel", ["%.3g" % x for x in res["max_rel"]])
    assert min(res["lit"]) >= 0.5 * res["m"], (name, "too few lit values: move the lights", res)
    assert sr.relit_ok(res), (name, res)
    if name == "transforms_textures":
        # the test does see the textures: with the material's coefficient instead it fails outright
        objs = qu.scene_arrays(hr)[1]
        kd_mat = sr.material_diffuse(hr)[objs["material"][s["object"][use]]]
        blind = sr.compare_relit(want[use, :3], sr.predict(hr, cam[use], s["t"][use], s["n"][use], kd_mat, lights))
        print(name, "with the material's kd: outside", blind["outside"], "of", blind["lit"])
        assert not sr.relit_ok(blind)
    if name == "bump_normal":
        blind = sr.compare_relit(want[use, :3], sr.predict(hr, cam[use], s["t"][use], s["ng"][use], s["kd"][use], lights))
        print(name, "with the geometric normal: outside", blind["outside"], "of", blind["lit"])
        assert not sr.relit_ok(blind)


# ---- 6. uv directly
@pytest.mark.parametrize("name", sorted(set(UV_MESH + UV_SPHERE)))
def test_uv_against_float64(name):
    """Measured maxima (MI355X): see the table there."""
    hs, ds, rays, n_cam, s = _scene(name)
    objs, meshes = qu.scene_arrays(hs)[1:3]
    uv, valid, excluded = sr.expected_uv(hs, rays, s)
    sphere = valid & (objs["kind"][np.maximum(s["object"], 0)] == qu.RTG_OBJ_SPHERE)
    mesh = valid & ~sphere
    print(name, "rays with uv", int(valid.sum()), "mesh", int(mesh.sum()), "sphere", int(sphere.sum()), "left out (near a wrap, the seam or a pole; grazing)",
          int(excluded.sum()))
    if name in UV_MESH:
        assert mesh.sum() > 1000
    if name in UV_SPHERE:
        assert sphere.sum() > 500
    assert excluded.sum() < sr.UV_EXCLUDED_CAP * valid.sum()
    # a mesh without UVs reports 0
    no_uv = (s["object"] >= 0) & ~valid & (objs["kind"][np.maximum(s["object"], 0)] != qu.RTG_OBJ_SPHERE)
    no_uv &= meshes["has_uv"][objs["mesh"][np.maximum(s["object"], 0)]] == 0
    assert not _bits(s["u"][no_uv]).any() and not _bits(s["v"][no_uv]).any()
    keep = valid & ~excluded
    got = np.stack([s["u"][keep], s["v"][keep]], 1).astype(np.float64)
    dev = np.abs(got - uv[keep]) / np.maximum(1.0, np.abs(uv[keep]))
    for label, sel in (("mesh", mesh[keep]), ("sphere", sphere[keep])):
        if sel.any():
            print(name, label, "max |d| / max(1, |uv|): u %.3g v %.3g" % (np.nanmax(dev[sel, 0]), np.nanmax(dev[sel, 1])))
    bad = np.flatnonzero(~(dev <= sr.UV_REL).all(1))               # (a NaN is outside the bound)
    for i in bad[:8]:
        k = np.flatnonzero(keep)[i]
        print("  ", name, "ray", int(k), rays[k], "object", int(s["object"][k]), "face", int(s["face"][k]), "t", float(s["t"][k]),
              "device uv", got[i].tolist(), "float64 uv", uv[k].tolist())
    assert bad.size == 0, (name, bad.size)
