"""Radiance queries on the device (rtg_radiance_rays*; rtg_radiance.hip) against the render, which
the oracle pins to the reference's goldens: on the camera's own rays a radiance query must give the
fused render's image bit for bit -- every MAXD / PT instantiation, every light kind, texture,
background-texture and environment misses, depth of field with motion blur, large leaves -- and on
other rays it must follow its documented semantics (eye, pixel ids, tmax, sample sums) exactly.
All comparisons are on raw bits unless said otherwise."""
import ctypes
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
FUSED = rtgpu.RTG_RENDER_FUSED
RENDER_NAMES = ["simple", "spheres_mirror", "cornell_dielectric", "cornell_conductors", "brdf_lights", "area_light",
                "env_light", "image_tex", "transforms_textures", "bump_normal", "mesh_light", "dof_motion",
                "pt_cornell", "pt_nee", "pt_rr", "pt_meshlight", "defer_gate"]


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _load(name, tmp_path):
    """(HostScene, DeviceScene) of a fixture whose cameras all take one sample; `defer_gate` is
    generated (large leaves: FEAT_BIGLEAF), as in test_gpu_query.py."""
    if name == "defer_gate":
        import scenes
        xml = scenes.config_defer_gate(str(tmp_path))
        old = os.getcwd()
        os.chdir(tmp_path)
        try:
            hs = rtgpu.HostScene(xml)
            ds = rtgpu.DeviceScene(hs, 0)
        finally:
            os.chdir(old)
    else:
        hs = rtgpu.HostScene(name + ".xml")
        if hs.camera(0)["spp"] != 1:
            hs.close()
            copy = tmp_path / (name + "_1spp.xml")
            copy.write_text(ob.with_samples(open(name + ".xml").read(), 1))
            hs = rtgpu.HostScene(str(copy))
        ds = rtgpu.DeviceScene(hs, 0)
    assert hs.camera(0)["spp"] == 1
    return hs, ds


_cache = {}


def _scene(name, tmp_path_factory):
    """One scene per module run: (hs, ds, rays, image) with rays = camera_rays(seed) and image the
    radiance of them under the camera's eye (test 1 holds it to the render); never modified."""
    if name not in _cache:
        hs, ds = _load(name, tmp_path_factory.mktemp(name))
        seed = 0xC0FFEE
        rays = ds.camera_rays(seed=seed)
        img = ds.radiance(rays, seed=seed, camera_eye=True)
        rays.setflags(write=False)
        img.setflags(write=False)
        _cache[name] = (hs, ds, seed, rays, img)
    return _cache[name]


# ---- 1. camera rays reproduce the render
@pytest.mark.parametrize("name", RENDER_NAMES)
def test_camera_rays_reproduce_render(name, tmp_path_factory):
    hs, ds, seed, rays, img = _scene(name, tmp_path_factory)
    hdr, _ = ds.render(0, flags=FUSED, seed=seed)
    want = hdr.reshape(-1, 3)
    assert img.shape == (rays.size, 4) and img.dtype == np.float32
    diff = int((_bits(img[:, :3]) != _bits(want)).sum())
    t = ds.trace(rays)["t"]
    tdiff = int((_bits(img[:, 3]) != _bits(t)).sum())
    print(name, "rays", rays.size, "differing values", diff, "differing t", tdiff, "hits", int(np.isfinite(t).sum()),
          "distinct colours", len(np.unique(_bits(want), axis=0)))
    assert diff == 0
    assert tdiff == 0
    assert len(np.unique(_bits(want), axis=0)) > 1          # not a blank frame


def test_camera_rays_reproduce_wavefront_render(tmp_path_factory):
    """A plain scene: also the image of the pipeline rtg_render chooses by itself (flags = 0)."""
    hs, ds, seed, rays, img = _scene("simple", tmp_path_factory)
    hdr, _ = ds.render(0, flags=0, seed=seed)
    diff = int((_bits(img[:, :3]) != _bits(hdr.reshape(-1, 3))).sum())
    print("simple flags=0 differing values", diff)
    assert diff == 0


# ---- 2. eye = ray origin, on rays that are not the camera's
def test_eye_is_ray_origin_other_camera():
    """car_smooth: two cameras of equal resolution over specular and mirror materials.  Camera
    1's rays shaded under opts.camera = 0 (flags and image size only) are camera 1's render; with
    the eye moved to camera 0's position the highlights move."""
    hs = rtgpu.HostScene("car_smooth.xml")
    ds = rtgpu.DeviceScene(hs, 0)
    c0, c1 = hs.camera(0), hs.camera(1)
    assert (c0["width"], c0["height"]) == (c1["width"], c1["height"]) and c0["spp"] == c1["spp"] == 1
    rays = ds.camera_rays(camera=1)
    want = ds.render(1, flags=FUSED)[0].reshape(-1, 3)
    got = ds.radiance(rays, camera=0)
    diff = int((_bits(got[:, :3]) != _bits(want)).sum())
    eye = ds.radiance(rays, camera=0, camera_eye=True)
    moved = int((_bits(eye[:, :3]) != _bits(want)).any(axis=1).sum())
    print("car_smooth rays", rays.size, "differing values", diff, "pixels moved by the camera eye", moved)
    assert diff == 0
    assert moved > 0
    assert np.array_equal(_bits(eye[:, 3]), _bits(got[:, 3]))          # the eye moves no hit


def test_eye_is_ray_origin_depth_of_field(tmp_path_factory):
    """dof_motion: the lens moves the rays' origins off the camera's position, so without the flag
    some pixels differ from the render; background pixels (no primary hit, no eye) never do."""
    hs, ds, seed, rays, img = _scene("dof_motion", tmp_path_factory)
    hdr = ds.render(0, flags=FUSED, seed=seed)[0].reshape(-1, 3)
    got = ds.radiance(rays, seed=seed)
    bg = qu.scene_arrays(hs)[0].astype(np.float32)
    is_bg = (hdr == bg[None, :]).all(axis=1)
    differs = (_bits(got[:, :3]) != _bits(hdr)).any(axis=1)
    print("dof_motion pixels", differs.size, "background", int(is_bg.sum()), "differing", int(differs.sum()),
          "differing on background", int((differs & is_bg).sum()))
    assert 0 < is_bg.sum() < is_bg.size
    assert differs.any()
    assert not (differs & is_bg).any()
    assert np.array_equal(_bits(got[:, 3]), _bits(img[:, 3]))


# ---- 3. order, ids and tails
def test_pixel_ids_permute(tmp_path_factory):
    hs, ds, seed, rays, img = _scene("area_light", tmp_path_factory)
    rng = np.random.default_rng(20258)
    perm = rng.permutation(rays.size).astype(np.int32)
    got = ds.radiance(rays[perm], seed=seed, pixel_ids=perm, camera_eye=True)
    diff = int((_bits(got) != _bits(img[perm])).sum())
    # the scene is stochastic: under the wrong pixels' keys the colours change
    wrong = ds.radiance(rays[perm], seed=seed, camera_eye=True)
    print("area_light permuted rays", perm.size, "differing values", diff, "differing without ids",
          int((_bits(wrong) != _bits(img[perm])).sum()))
    assert diff == 0
    assert (_bits(wrong) != _bits(img[perm])).any()


def test_first_pixel_tail(tmp_path_factory):
    hs, ds, seed, rays, img = _scene("area_light", tmp_path_factory)
    for k in (1, 64, 1000, rays.size - 1):
        got = ds.radiance(rays[k:], seed=seed, first_pixel=k, camera_eye=True)
        assert np.array_equal(_bits(got), _bits(img[k:])), k
    print("area_light tails ok")


@pytest.mark.parametrize("name", ["spheres_mirror", "defer_gate"])
def test_partial_waves_and_blocks(name, tmp_path_factory):
    """n in {1, 63, 65, 257} of permuted rays: partial waves and blocks with divergent trees."""
    hs, ds, seed, rays, img = _scene(name, tmp_path_factory)
    rng = np.random.default_rng(20259)
    perm = rng.permutation(rays.size).astype(np.int32)
    for n in (1, 63, 65, 257):
        got = ds.radiance(rays[perm[:n]], seed=seed, pixel_ids=perm[:n], camera_eye=True)
        diff = int((_bits(got) != _bits(img[perm[:n]])).sum())
        print(name, "n", n, "differing values", diff, "hits", int(np.isfinite(got[:, 3]).sum()))
        assert got.shape == (n, 4)
        assert diff == 0, (name, n)


def test_equal_ids_equal_colours(tmp_path_factory):
    """With ids all 0, two equal rays get equal colours (area_light is stochastic: the pixel id
    is the only source of randomness)."""
    hs, ds, seed, rays, img = _scene("area_light", tmp_path_factory)
    hit = np.flatnonzero(np.isfinite(img[:, 3]))
    pick = rays[hit[[hit.size // 2, hit.size // 2, hit.size // 3, hit.size // 3]]]
    got = ds.radiance(pick, seed=seed, pixel_ids=np.zeros(4, np.int32), camera_eye=True)
    other = ds.radiance(pick, seed=seed, pixel_ids=np.array([0, 1, 0, 1], np.int32), camera_eye=True)
    print("area_light equal rays", got[:, :3].tolist())
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and np.array_equal(_bits(got[2]), _bits(got[3]))
    assert np.array_equal(_bits(other[[0, 2]]), _bits(got[[0, 2]]))


# ---- 4. tmax
def test_tmax_bounds_primary_ray(tmp_path_factory):
    hs, ds, seed, rays, img = _scene("simple", tmp_path_factory)
    hit = np.flatnonzero(np.isfinite(img[:, 3]))
    assert 0 < hit.size < rays.size
    bg = qu.scene_arrays(hs)[0].astype(np.float32)
    half = rays[hit].copy()
    half["tmax"] = img[hit, 3] * np.float32(0.5)
    got = ds.radiance(half, seed=seed, pixel_ids=hit.astype(np.int32), camera_eye=True)
    print("simple hits", hit.size, "cut rays not background", int((got[:, :3] != bg[None, :]).any(axis=1).sum()))
    assert np.array_equal(_bits(got[:, :3]), _bits(np.broadcast_to(bg, (hit.size, 3))))
    assert np.array_equal(_bits(got[:, 3]), _bits(half["tmax"]))
    above = rays[hit].copy()
    above["tmax"] = np.nextafter(img[hit, 3], np.float32(np.inf))
    got = ds.radiance(above, seed=seed, pixel_ids=hit.astype(np.int32), camera_eye=True)
    assert np.array_equal(_bits(got), _bits(img[hit]))


# ---- 5. samples
@pytest.mark.parametrize("name", ["area_light", "pt_cornell"])
def test_sample_sum_order(name, tmp_path_factory):
    hs, ds, seed, rays, img = _scene(name, tmp_path_factory)
    c = [ds.radiance(rays, seed=seed, sample=s, camera_eye=True) for s in (2, 3, 4)]
    assert (_bits(c[0][:, :3]) != _bits(c[1][:, :3])).any()                  # stochastic: the samples differ
    want = (((np.float32(0) + c[0][:, :3]) + c[1][:, :3]) + c[2][:, :3]) / np.float32(3)
    assert want.dtype == np.float32
    got = ds.radiance(rays, seed=seed, sample=2, samples=3, camera_eye=True)
    diff = int((_bits(got[:, :3]) != _bits(want)).sum())
    print(name, "3-sample means: differing values", diff)
    assert diff == 0
    for k in range(3):
        assert np.array_equal(_bits(got[:, 3]), _bits(c[k][:, 3]))
    assert np.array_equal(_bits(c[0][:, 3]), _bits(img[:, 3]))


@pytest.mark.parametrize("name", ["area_light", "pt_cornell"])
def test_single_sample_is_render_pixels(name, tmp_path):
    """Sample s alone is RenderPixel's colour of sample s: a 4-spp copy rendered through
    RTG_RENDER_ACCUM_ONLY with sample_begin = s, sample_count = 1 accumulates float32(c) *
    float32(w), w (the sample's Gaussian weight) being the accumulation's fourth component."""
    torch = pytest.importorskip("torch")
    copy = tmp_path / (name + "_4spp.xml")
    copy.write_text(ob.with_samples(open(name + ".xml").read(), 4))
    hs = rtgpu.HostScene(str(copy))
    assert hs.camera(0)["spp"] == 4
    ds = rtgpu.DeviceScene(hs, 0)
    H, W = hs.camera(0)["height"], hs.camera(0)["width"]
    seed = 77
    for s in (0, 1, 3):
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        ds.render_device(0, 0, 0, accum_ptr=acc.data_ptr(), flags=FUSED | rtgpu.RTG_RENDER_ACCUM_ONLY, seed=seed,
                         sample_begin=s, sample_count=1)
        torch.cuda.synchronize()
        a = acc.cpu().numpy().reshape(-1, 4)
        c = ds.radiance(ds.camera_rays(sample=s, seed=seed), seed=seed, sample=s, camera_eye=True)
        want = c[:, :3] * a[:, 3:4]
        diff = int((_bits(a[:, :3]) != _bits(want)).sum())
        print(name, "sample", s, "differing values", diff, "weights", float(a[:, 3].min()), float(a[:, 3].max()))
        assert (a[:, 3] > 0).all()
        assert diff == 0, s


# ---- 6. plumbing
def test_torch_plumbing(tmp_path_factory):
    """radiance_device on torch tensors' pointers on the current stream gives the bytes of the
    host-buffer call, with and without device-resident ids."""
    import torch
    hs, ds, seed, rays, img = _scene("transforms_textures", tmp_path_factory)
    n = rays.size
    rng = np.random.default_rng(20260)
    perm = rng.permutation(n).astype(np.int32)
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        d_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        d_out = torch.full((n, 4), 7.0, dtype=torch.float32, device=dev)
        ds.camera_rays_device(d_rays.data_ptr(), seed=seed, stream=stream.cuda_stream)
        ds.radiance_device(d_rays.data_ptr(), n, d_out.data_ptr(), stream=stream.cuda_stream, seed=seed, camera_eye=True)
        d_perm = torch.from_numpy(perm).to(dev)
        d_prays = d_rays[d_perm.long()].contiguous()
        d_pout = torch.full((n, 4), 7.0, dtype=torch.float32, device=dev)
        ds.radiance_device(d_prays.data_ptr(), n, d_pout.data_ptr(), ids_ptr=d_perm.data_ptr(),
                           stream=stream.cuda_stream, seed=seed, camera_eye=True)
        stream.synchronize()
        assert d_out.cpu().numpy().tobytes() == img.tobytes()
        assert d_pout.cpu().numpy().tobytes() == img[perm].tobytes()


def test_render_unchanged_by_radiance(tmp_path_factory):
    """A render, 200 radiance calls and a second render give identical images."""
    hs, ds, seed, rays, img = _scene("transforms_textures", tmp_path_factory)
    hdr0, ldr0 = ds.render(0)
    part = rays[:2048]
    ids = np.arange(2048, dtype=np.int32)
    for k in range(200):
        got = ds.radiance(part, seed=seed, camera_eye=bool(k & 1), pixel_ids=ids if k & 2 else None,
                          samples=1 + (k % 3 == 0))
    assert np.array_equal(_bits(ds.radiance(part, seed=seed, camera_eye=True)), _bits(img[:2048]))
    hdr1, ldr1 = ds.render(0)
    assert hdr0.tobytes() == hdr1.tobytes() and ldr0.tobytes() == ldr1.tobytes()
    assert got is not None


def test_argument_errors_device(tmp_path_factory):
    L = rtgpu.lib()
    hs, ds, seed, rays, img = _scene("simple", tmp_path_factory)
    r4 = np.array(rays[:4])
    out = np.zeros((4, 4), np.float32)
    R, O = r4.ctypes.data, out.ctypes.data
    o = rtgpu.DeviceScene.radiance_opts()
    ok = ctypes.byref(o)
    assert ds.radiance(np.zeros(0, rtgpu.RAY_DTYPE)).shape == (0, 4)                       # n = 0
    assert L.rtg_radiance_rays(ds._s, ok, None, None, 0, None) == 0
    assert L.rtg_radiance_rays_device(ds._s, ok, None, None, 0, None, None) == 0
    assert L.rtg_radiance_rays(ds._s, None, R, None, 4, O) == -1
    assert L.rtg_radiance_rays(ds._s, ok, None, None, 4, O) == -1
    assert L.rtg_radiance_rays(ds._s, ok, R, None, 4, None) == -1
    assert L.rtg_radiance_rays(ds._s, ok, R, None, 1 << 31, O) == -1
    assert L.rtg_radiance_rays_device(ds._s, ok, None, None, 4, None, None) == -1
    assert L.rtg_radiance_rays(None, ok, R, None, 4, O) == -1
    for bad in (rtgpu.RadianceOpts(0, 0, 1, 2, seed, 0, 0), rtgpu.DeviceScene.radiance_opts(camera=99),
                rtgpu.DeviceScene.radiance_opts(camera=-1), rtgpu.DeviceScene.radiance_opts(first_pixel=-1)):
        assert L.rtg_radiance_rays(ds._s, ctypes.byref(bad), R, None, 4, O) == -1
        assert L.rtg_radiance_rays_device(ds._s, ctypes.byref(bad), R, None, 4, O, None) == -1
    ids = np.array([0, 1, -2, 3], np.int32)
    assert L.rtg_radiance_rays(ds._s, ok, R, ids.ctypes.data, 4, O) == -1 and b"pixel id" in L.rtg_last_error()
    assert not out.any()
    with pytest.raises(ValueError):
        ds.radiance(r4, pixel_ids=np.zeros(3, np.int32))
    # sample_begin < 0 is 0 and sample_count <= 0 is 1
    lo = rtgpu.RadianceOpts(0, -5, 0, rtgpu.RTG_RADIANCE_CAMERA_EYE, seed, 0, 0)
    assert L.rtg_radiance_rays(ds._s, ctypes.byref(lo), R, None, 4, O) == 0
    assert np.array_equal(_bits(out), _bits(img[:4]))
