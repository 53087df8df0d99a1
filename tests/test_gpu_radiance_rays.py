"""Radiance queries on the device against the CPU oracle on off-camera rays (radiance_rays.py): probes
inside the scene and inside its bodies, directions that are not unit vectors, origins on surfaces,
back faces and grazing hits, a bounded primary ray on every kind of object, the motion-blur time as
given, misses whose pixel id is not the ray's index.  test_gpu_radiance.py compares the camera's own
rays with the render, which walks the same ray tree; here the yardstick is independent:

  reference (refdriver radiance) -> goldens -> oracle, bit for bit (test_radiance_rays_oracle.py)
  oracle -> device, within the project's parity bound 1e-4 (this file)

Deterministic scenes take their rays from the goldens; the stochastic ones generate theirs with the
same generator and compare under the same (seed, pixel id, sample) keys.  `motion_mirror` is
dof_motion with a mirror floor and a depth of 2, written at test time: the one scene in which rays
below the primary one meet moving objects, so that the time the tree inherits is visible.

Asserted: on every class and under both eyes, 0 colour values outside the bound against the oracle
(which must itself still equal the reference's goldens), and t bit-identical to HostScene.trace; on
the path-tracing, mesh-light and environment scenes at most 0.5 % of the rays outside it; class N's
t scaling exactly where the oracle's does; every wave mix, partial block and device-resident
submission bit-identical to one plain call.  DESIGN.md §2 lists which of these fail under which
one-line change to the device code."""
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import radiance_rays as rr
import rtgpu

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
REL = 1e-4                                   # the project's parity bound (oracle_bind.compare)
EXACT = ["area_light", "dof_motion", "defer_gate", "motion_mirror"]        # + - * / sqrt only below the primary ray
FLIPS = ["mesh_light", "env_light", "pt_cornell", "pt_nee", "pt_rr", "pt_meshlight"]   # device sinf / acosf / atan2f
FLIP_CAP = 0.005                             # of a scene's rays (path tracing)
ENV_EPS = 1e-3                               # see test_device_equals_oracle_stochastic
ENV_FILTER_CAP = 0.02
SEED = 0xBADC0DE

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)
    _cache.clear()


def _scene(name, tmp_path_factory):
    """(hs, ds, rays, ids, labels) once per module run; golden rays where the scene has a golden."""
    if name in _cache:
        return _cache[name]
    if name in ("defer_gate", "motion_mirror"):
        d = tmp_path_factory.mktemp(name)
        if name == "defer_gate":
            import scenes
            xml = scenes.config_defer_gate(str(d))
        else:
            xml = rr.write_motion_mirror(d)
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
    if name in rr.GOLDEN_SCENES:
        rays, ids, labels, _, _ = rr.load_golden(name)
    else:
        rays, ids, labels = rr.generate(hs)
    for a in (rays, ids, labels):
        a.setflags(write=False)
    _cache[name] = (hs, ds, rays, ids, labels)
    return _cache[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _failing_rays(got, want):
    """Rays with a colour component outside |d| <= REL * max(1, |ref|); equal bits and a NaN on both
    sides pass (oracle_bind.compare's rule, per ray)."""
    g, w = got[:, :3].astype(np.float64), want[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(g - w) <= REL * np.maximum(1.0, np.abs(w))) | rr.same_bits(got[:, :3], want[:, :3])
    return np.flatnonzero(~ok.all(1))


def _check_t(name, hs, rays, got, want):
    """The fourth float: the host walk's t bit for bit (tmax's own bits on a miss), and the oracle's."""
    host = hs.trace(rays)["t"]
    bad = np.flatnonzero(_bits(got[:, 3]) != _bits(host))
    assert bad.size == 0, (name, "t differs from HostScene.trace", rays[bad[:4]], got[bad[:4], 3], host[bad[:4]])
    assert np.array_equal(_bits(want[:, 3]), _bits(host)), (name, "oracle t differs from HostScene.trace")


# ---- 1. deterministic scenes: the goldens' rays, per class and eye
@pytest.mark.parametrize("name", rr.GOLDEN_SCENES)
def test_device_equals_oracle_on_golden_rays(name, tmp_path_factory):
    hs, ds, rays, ids, labels = _scene(name, tmp_path_factory)
    _, _, _, ref_bits, _ = rr.load_golden(name)
    for eye in (False, True):
        got = ds.radiance(rays, pixel_ids=ids, camera_eye=eye)
        want, _ = ob.radiance(hs, rays, ids, camera_eye=eye)
        assert rr.same_bits(want, ref_bits[eye]).all(), (name, "the oracle left the reference's goldens")
        _check_t(name, hs, rays, got, want)
        for cls, c in rr.CLASSES.items():
            sel = labels == c
            if not sel.any():
                continue
            r = ob.compare(got[sel, :3], want[sel, :3], REL)
            print(name, "camera eye" if eye else "origin eye", "class", cls, "rays", int(sel.sum()), "bit exact %.4f" % r["bit_exact"],
                  "max abs %.3g" % r["max_abs"], "n_fail", r["n_fail"])
            bad = np.flatnonzero(sel)[_failing_rays(got[sel], want[sel])]
            assert r["n_fail"] == 0 and bad.size == 0, (name, eye, cls, rays[bad[:4]], ids[bad[:4]], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("name", rr.GOLDEN_SCENES + ["motion_mirror"])
def test_direction_length(name, tmp_path_factory):
    """Class N: t(scaled) * scale == t(unit) on the device wherever the oracle says so, and nowhere
    else; the scaled rays' colours follow the oracle (the test above), which need not equal the unit
    ray's."""
    hs, ds, rays, ids, labels = _scene(name, tmp_path_factory)
    g = np.flatnonzero(labels == rr.CLASSES["N"]).reshape(-1, len(rr.N_SCALES))
    got = ds.radiance(rays[g.reshape(-1)], pixel_ids=ids[g.reshape(-1)]).reshape(g.shape + (4,))
    want = ob.radiance(hs, rays[g.reshape(-1)], ids[g.reshape(-1)])[0].reshape(g.shape + (4,))
    with np.errstate(invalid="ignore"):
        d_exact = got[:, :, 3] * rr.N_SCALES[None] == got[:, :1, 3]
        o_exact = want[:, :, 3] * rr.N_SCALES[None] == want[:, :1, 3]
    moved = (_bits(want[:, 1:, :3]) != _bits(want[:, :1, :3])).any(2)
    print(name, "N groups", g.shape[0], "t scales exactly (oracle)", o_exact.sum(0).tolist(), "colour differs from the unit ray's",
          moved.sum(0).tolist())
    assert np.array_equal(d_exact, o_exact)
    assert np.isfinite(want[:, 0, 3]).sum() > 5 and o_exact[:, 1:].any()


# ---- 2. stochastic scenes: generated rays under the oracle's own keys
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", EXACT + FLIPS)
def test_device_equals_oracle_stochastic(name, samples, tmp_path_factory):
    """samples = 1 under the origin eye, sample 0; samples = 3 under the camera's eye from sample 2."""
    hs, ds, rays, ids, labels = _scene(name, tmp_path_factory)
    eye, first = samples > 1, 0 if samples == 1 else 2
    got = ds.radiance(rays, pixel_ids=ids, camera_eye=eye, seed=SEED, sample=first, samples=samples)
    env = name == "env_light"
    want, near = ob.radiance(hs, rays, ids, camera_eye=eye, seed=SEED, sample=first, samples=samples,
                             env_eps=ENV_EPS if env else 0.0)
    _check_t(name, hs, rays, got, want)
    for cls, c in rr.CLASSES.items():
        assert (labels == c).any() or cls == "M" and not rr.has_motion_blur(hs), (name, cls)
    keep = np.ones(rays.size, bool)
    if qu.Desc.from_address(hs.desc).num_env_lights > 0:
        # a primary ray that misses looks the environment map up at acos(d.y) of the direction as given:
        # NaN for |d.y| > 1, where the reference reads outside its image -- no colour is defined
        # (INTEGRATION.md §6); the oracle's bounds check gives black there, the device row 0
        keep = ~((hs.trace(rays)["object"] < 0) & (np.abs(rays["dy"]) > 1))
        print(name, "primary misses with |d.y| > 1 (colour undefined)", int((~keep).sum()))
        assert (~keep).sum() < 0.05 * rays.size
    if env:
        # an environment lookup within ENV_EPS of a texel boundary may take the neighbouring texel
        # under a last-ulp different atan2f / acosf: those rays are not compared
        print(name, "rays near a texel boundary", int((near > 0).sum()), "of", rays.size)
        assert (near > 0).sum() < ENV_FILTER_CAP * rays.size
        keep &= near == 0
    bad = np.flatnonzero(keep)[_failing_rays(got[keep], want[keep])]
    r = ob.compare(got[keep, :3], want[keep, :3], REL)
    print(name, "samples", samples, "rays", int(keep.sum()), "bit exact %.4f" % r["bit_exact"], "max abs %.3g" % r["max_abs"],
          "n_fail", r["n_fail"], "failing rays", bad.size)
    for i in bad:
        print("  ", name, "ray", int(i), "class", rr.NAMES[int(labels[i])], "id", int(ids[i]), "device", got[i].tolist(),
              "oracle", want[i].tolist())
    hit = np.isfinite(got[:, 3])
    assert 0 < hit.sum() and len(np.unique(_bits(want[hit, :3]), axis=0)) > 50
    if name in EXACT:
        assert r["n_fail"] == 0 and bad.size == 0, (name, samples, rays[bad[:4]], got[bad[:4]], want[bad[:4]])
    else:
        assert bad.size <= FLIP_CAP * rays.size, (name, samples, bad.size)


# ---- 3. waves and plumbing: every submission equals the same rays shaded in one plain call
def _one_per_wave(off, n_off, n_cam, rng):
    """Waves of 63 consecutive camera rays and one off-camera ray: lane 0 in even waves, 63 in odd."""
    m = off.size
    out = n_off + (rng.integers(n_cam, size=m)[:, None] + np.arange(64)[None]) % n_cam
    out[np.arange(m), np.where(np.arange(m) % 2 == 0, 0, 63)] = off
    return out.reshape(-1)


def _half_waves(off, n_off, n_cam, rng):
    m = off.size
    out = np.empty(2 * m, np.int64)
    out[0::2] = off
    out[1::2] = n_off + (rng.integers(n_cam) + np.arange(m)) % n_cam
    return out


@pytest.mark.parametrize("name", ["cornell_dielectric", "transforms_textures", "area_light", "defer_gate"])
def test_waves_and_plumbing(name, tmp_path_factory):
    hs, ds, rays, ids, labels = _scene(name, tmp_path_factory)
    rng = np.random.default_rng(20271)
    cam = ds.camera_rays(seed=SEED)
    pick = rng.permutation(cam.size)[:4096]                       # a pool: the off-camera rays, then camera rays
    pool = np.concatenate([rays, cam[np.sort(pick)]])
    pool_ids = np.concatenate([ids, np.sort(pick).astype(np.int32)])
    n_off, n_cam = rays.size, pick.size
    plain = ds.radiance(pool, pixel_ids=pool_ids, seed=SEED)
    want, _ = ob.radiance(hs, pool, pool_ids, seed=SEED)
    if name != "defer_gate":                                      # (its oracle comparison is test 2's)
        assert _failing_rays(plain, want).size == 0
    off = rng.permutation(n_off)[:192]
    subs = [("1 lane per 64", _one_per_wave(off, n_off, n_cam, rng)), ("32 lanes per 64", _half_waves(off, n_off, n_cam, rng))]
    perm = rng.permutation(n_off)
    subs += [("n = %d" % n, perm[:n]) for n in (1, 63, 65, 257)]
    for label, idx in subs:
        got = ds.radiance(np.ascontiguousarray(pool[idx]), pixel_ids=pool_ids[idx], seed=SEED)
        bad = np.flatnonzero((_bits(got) != _bits(plain[idx])).any(1))
        assert bad.size == 0, (name, label, idx[bad[:8]].tolist(), got[bad[:4]], plain[idx][bad[:4]])
    import torch                                                  # only the device-resident submission needs it
    idx = subs[0][1]
    dev = torch.device("cuda:0")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream()
        d_rays = torch.from_numpy(np.ascontiguousarray(pool[idx]).view(np.float32).reshape(-1, 8)).to(dev)
        d_ids = torch.from_numpy(np.ascontiguousarray(pool_ids[idx])).to(dev)
        d_out = torch.full((idx.size, 4), 7.0, dtype=torch.float32, device=dev)
        ds.radiance_device(d_rays.data_ptr(), idx.size, d_out.data_ptr(), ids_ptr=d_ids.data_ptr(), stream=stream.cuda_stream,
                           seed=SEED)
        stream.synchronize()
        assert d_out.cpu().numpy().tobytes() == np.ascontiguousarray(plain[idx]).tobytes()
    print(name, "pool", pool.size, "submissions", len(subs) + 1, "all equal to the plain call")
