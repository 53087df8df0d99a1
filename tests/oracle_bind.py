"""Test-only binding of the CPU oracle (oracle/liboracle.so) and golden fixtures.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use this module;
the product (advanced-cpu-raytracing_amd/) never imports it.
"""
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_LIB = os.path.join(ROOT, "oracle", "liboracle.so")
REF_DRIVER = os.path.join(ROOT, "oracle", "_ref", "refdriver")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(ORACLE_LIB):
            raise RuntimeError(f"{ORACLE_LIB} not built: run `make -C {os.path.dirname(ORACLE_LIB)}`")
        L = ctypes.CDLL(ORACLE_LIB)
        vp = ctypes.c_void_p
        L.oracle_render.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_uint64, ctypes.c_int, vp, vp, vp, vp]
        L.oracle_render.restype = ctypes.c_int
        _lib = L
    return _lib


STAT_NAMES = ("camera_rays", "secondary_rays", "shadow_rays", "node_visits", "tri_tests", "sphere_tests",
              "object_tests", "shadow_node_visits", "shadow_tri_tests")


def render(host_scene, camera=0, rows=(0, 0), seed=0x5EED, threads=None, sample_begin=0, sample_count=-1,
           accum=False):
    """CPU restatement of RenderPixel over a parsed scene -> (hdr, ldr, stats) or (accum, stats)."""
    c = host_scene.camera(camera)
    h, w = c["height"], c["width"]
    threads = threads or min(16, os.cpu_count() or 1)
    st = np.zeros(9, np.uint64)
    if accum:
        acc = np.zeros((h, w, 4), np.float32)
        rc = lib().oracle_render(host_scene.desc, camera, rows[0], rows[1], sample_begin, sample_count, seed,
                                 threads, None, None, acc.ctypes.data, st.ctypes.data)
        if rc:
            raise RuntimeError("oracle_render failed")
        return acc, dict(zip(STAT_NAMES, map(int, st)))
    hdr = np.zeros((h, w, 3), np.float32)
    ldr = np.zeros((h, w, 3), np.uint8)
    rc = lib().oracle_render(host_scene.desc, camera, rows[0], rows[1], sample_begin, sample_count, seed, threads,
                             hdr.ctypes.data, ldr.ctypes.data, None, st.ctypes.data)
    if rc:
        raise RuntimeError("oracle_render failed")
    return hdr, ldr, dict(zip(STAT_NAMES, map(int, st)))


def render_pixel(host_scene, x, y, camera=0, seed=0x5EED, env_eps=0.0, env_flip=0):
    """One pixel as render() computes it -> (rgb float32[3], n_near).  With env_eps > 0 the
    distinct texel coordinates of environment lookups that lie within env_eps of a texel
    boundary are numbered ("near", n_near of them) and the lookups at those whose bit is set in
    env_flip take the texel on the other side: the effect of a last-ulp different atan2f /
    acosf on the device."""
    L = lib()
    L.oracle_render_pixel.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                      ctypes.c_float, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    rgb = np.zeros(3, np.float32)
    n = ctypes.c_int32()
    if L.oracle_render_pixel(host_scene.desc, camera, x, y, seed, env_eps, env_flip, rgb.ctypes.data,
                             ctypes.byref(n)):
        raise RuntimeError("oracle_render_pixel failed")
    return rgb, n.value


def radiance(host_scene, rays, pixel_ids=None, camera=0, sample=0, samples=1, seed=0x5EED, first_pixel=0,
             camera_eye=False, env_eps=0.0, env_flip=0, threads=None):
    """CPU restatement of a radiance query (oracle_radiance_rays), the arguments
    of rtgpu.DeviceScene.radiance -> ((n, 4) float32 rgb + primary t, n_near int32 per ray).
    rays: RAY_DTYPE-compatible 32-byte records.  env_eps / env_flip: as render_pixel."""
    L = lib()
    vp = ctypes.c_void_p
    L.oracle_radiance_rays.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                       ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64,
                                       ctypes.c_int, vp, vp]
    rays = np.ascontiguousarray(rays)
    assert rays.dtype.itemsize == 32 and rays.ndim == 1
    n = rays.size
    ids = None if pixel_ids is None else np.ascontiguousarray(pixel_ids, np.int32)
    assert ids is None or ids.size == n
    out = np.zeros((n, 4), np.float32)
    near = np.zeros(n, np.int32)
    threads = threads or min(16, os.cpu_count() or 1)
    if L.oracle_radiance_rays(host_scene.desc, camera, sample, samples, int(bool(camera_eye)), seed, first_pixel,
                              rays.ctypes.data, None if ids is None else ids.ctypes.data, n, env_eps, env_flip,
                              threads, out.ctypes.data, near.ctypes.data):
        raise RuntimeError("oracle_radiance_rays failed")
    return out, near


def explain_env_flips(host_scene, got, ref, rows=(0, 0), camera=0, seed=0x5EED, env_eps=2e-3, rel=1e-4):
    """Every pixel of `got` (GPU, rows [rows[0], ...) of the frame) outside the parity bound of
    `ref` (oracle), explained: some set of environment lookups within env_eps of a texel
    boundary, flipped to the neighbouring texel (render_pixel), reproduces the GPU's value within
    the bound.  Returns (failing pixels, unexplained [(y, x, n_near)])."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    ok = np.abs(got.astype(np.float64) - ref) <= rel * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    bad = np.argwhere(~ok.all(axis=-1))
    unexplained = []
    for yy, xx in bad:
        y = int(yy) + rows[0]
        g = got[yy, xx].astype(np.float64)
        base, n = render_pixel(host_scene, int(xx), y, camera, seed, env_eps, 0)
        assert np.array_equal(base, ref[yy, xx]), "render_pixel differs from render"
        found = False
        for mask in range(1, 1 << min(n, 8)):
            v, _ = render_pixel(host_scene, int(xx), y, camera, seed, env_eps, mask)
            if np.all(np.abs(g - v) <= rel * np.maximum(1.0, np.abs(v.astype(np.float64)))):
                found = True
                break
        if not found:
            unexplained.append((y, int(xx), n))
    return len(bad), unexplained


def tonemap(hdr, key=0.18, burn=1.0, saturation=1.0, gamma=2.2):
    """CPU restatement of Tonemapper::Tonemap (tonemapper.h:28-60)."""
    hdr = np.ascontiguousarray(hdr, np.float32)
    h, w, _ = hdr.shape
    out = np.zeros((h, w, 3), np.uint8)
    f = ctypes.c_float
    L = lib()
    L.oracle_tonemap.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, f, f, f, f, ctypes.c_void_p]
    if L.oracle_tonemap(hdr.ctypes.data, w, h, key, burn, saturation, gamma, out.ctypes.data):
        raise RuntimeError("oracle_tonemap failed")
    return out


def tonemap_goldens():
    """[(source name, params, reference LDR)] from tests/golden/tonemap.npz."""
    meta = json.load(open(os.path.join(GOLDEN, "tonemap.json")))
    d = np.load(os.path.join(GOLDEN, "tonemap.npz"), allow_pickle=False)
    return [(n, tuple(p), d[f"{n}__{k}"]) for n in meta["sources"] for k, p in enumerate(meta["params"])]


def clamp_ldr(hdr):
    """x86 (int) conversion + clamp to [0,255] (helperMath.cpp:140-152)."""
    x = np.asarray(hdr, np.float64)
    ok = (x > -2147483904.0) & (x < 2147483648.0)
    i = np.where(ok, np.trunc(np.where(ok, x, 0)), -2147483648.0)
    return np.clip(i, 0, 255).astype(np.uint8)


def load_golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["hdr"]


def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def compare(got, ref, rel=1e-4):
    """Parity figures: relative check |d| <= rel*max(1,|ref|), bit-exact and LDR-exact rates."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = rel * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    both_nan = np.isnan(got) & np.isnan(ref)
    ok = (d <= tol) | both_nan
    return {
        "rel_pass": float(np.mean(ok)),
        "bit_exact": float(np.mean((got.view(np.uint32) == ref.view(np.uint32)) | both_nan)),
        "ldr_exact": float(np.mean(clamp_ldr(got) == clamp_ldr(ref))),
        "max_abs": float(np.nanmax(np.where(both_nan, 0, d))) if d.size else 0.0,
        "n_fail": int(np.sum(~ok)),
    }


# ---------------------------------------------------------------------------
# Statistical goldens (kind "stochastic_avg": path tracing).  The reference golden is the
# per-pixel mean of n RenderPixel samples plus the variance of that mean (refdriver
# dumpavg).  Renders here use a camera with NumSamples = spp, whose Gaussian-weighted mean
# (main.cpp:60-101) has the variance of ~0.35*spp plain samples (the sigma = 1/6 px
# Gaussian over stratified positions), computed by gauss_eff_fraction().
# ---------------------------------------------------------------------------
def load_golden_avg(name):
    """Statistical golden: the reference's per-pixel mean of many RenderPixel samples and the
    variance of that mean -- <name>.npz for the path-tracing fixtures, <name>_avg.npz beside
    the 1-spp golden of the other stochastic fixtures."""
    p = os.path.join(GOLDEN, name + "_avg.npz")
    d = np.load(p if os.path.exists(p) else os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d["hdr"], d["var"]


def gauss_eff_fraction(spp):
    """Effective-sample fraction (sum w)^2 / (n sum w^2) of renderThreadMain's weights."""
    rng = np.random.default_rng(0)
    n = int(np.sqrt(spp))
    row, col = np.divmod(np.arange(n * n), n)
    fr = []
    for _ in range(64):
        sx = (col + rng.random(n * n)) / n - 0.5
        sy = (row + rng.random(n * n)) / n - 0.5
        w = np.exp(-0.5 * (sx * sx + sy * sy) * 36.0)
        fr.append(w.sum() ** 2 / (len(w) * (w * w).sum()))
    return float(np.mean(fr))


def with_samples(xml_text, spp):
    """The scene text with the camera's <NumSamples> set to spp."""
    import re
    xml_text = re.sub(r"\s*<NumSamples>[^<]*</NumSamples>", "", xml_text)
    return xml_text.replace("<ImageName>", f"<NumSamples>{spp}</NumSamples>\n            <ImageName>", 1)


def block_zscores(got, name, spp, block=8):
    """z-scores of 8x8-pixel block means of `got` (rendered at spp samples per pixel)
    against the reference's statistical golden `name`."""
    ref, var = load_golden_avg(name)
    m = manifest()[name]
    n_ref = m.get("samples", m.get("avg_samples"))
    h, w, _ = ref.shape
    h, w = h - h % block, w - w % block            # whole blocks only
    def blk(a):
        return np.asarray(a, np.float64)[:h, :w].reshape(h // block, block, w // block, block, 3).mean((1, 3))
    vref = np.asarray(var, np.float64)[:h, :w].reshape(h // block, block, w // block, block, 3).sum((1, 3)) / block ** 4
    vgot = vref * n_ref / (spp * gauss_eff_fraction(spp))
    # deterministic pixels (environment background, zero sample variance) differ by the
    # rounding of the weighted spp average: differences within north_star's 1e-4 relative
    # bound are not counted against the estimate
    tol = (1e-4 * np.maximum(1.0, np.abs(blk(ref)))) ** 2
    return (blk(got) - blk(ref)) / np.sqrt(vref + vgot + tol + 1e-12)


def zscore_ok(z):
    """Heavy-tailed estimators (GI rays that find the emitter): rms of |z| clipped at 10
    below 1.5 and at most 2% of blocks beyond 4 sigma."""
    a = np.minimum(np.abs(z), 10.0)
    return float(np.sqrt(np.mean(a * a))) < 1.5 and float(np.mean(a > 4.0)) <= 0.02, \
        {"rms": float(np.sqrt(np.mean(a * a))), "frac_gt4": float(np.mean(a > 4.0)), "max": float(np.abs(z).max())}


def load_native(name):
    """Native-resolution golden of a shipped scene (tests/golden/make_native.py): the
    reference's whole 8-bit frame, its float frame at a fixed pixel sample, per-row float sums
    and the float frame's SHA-256."""
    d = np.load(os.path.join(GOLDEN, "native", name + ".npz"), allow_pickle=False)
    return {k: d[k] for k in d.files}


def compare_native(hdr, ldr, gold, rel=1e-4):
    """GPU / oracle frame against a native golden: the share of equal 8-bit values, the
    parity bound at the sampled pixels, and the per-row sums within the bound summed over
    the row (|sum(got) - sum(ref)| <= rel * sum(max(1, |ref|)) <= rel * (3W + sum|ref|))."""
    idx = gold["sample_idx"]
    got = hdr.reshape(-1, 3)[idx]
    ref = gold["sample_hdr"]
    ok = np.abs(got.astype(np.float64) - ref) <= rel * np.maximum(1.0, np.abs(ref.astype(np.float64)))
    rows = hdr.astype(np.float64).sum(axis=(1, 2))
    w = hdr.shape[1]
    row_ok = np.abs(rows - gold["row_sums"]) <= rel * (3 * w + np.abs(hdr.astype(np.float64)).sum(axis=(1, 2)))
    return {"ldr_equal": float(np.mean(ldr == gold["ldr"])), "sample_pass": float(ok.all(axis=1).mean()),
            "sample_bit_exact": float((got.view(np.uint32) == ref.view(np.uint32)).all(axis=1).mean()),
            "rows_pass": float(row_ok.mean())}

