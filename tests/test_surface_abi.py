"""The surface queries' C-ABI boundary (rtg_surface_rays*, include/rtgpu.h) and the yardstick the
device test re-lights with (surface_rays.py).

1. The symbols exist, rtg_surface is the 64 bytes Python binds with the header's field offsets,
   argument errors are codes, and without a GPU the call is an error, never a fallback.  (n == 0 with
   a live scene, which needs a device to exist, is checked in test_gpu_surface.py.)
2. The re-lighting relation holds along the reference chain: on scenes without textures or maps the
   CPU oracle's colour of the relit scene equals kd * max(0, n . w) * I / |L - p|^2 with n from
   HostScene.trace(normals=True), kd from the material and occlusion from HostScene.trace(any_hit=True).
   No surface query is involved: this shows that test_gpu_surface.py's relation pins what it claims to."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu
import surface_rays as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
INVALID, HIP = -1, -4
OFFSETS = {"t": 0, "object": 4, "face": 8, "material": 12, "nx": 16, "ny": 20, "nz": 24, "u": 28, "gx": 32, "gy": 36,
           "gz": 40, "v": 44, "kd_r": 48, "kd_g": 52, "kd_b": 56, "pad": 60}


def test_symbols_exist():
    L = rtgpu.lib()
    for name in ("rtg_surface_rays", "rtg_surface_rays_device"):
        assert name in rtgpu.EXPORTED
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", rtgpu.LIB_PATH], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"rtg_surface_rays", "rtg_surface_rays_device"} <= syms
    assert L.rtg_abi_version() == 6
    assert hasattr(rtgpu.DeviceScene, "surface") and hasattr(rtgpu.DeviceScene, "surface_device")


def test_struct_layout(tmp_path):
    dt = rtgpu.SURFACE_DTYPE
    assert dt.itemsize == 64
    assert dt.names == ("t", "object", "face", "material", "n", "u", "ng", "v", "kd", "pad")
    py = {"t": "t", "object": "object", "face": "face", "material": "material", "nx": "n", "u": "u", "gx": "ng", "v": "v",
          "kd_r": "kd", "pad": "pad"}
    for c_name, field in py.items():
        assert dt.fields[field][1] == OFFSETS[c_name], field
    assert dt["n"].shape == dt["ng"].shape == dt["kd"].shape == (3,)
    assert dt["object"].base == dt["face"].base == dt["material"].base == np.dtype("<i4")
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        return      # the Python side above is the check the library's users rely on
    names = list(OFFSETS)
    src = tmp_path / "sz.c"
    src.write_text('#include "rtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu", sizeof(rtg_surface));\n'
                   + "".join('printf(" %%zu", offsetof(rtg_surface, %s));\n' % n for n in names) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    assert vals[0] == 64
    assert dict(zip(names, vals[1:])) == OFFSETS


def test_argument_errors_are_codes():
    """Every malformed call is RTG_ERR_INVALID with a message, for both entry points; with a null scene
    nothing is dereferenced and nothing is written."""
    L = rtgpu.lib()
    rays = np.zeros(4, rtgpu.RAY_DTYPE)
    out = np.zeros(4, rtgpu.SURFACE_DTYPE)
    R, O = rays.ctypes.data, out.ctypes.data
    cases = {
        "any hit": (R, 4, rtgpu.RTG_QUERY_ANY_HIT, O, b"ANY_HIT"),
        "any hit + coherent": (R, 4, rtgpu.RTG_QUERY_ANY_HIT | rtgpu.RTG_QUERY_COHERENT, O, b"ANY_HIT"),
        "unknown flag": (R, 4, 4, O, b"flags"),
        "unknown flag (high bit)": (R, 4, 0x80000002, O, b"flags"),
        "n = 2**31": (R, 1 << 31, 0, O, b"INT32_MAX"),
        "n < 0": (R, -1, 0, O, b"INT32_MAX"),
        "null rays": (None, 4, 0, O, b"null buffer"),
        "null output": (R, 4, 0, None, b"null buffer"),
        "null scene": (R, 4, 0, O, b"null scene"),
        "null scene, coherent": (R, 4, rtgpu.RTG_QUERY_COHERENT, O, b"null scene"),
        "null scene, n = 0": (R, 0, 0, O, b"null scene"),
    }
    for label, (r, n, flags, o, msg) in cases.items():
        assert L.rtg_surface_rays(None, r, n, flags, o) == INVALID, label
        assert msg in L.rtg_last_error(), (label, L.rtg_last_error())
        assert L.rtg_surface_rays_device(None, r, n, flags, o, None) == INVALID, label
        assert msg in L.rtg_last_error(), (label, L.rtg_last_error())
    assert not out.view(np.uint8).any()


@pytest.mark.skipif(rtgpu.device_count() > 0, reason="checks the no-GPU path")
def test_no_gpu_is_an_error_not_a_fallback():
    """As test_abi.py has it for rtg_render: the scene a surface call needs cannot be created without a
    device (RTG_ERR_HIP), so no surface value is ever computed on the host."""
    hs = rtgpu.HostScene(os.path.join(SCENES, "simple.xml"))
    with pytest.raises(rtgpu.RTGError) as e:
        rtgpu.DeviceScene(hs, 0).surface(np.zeros(1, rtgpu.RAY_DTYPE))
    assert e.value.code == HIP


def test_relit_rewrites_only_what_it_says():
    text = open(os.path.join(SCENES, "transforms_textures.xml")).read()
    lights = sr.light_setup([0, 4, 10], 9.0)
    out = sr.relit(text, lights)
    assert out.count("<PointLight") == 3 and "<AmbientLight>0 0 0</AmbientLight>" in out
    assert out.count("<SpecularReflectance>0 0 0</SpecularReflectance>") == text.count("<SpecularReflectance>")
    assert 'type="mirror"' not in out and out.count('type="image"') == text.count('type="image"')
    assert out.count('type="perlin"') == text.count('type="perlin"')
    strip = lambda s: s[:s.index("<Lights>")] + s[s.index("</Lights>"):]
    a, b = strip(text).splitlines(), strip(out).splitlines()
    changed = [(x, y) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and all("SpecularReflectance" in x or "<Material" in x for x, _ in changed)
    assert [tuple(p) for p, _ in lights] == [(0, 4, 10), (3, 5.5, 10), (-1.5, 7, 10)]
    assert [tuple(i) for _, i in lights] == [(81, 0, 0), (0, 81, 0), (0, 0, 81)]


@pytest.mark.parametrize("name", ["simple", "spheres", "two_spheres", "cornell_dielectric"])
def test_relighting_relation_holds_along_the_reference_chain(name, tmp_path):
    """The yardstick's own check (passes with and without the surface queries).  Measured on these
    scenes with pixel-centre camera rays: no disagreement about lit / not lit among about 270 000
    values, largest relative deviation of a lit value 2.3e-5 (two_spheres), 4e-6 typical, and one
    value in spheres 1.3 % off at n . w = 0.065; hence sr.REL = 1e-4 and sr.CAP = 0.1 %."""
    old = os.getcwd()
    os.chdir(SCENES)
    try:
        hs = rtgpu.HostScene(name + ".xml")
        assert not (qu.scene_arrays(hs)[1]["tex"] >= 0).any(), "a scene without textures or maps"
        rays = qu.numpy_camera_rays(qu.camera_record(hs))
        hits = hs.trace(rays)
        hit = hits["object"] >= 0
        eye = qu.origins(rays)[0]
        assert (qu.origins(rays) == eye).all()
        lights = sr.light_setup(eye, float(np.median(hits["t"][hit])))
        path = tmp_path / (name + "_relit.xml")
        path.write_text(sr.relit(open(name + ".xml").read(), lights))
        hr = rtgpu.HostScene(str(path))
        h2, nrm = hr.trace(rays, normals=True)
        assert np.array_equal(h2, hits)                    # the geometry did not move
        want, _ = ob.radiance(hr, rays)
    finally:
        os.chdir(old)
    kd = sr.material_diffuse(hr)[qu.scene_arrays(hr)[1]["material"][hits["object"][hit]]]
    pred = sr.predict(hr, rays[hit], hits["t"][hit], nrm[hit, :3], kd, lights)
    res = sr.compare_relit(want[hit, :3], pred)
    print(name, "hits", res["m"], "lit", res["lit"], "outside 1e-4", res["outside"], "lit / not lit disagree", res["disagree"],
          "max rel", ["%.3g" % x for x in res["max_rel"]])
    assert res["m"] > 1000 and min(res["lit"]) > 0
    assert sr.relit_ok(res), res
