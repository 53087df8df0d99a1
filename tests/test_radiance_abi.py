"""The radiance queries' C-ABI boundary (rtg_radiance_rays*, include/rtgpu.h): the symbols exist,
rtg_radiance_opts is the 32 bytes Python binds, argument errors are codes, and without a GPU the
call is an error, never a fallback.  (n == 0 with a live scene, which needs a device to exist, is
checked in test_gpu_radiance.py.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import rtgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
INVALID, HIP = -1, -4


def test_symbols_exist():
    L = rtgpu.lib()
    for name in ("rtg_radiance_rays", "rtg_radiance_rays_device"):
        assert name in rtgpu.EXPORTED
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    out = subprocess.run(["nm", "-D", "--defined-only", rtgpu.LIB_PATH], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert {"rtg_radiance_rays", "rtg_radiance_rays_device"} <= syms
    assert rtgpu.RTG_RADIANCE_CAMERA_EYE == 1
    assert L.rtg_abi_version() == 6
    assert hasattr(rtgpu.DeviceScene, "radiance") and hasattr(rtgpu.DeviceScene, "radiance_device")


def test_opts_layout(tmp_path):
    assert ctypes.sizeof(rtgpu.RadianceOpts) == 32
    assert rtgpu.RadianceOpts.seed.offset == 16 and rtgpu.RadianceOpts.first_pixel.offset == 24
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        return      # the Python side above is the check the library's users rely on
    src = tmp_path / "sz.c"
    src.write_text('#include "rtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(rtg_radiance_opts), offsetof(rtg_radiance_opts, flags), offsetof(rtg_radiance_opts, seed), '
                   'offsetof(rtg_radiance_opts, first_pixel), (int)RTG_RADIANCE_CAMERA_EYE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, flags, seed, first, eye = map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(rtgpu.RadianceOpts) == 32
    assert (flags, seed, first) == (rtgpu.RadianceOpts.flags.offset, rtgpu.RadianceOpts.seed.offset,
                                    rtgpu.RadianceOpts.first_pixel.offset)
    assert eye == rtgpu.RTG_RADIANCE_CAMERA_EYE


def test_argument_errors_are_codes():
    """With a null scene every malformed call is RTG_ERR_INVALID with a message, for both entry
    points; nothing is dereferenced."""
    L = rtgpu.lib()
    rays = np.zeros(4, rtgpu.RAY_DTYPE)
    out = np.zeros((4, 4), np.float32)
    ids = np.zeros(4, np.int32)
    R, O, I = rays.ctypes.data, out.ctypes.data, ids.ctypes.data
    ok = rtgpu.DeviceScene.radiance_opts()
    cases = {
        "null opts": (None, R, None, 4, O),
        "null rays": (ctypes.byref(ok), None, None, 4, O),
        "null output": (ctypes.byref(ok), R, None, 4, None),
        "n = 2**31": (ctypes.byref(ok), R, None, 1 << 31, O),
        "unknown flag": (ctypes.byref(rtgpu.RadianceOpts(0, 0, 1, 2, 0x5EED, 0, 0)), R, None, 4, O),
        "unknown flag (high bit)": (ctypes.byref(rtgpu.RadianceOpts(0, 0, 1, 0x80000001, 0x5EED, 0, 0)), R, None, 4, O),
        "camera 99": (ctypes.byref(rtgpu.DeviceScene.radiance_opts(camera=99)), R, None, 4, O),
        "negative first_pixel": (ctypes.byref(rtgpu.DeviceScene.radiance_opts(first_pixel=-1)), R, None, 4, O),
        "null scene": (ctypes.byref(ok), R, I, 4, O),
        "null scene, n = 0": (ctypes.byref(ok), R, None, 0, O),
    }
    for label, (o, r, i, n, c) in cases.items():
        assert L.rtg_radiance_rays(None, o, r, i, n, c) == INVALID, label
        assert L.rtg_last_error(), label
        assert L.rtg_radiance_rays_device(None, o, r, i, n, c, None) == INVALID, label
    # the messages name the argument at fault where the scene is not needed to see it
    assert L.rtg_radiance_rays(None, None, R, None, 4, O) == INVALID and b"null options" in L.rtg_last_error()
    assert L.rtg_radiance_rays(None, ctypes.byref(ok), R, None, 1 << 31, O) == INVALID and b"INT32_MAX" in L.rtg_last_error()
    bad = rtgpu.RadianceOpts(0, 0, 1, 6, 0x5EED, 0, 0)
    assert L.rtg_radiance_rays(None, ctypes.byref(bad), R, None, 4, O) == INVALID and b"flags" in L.rtg_last_error()
    neg = rtgpu.DeviceScene.radiance_opts(first_pixel=-7)
    assert L.rtg_radiance_rays(None, ctypes.byref(neg), R, None, 4, O) == INVALID and b"first_pixel" in L.rtg_last_error()
    assert not out.any()


@pytest.mark.skipif(rtgpu.device_count() > 0, reason="checks the no-GPU path")
def test_no_gpu_is_an_error_not_a_fallback():
    """As test_abi.py has it for rtg_render: the scene a radiance call needs cannot be created
    without a device (RTG_ERR_HIP), so no colour is ever computed on the host."""
    hs = rtgpu.HostScene(os.path.join(SCENES, "simple.xml"))
    with pytest.raises(rtgpu.RTGError) as e:
        rtgpu.DeviceScene(hs, 0).radiance(np.zeros(1, rtgpu.RAY_DTYPE))
    assert e.value.code == HIP
