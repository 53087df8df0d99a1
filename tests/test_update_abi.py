"""The scene-update C-ABI boundary (include/rtgpu.h: rtg_scene_update, rtg_scene_set_camera,
rtg_scene_num_cameras, rtg_camera_setup, rtg_scene_clone, rtg_scene_shares_geometry), without a GPU:
the symbols exist and the ABI version stays 6, rtg_camera_view is the struct Python binds, null
arguments are codes, and rtg_camera_setup reproduces the loader's cameras bit for bit on every
fixture scene (the loader calls the same function; the inputs here come from the XML text)."""
import ctypes
import glob
import os
import shutil
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import rtgpu
import scene_variants as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NEW = ("rtg_scene_update", "rtg_scene_set_camera", "rtg_scene_num_cameras", "rtg_camera_setup", "rtg_scene_clone",
       "rtg_scene_shares_geometry")
OFFSETS = {"position": 0, "gaze": 12, "up": 24, "look_at": 36, "near_plane": 40, "fov_y": 56, "near_dist": 60,
           "width": 64, "height": 68}
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(sv.SCENES, "*.xml")))


def test_symbols_exist():
    L = rtgpu.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", rtgpu.LIB_PATH], capture_output=True, text=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in rtgpu.EXPORTED
        assert name in syms, name
        assert getattr(L, name).argtypes is not None, name
    assert L.rtg_abi_version() == 6
    for m in ("update", "set_camera", "num_cameras", "clone", "shares_geometry"):
        assert hasattr(rtgpu.DeviceScene, m), m
    assert callable(rtgpu.camera_setup)


def test_camera_view_layout(tmp_path):
    V = rtgpu.CameraView
    assert ctypes.sizeof(V) == 72
    assert {n: getattr(V, n).offset for n in OFFSETS} == OFFSETS
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        return      # the Python side above is the check the library's users rely on
    names = list(OFFSETS)
    src = tmp_path / "sz.c"
    src.write_text('#include "rtgpu.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){'
                   'printf("%zu %zu", sizeof(rtg_camera_view), sizeof(rtg_camera));\n'
                   + "".join('printf(" %%zu", offsetof(rtg_camera_view, %s));\n' % n for n in names)
                   + 'printf(" %zu %zu", offsetof(rtg_camera, width), offsetof(rtg_camera, spp));'
                   + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()))
    assert vals[:2] == [72, rtgpu.RTG_CAMERA_SIZE]
    assert dict(zip(names, vals[2:2 + len(names)])) == OFFSETS
    # Camera.view_bytes(): everything before spp; the size sits at its end
    assert vals[-2:] == [80, 88] and rtgpu._Camera.width.offset == 80 and rtgpu._Camera.spp.offset == 88


def test_null_arguments_are_codes():
    L = rtgpu.lib()
    cam = rtgpu.Camera()
    view = rtgpu.CameraView()
    C, n, h = ctypes.addressof(cam.buf), ctypes.c_int32(7), ctypes.c_void_p(5)
    calls = {
        "update: null scene": lambda: L.rtg_scene_update(None, None, None),
        "set_camera: null scene": lambda: L.rtg_scene_set_camera(None, 0, C),
        "num_cameras: null scene": lambda: L.rtg_scene_num_cameras(None, ctypes.byref(n)),
        "camera_setup: null view": lambda: L.rtg_camera_setup(None, C),
        "camera_setup: null camera": lambda: L.rtg_camera_setup(ctypes.byref(view), None),
        "clone: null scene": lambda: L.rtg_scene_clone(None, ctypes.byref(h)),
        "shares_geometry: null scenes": lambda: L.rtg_scene_shares_geometry(None, None, ctypes.byref(n)),
    }
    for label, call in calls.items():
        assert call() == INVALID, label
        assert b"null argument" in L.rtg_last_error(), (label, L.rtg_last_error())
    assert n.value == 7 and not any(cam.buf.raw)
    assert h.value == 5         # nothing is written before the arguments are checked
    hs = rtgpu.HostScene(os.path.join(sv.SCENES, "simple.xml"))
    assert L.rtg_scene_update(None, hs.desc, None) == INVALID


def _floats(el, n):
    """The first n numbers of an element's text as the loader's stream reads them (float32); zeros
    where the element is missing."""
    toks = el.text.split() if el is not None and el.text else []
    return [np.float32(t) for t in toks[:n]] + [np.float32(0)] * (n - len(toks[:n]))


@pytest.mark.parametrize("name", NAMES)
def test_camera_setup_reproduces_the_loader(name):
    with sv.in_scenes():
        hs = rtgpu.HostScene(name + ".xml", device_bvh=True)      # no BVH build: the cameras are all this reads
    cams = ET.parse(sv.golden(name)).getroot().find("Cameras").findall("Camera")
    assert len(cams) == hs.num_cameras() > 0
    for i, el in enumerate(cams):
        look_at = el.get("type") == "lookAt"
        w, h = (int(x) for x in _floats(el.find("ImageResolution"), 2))
        gaze = el.find("GazePoint") if look_at and el.find("GazePoint") is not None else el.find("Gaze")
        want = hs.camera_record(i)
        got = rtgpu.camera_setup(_floats(el.find("Position"), 3), _floats(gaze, 3), _floats(el.find("Up"), 3),
                                 _floats(el.find("NearDistance"), 1)[0], w, h,
                                 near_plane=None if look_at else _floats(el.find("NearPlane"), 4),
                                 fov_y=_floats(el.find("FovY"), 1)[0] if look_at else None, base=want)
        assert got.view_bytes() == want.view_bytes(), (name, i)
        assert got.buf.raw == want.buf.raw, (name, i)          # the other fields are left as they are
        # and from an empty camera: only the view's fields are written
        bare = rtgpu.camera_setup(_floats(el.find("Position"), 3), _floats(gaze, 3), _floats(el.find("Up"), 3),
                                  _floats(el.find("NearDistance"), 1)[0], w, h,
                                  near_plane=None if look_at else _floats(el.find("NearPlane"), 4),
                                  fov_y=_floats(el.find("FovY"), 1)[0] if look_at else None)
        assert bare.view_bytes() == want.view_bytes()
        assert bare.head.spp == 1 and not any(bare.buf.raw[92:])
