"""The frame kernel's per-pixel set-up (k_shade<..., FRAME>: one camera ray per pixel, used by the walk
and by shading; the variant's feature bits in surface(); no motion-blur draw) on images that do not
fill their tiles, under each traversal variant of the kernel, and on every light kind of the fused
layouts.  Every case asserts that the render under test ran k_frame.

  awkward sizes   a 200-triangle height field at 37x21, 16x8 and 131x67 (partial 16x16 tiles, partial
                  8x8 waves, a height that is no multiple of 8), rendered whole, as a row band and as
                  three parts: the production render (k_frame), the two-kernel layout
                  (RTG_FRAME_KERNEL=0) and the fused kernel (RTG_RENDER_FUSED) agree bit for bit, and
                  with the CPU oracle by test_gpu_parity's criterion
  variants        the dof_motion fixture (aperture 0.4: the depth-of-field branch of the single ray; a
                  mesh, a moved mesh, two instances, a sphere) at 37x21 with its <MotionBlur> elements
                  removed -- a scene with motion blur never reaches the wavefront kernels -- as it is
                  (the instance variant of k_frame) and without its instances (the sphere variant);
                  `spheres` at 37x21 (sphere variant, two lights: the several-lights kernel)
  lights          point + area + directional light together (the several-lights frame kernel), and an
                  area and a directional light alone (the one-light frame kernel), at 37x21.  On the
                  height field, not on brdf_lights / area_light resized: brdf_lights has BRDF
                  materials and a spot light, so it takes the queued k_shade, and area_light at depth
                  0 has one light, which the "area" case here covers.  The stage is named k_frame
                  for the one-light and the several-lights kernel alike; a scene with three light
                  slots takes the latter (launch_wave_t: `one` needs at most one slot).
  normal          cornell_dielectric's shading normals (surface queries, as uint32) against the same
                  scene with one -0.0 entry in every object's inverse transpose and against the
                  host's own trace: the product with the identity is formed in full on all three
"""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import rtgpu
import scenes

pytestmark = pytest.mark.gpu

REL = 1e-4                  # test_gpu_parity's tolerance
SCENES = os.path.join(ob.GOLDEN, "scenes")
SIZES = [(37, 21), (16, 8), (131, 67)]
BAND = (5, 19)
LAYOUTS = ("frame", "two", "fused")

AREA = """        <AreaLight id="1">
            <Position>0.1 0.6 1.4</Position>
            <Normal>0 0 -1</Normal>
            <Radiance>900 850 800</Radiance>
            <Size>0.4</Size>
        </AreaLight>
"""
DIRECTIONAL = """        <DirectionalLight id="1">
            <Direction>-0.3 0.2 -1</Direction>
            <Radiance>40 40 45</Radiance>
        </DirectionalLight>
"""
LIGHTS = {"point_area_dir": ("keep", AREA + DIRECTIONAL), "area": ("drop", AREA), "dir": ("drop", DIRECTIONAL)}


def _bits(a):
    return a.view(np.uint32)


def _field(out_dir, w, h, lights=None):
    """(hs, ds) of the K = 200 height field at w x h; lights: a key of LIGHTS."""
    name = f"f{w}x{h}" + ("_" + lights if lights else "")
    xml = scenes.synthetic_heightfield(str(out_dir), K=200, width=w, height=h, name=name)
    if lights:
        point, extra = LIGHTS[lights]
        s = open(xml).read()
        if point == "drop":
            s, n = re.subn(r"\s*<PointLight id=\"1\">.*?</PointLight>", "", s, flags=re.S)
            assert n == 1
        s = s.replace("    </Lights>", extra + "    </Lights>", 1)
        with open(xml, "w") as f:
            f.write(s)
    old = os.getcwd()
    os.chdir(out_dir)           # the PLY's path is relative
    try:
        hs = rtgpu.HostScene(xml)
        return hs, rtgpu.DeviceScene(hs, 0)
    finally:
        os.chdir(old)


def _render(ds, layout, monkeypatch, **kw):
    if layout == "two":
        monkeypatch.setenv("RTG_FRAME_KERNEL", "0")
    try:
        return ds.render(0, flags=rtgpu.RTG_RENDER_FUSED if layout == "fused" else 0, **kw)
    finally:
        monkeypatch.delenv("RTG_FRAME_KERNEL", raising=False)


def _stages(ds, layout, monkeypatch):
    if layout == "two":
        monkeypatch.setenv("RTG_FRAME_KERNEL", "0")
    try:
        ds.render(0, flags=rtgpu.RTG_RENDER_TIMING | (rtgpu.RTG_RENDER_FUSED if layout == "fused" else 0))
        return list(ds.timings())
    finally:
        monkeypatch.delenv("RTG_FRAME_KERNEL", raising=False)


@pytest.mark.parametrize("w,h", SIZES)
def test_awkward_image_sizes(w, h, tmp_path, monkeypatch):
    hs, ds = _field(tmp_path, w, h)
    assert _stages(ds, "frame", monkeypatch) == ["k_frame"]
    assert _stages(ds, "two", monkeypatch) == ["k_primary", "k_shade_shadow"]
    assert _stages(ds, "fused", monkeypatch) == ["k_render"]
    ohdr, oldr, _ = ob.render(hs)
    whole = {}
    for layout in LAYOUTS:
        hdr, ldr = _render(ds, layout, monkeypatch)
        whole[layout] = hdr
        if layout != "frame":
            assert np.array_equal(_bits(hdr), _bits(whole["frame"])), (layout, "whole")
        assert np.array_equal(ldr, ob.clamp_ldr(hdr)), layout
        # a row band: its rows are the whole render's, nothing else is written
        if h >= BAND[1]:
            band, _ = _render(ds, layout, monkeypatch, rows=BAND)
            assert np.array_equal(_bits(band[BAND[0]:BAND[1]]), _bits(hdr[BAND[0]:BAND[1]])), (layout, "rows")
            assert not _bits(band[:BAND[0]]).any() and not _bits(band[BAND[1]:]).any(), (layout, "rows")
        # three parts into one pair of buffers
        out = (np.zeros_like(hdr), np.zeros_like(ldr))
        for r in range(3):
            _render(ds, layout, monkeypatch, part=(r, 3), out=out)
        assert np.array_equal(_bits(out[0]), _bits(hdr)) and np.array_equal(out[1], ldr), (layout, "parts")
    r = ob.compare(whole["frame"], ohdr, REL)
    print(w, h, r)
    assert r["n_fail"] == 0 and r["rel_pass"] == 1.0, r
    assert (whole["frame"] != 0).any(axis=2).all()       # every pixel was written


def _variant_xml(name, tmp_path):
    """A fixture at 37x21 that renders through k_frame under the named traversal variant."""
    src = {"instances": "dof_motion", "spheres_dof": "dof_motion", "spheres": "spheres"}[name]
    s = open(os.path.join(SCENES, src + ".xml")).read()
    if src == "dof_motion":
        s, n = re.subn(r"\s*<MotionBlur>[^<]*</MotionBlur>", "", s)
        assert n == 3
        if name == "spheres_dof":
            s, n = re.subn(r"\s*<MeshInstance .*?</MeshInstance>", "", s, flags=re.S)
            assert n == 2
    raw = tmp_path / (name + "_raw.xml")
    raw.write_text(s)
    return scenes.with_resolution(scenes.with_depth(str(raw), str(tmp_path / (name + "_d0.xml")), 0),
                                  str(tmp_path / (name + "_37x21.xml")), 37, 21)


@pytest.mark.parametrize("name", ["instances", "spheres_dof", "spheres"])
def test_traversal_variants_at_an_awkward_size(name, tmp_path, monkeypatch):
    xml = _variant_xml(name, tmp_path)
    old = os.getcwd()
    os.chdir(SCENES)            # PLY / image paths are relative
    try:
        hs = rtgpu.HostScene(xml)
        ds = rtgpu.DeviceScene(hs, 0)
        assert _stages(ds, "frame", monkeypatch) == ["k_frame"]
        assert _stages(ds, "two", monkeypatch) == ["k_primary", "k_shade_shadow"]
        kinds = set(qu.scene_arrays(hs)[1]["kind"].tolist())
        assert qu.RTG_OBJ_SPHERE in kinds and (qu.RTG_OBJ_INSTANCE in kinds) == (name == "instances")
        assert (qu.camera_record(hs)["aperture"] > 0.0001) == (name != "spheres")
        hdr, ldr = _render(ds, "frame", monkeypatch, seed=1234)
        for layout in ("two", "fused"):
            b, lb = _render(ds, layout, monkeypatch, seed=1234)
            assert np.array_equal(_bits(b), _bits(hdr)) and np.array_equal(lb, ldr), layout
        out = (np.zeros_like(hdr), np.zeros_like(ldr))
        for r in range(3):
            _render(ds, "frame", monkeypatch, seed=1234, part=(r, 3), out=out)
        assert np.array_equal(_bits(out[0]), _bits(hdr)) and np.array_equal(out[1], ldr)
        ds.reset_stats()
        chdr, _ = ds.render(0, seed=1234, flags=rtgpu.RTG_RENDER_COUNT_STATS)
        st = ds.stats()
        ohdr, _, ost = ob.render(hs, seed=1234)
    finally:
        os.chdir(old)
    r = ob.compare(hdr, ohdr, REL)
    print(name, r, st)
    assert hdr.shape == (21, 37, 3)
    assert r["n_fail"] == 0, r
    assert np.array_equal(_bits(chdr), _bits(hdr))
    # the scene exercises what the variant is for: sphere tests, and hits that cast shadow rays
    assert st["sphere_tests"] > 0 and st["shadow_rays"] > 100
    assert st["camera_rays"] == ost["camera_rays"] == 37 * 21


@pytest.mark.parametrize("lights", sorted(LIGHTS))
def test_every_shadow_casting_light_kind(lights, tmp_path, monkeypatch):
    hs, ds = _field(tmp_path, 37, 21, lights)
    assert _stages(ds, "frame", monkeypatch) == ["k_frame"]
    hdr, ldr = _render(ds, "frame", monkeypatch, seed=7)
    for layout in ("two", "fused"):
        b, lb = _render(ds, layout, monkeypatch, seed=7)
        assert np.array_equal(_bits(b), _bits(hdr)) and np.array_equal(lb, ldr), layout
    ohdr, _, ost = ob.render(hs, seed=7)
    r = ob.compare(hdr, ohdr, REL)
    print(lights, r, ost)
    assert r["n_fail"] == 0, r
    # the lights are in effect: every camera ray hits, and casts one shadow ray per light
    assert ost["shadow_rays"] == 37 * 21 * (3 if lights == "point_area_dir" else 1)


def test_shading_normal_with_a_negative_zero_in_the_inverse_transpose():
    """surface()'s last product, n * inverse transpose, on axis-aligned faces (normal components that
    are zeros of either sign).  With +1 / +0 entries each row is x + 0 y + 0 z + 0 * 0, whose last
    term is +0: a -0 off the diagonal changes no bit.  Both scenes take the full product; the host's
    trace forms the same one."""
    old = os.getcwd()
    os.chdir(SCENES)
    try:
        hs = rtgpu.HostScene("cornell_dielectric.xml")
        hz = rtgpu.HostScene("cornell_dielectric.xml")
    finally:
        os.chdir(old)
    d = qu.Desc.from_address(hz.desc)
    objs = np.frombuffer((ctypes.c_char * (d.num_objects * qu.OBJ_DTYPE.itemsize)).from_address(d.objects), qu.OBJ_DTYPE)
    meshes = np.flatnonzero(objs["kind"] != qu.RTG_OBJ_SPHERE)
    assert meshes.size > 0
    for k in meshes:
        assert objs["inv_transpose"][k][1] == 0.0
        objs["inv_transpose"][k][1] = -0.0          # row 0, column y (in place: the description's own memory)
    assert np.signbit(qu.scene_arrays(hz)[1]["inv_transpose"][meshes, 1]).all()
    assert not np.signbit(qu.scene_arrays(hs)[1]["inv_transpose"][meshes, 1]).any()
    ds, dz = rtgpu.DeviceScene(hs, 0), rtgpu.DeviceScene(hz, 0)
    rays = ds.camera_rays()
    s, z = ds.surface(rays), dz.surface(rays)
    hit = s["object"] >= 0
    on_mesh = hit & np.isin(s["object"], meshes)
    _, hn = hs.trace(rays, normals=True)
    _, hzn = hz.trace(rays, normals=True)
    n = s["n"][on_mesh]
    print("hits", int(hit.sum()), "on meshes", int(on_mesh.sum()), "normal components that are zero",
          int((n == 0).sum()), "of them -0", int(((n == 0) & np.signbit(n)).sum()))
    assert on_mesh.sum() > 1000 and (n == 0).sum() > 1000
    assert np.array_equal(s["object"], z["object"]) and np.array_equal(s["face"], z["face"])
    assert np.array_equal(_bits(np.ascontiguousarray(s["n"][hit])), _bits(np.ascontiguousarray(z["n"][hit])))
    assert np.array_equal(_bits(np.ascontiguousarray(s["n"][hit])), _bits(np.ascontiguousarray(hn[hit, :3])))
    assert np.array_equal(_bits(np.ascontiguousarray(z["n"][hit])), _bits(np.ascontiguousarray(hzn[hit, :3])))
