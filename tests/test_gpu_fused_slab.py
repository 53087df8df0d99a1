"""The packet walks' fused slab distances (csrc/rtg_isect.hpp SlabFma: t = fma(m, inv, -fl(o inv)))
on the scenes where their new absolute error term, 2^-24 max|o inv|, matters most: a far origin,
near-axis camera rays, a grazing far light and an instanced mesh.  Small height fields (1 000
triangles) built here with scenes.heightfield_mesh / scenes.write_ply and an XML of the shape of
scenes.synthetic_heightfield's.

Each scene: the production render against the CPU oracle (no failing pixel, LDR byte for byte),
the counting render's node visits and triangle tests equal to the oracle's, and the production
render bit for bit what the reference shadow walk (RTG_RENDER_EXACT_SHADOW) gives.  A shadow ray
the any-hit walk leaves undecided takes the reference walk, which is exact whatever the fast path
did, so scenes 1-3 must also keep `shadow_fallbacks` within 5 % of their shadow rays.

`shadow_fallbacks` / shadow rays, measured on the parent commit first and then on this code
(the count depends on the exact decisions only, which the change does not alter):

    scene                         parent        result
    far origin (3000,-2000,1000)  0 / 9 216     0 / 9 216
    far origin (3000, 2000,1000)  0 / 9 216     0 / 9 216
    near axis 64x64               0 / 4 096     0 / 4 096
    near axis 65x65               0 / 4 225     0 / 4 225
    grazing far light             0 / 9 216     0 / 9 216
    transforms_textures, depth 0  0 / 17 694    0 / 17 694
"""
import os

import numpy as np
import pytest

import oracle_bind as ob
import rtgpu
import scenes

pytestmark = pytest.mark.gpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
CAM_POS = np.array([0.0, -1.2, 1.3])
CAM_LOOK = np.array([0.0, 0.9, -0.05])
LIGHT = np.array([1.6, -0.4, 1.1])


def _v(v):
    return " ".join(repr(float(x)) for x in v)


def _write_scene(out_dir, name, res, pos, gaze, up, light, extent, offset=(0.0, 0.0, 0.0), K=1000,
                 intensity=(420, 400, 380)):
    """A K-triangle height field over `extent`, one point light, default Blinn-Phong: the
    headline scene's XML; mesh, camera and light all translated by `offset`."""
    off = np.asarray(offset, np.float64)
    verts, faces = scenes.heightfield_mesh(K, extent)
    verts = (verts.astype(np.float64) + off).astype(np.float32)
    scenes.write_ply(os.path.join(out_dir, name + ".ply"), verts, faces)
    half_w = 0.45
    half_h = half_w * res[1] / res[0]
    xml = f"""<Scene>
    <MaxRecursionDepth>0</MaxRecursionDepth>
    <BackgroundColor>10 10 30</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>{_v(np.asarray(pos) + off)}</Position>
            <Gaze>{_v(gaze)}</Gaze>
            <Up>{_v(up)}</Up>
            <NearPlane>{_v((-half_w, half_w, -half_h, half_h))}</NearPlane>
            <NearDistance>0.6</NearDistance>
            <ImageResolution>{res[0]} {res[1]}</ImageResolution>
            <ImageName>{name}.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>20 20 20</AmbientLight>
        <PointLight id="1">
            <Position>{_v(np.asarray(light) + off)}</Position>
            <Intensity>{_v(intensity)}</Intensity>
        </PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>0.75 0.6 0.45</DiffuseReflectance>
            <SpecularReflectance>0.35 0.35 0.35</SpecularReflectance>
            <PhongExponent>20</PhongExponent>
        </Material>
    </Materials>
    <VertexData>0 0 0</VertexData>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces plyFile="{name}.ply"/>
        </Mesh>
    </Objects>
</Scene>
"""
    path = os.path.join(out_dir, name + ".xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def _footprint(pos, gaze, up, res, zmin=-0.125, margin=0.08):
    """The frustum's footprint on the lowest possible surface plus a margin, as
    scenes.synthetic_heightfield computes it: every camera ray hits the field."""
    right = np.cross(up, -gaze)
    right /= np.linalg.norm(right)
    upo = np.cross(-gaze, right)
    half_w = 0.45
    half_h = half_w * res[1] / res[0]
    pts = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            d = gaze * 0.6 + right * sx * half_w + upo * sy * half_h
            pts.append(pos + (zmin - pos[2]) / d[2] * d)
    pts = np.array(pts)
    mx = margin * (pts[:, 0].max() - pts[:, 0].min())
    my = margin * (pts[:, 1].max() - pts[:, 1].min())
    return (pts[:, 0].min() - mx, pts[:, 0].max() + mx, pts[:, 1].min() - my, pts[:, 1].max() + my)


def _oblique(out_dir, name, res=(128, 72), light=LIGHT, offset=(0.0, 0.0, 0.0), intensity=(420, 400, 380)):
    """The headline camera (scenes.synthetic_heightfield) over a field that fills its frame."""
    gaze = CAM_LOOK - CAM_POS
    gaze /= np.linalg.norm(gaze)
    up = np.array([0.0, 0.0, 1.0])
    return _write_scene(out_dir, name, res, CAM_POS, gaze, up, light, _footprint(CAM_POS, gaze, up, res), offset,
                        intensity=intensity)


def _near_axis(out_dir, name, n):
    """The camera above the field looking almost straight down: the central rays' x / y direction
    components are 1e-7 ... 1e-6 (a huge max|o inv|: never sure) or exactly zero (off the fast
    path), in the same waves as ordinary lanes."""
    gaze = np.array([1e-7, 1e-6, -1.0])
    gaze /= np.linalg.norm(gaze)
    return _write_scene(out_dir, name, (n, n), (0.05, -0.03, 1.5), gaze, (0.0, 1.0, 0.0), LIGHT, (-1.4, 1.4, -1.4, 1.4))


def _check(xml, cwd, fallback_cap=True, nodes=None):
    old = os.getcwd()
    os.chdir(cwd)
    try:
        hs = rtgpu.HostScene(xml)
        assert nodes is None or hs.counts()["nodes"] == nodes, hs.counts()
        ds = rtgpu.DeviceScene(hs, 0)
        hdr, ldr = ds.render(0)
        ehdr, eldr = ds.render(0, flags=rtgpu.RTG_RENDER_EXACT_SHADOW)
        ds.reset_stats()
        chdr, cldr = ds.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS)
        st = ds.stats()
        ohdr, oldr, ost = ob.render(hs)
    finally:
        os.chdir(old)
    r = ob.compare(hdr, ohdr)
    print(os.path.basename(xml), r, {k: st[k] for k in ("camera_rays", "shadow_rays", "node_visits", "tri_tests",
                                                         "shadow_wide_visits", "shadow_fallbacks")})
    assert r["n_fail"] == 0, r
    assert np.array_equal(ldr, oldr)
    for k in ("camera_rays", "shadow_rays", "node_visits", "tri_tests"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert np.array_equal(chdr.view(np.uint32), hdr.view(np.uint32)) and np.array_equal(cldr, ldr)
    assert np.array_equal(ehdr.view(np.uint32), hdr.view(np.uint32)) and np.array_equal(eldr, ldr)
    if fallback_cap:
        assert st["shadow_rays"] > 0
        assert st["shadow_fallbacks"] <= 0.05 * st["shadow_rays"], (st["shadow_fallbacks"], st["shadow_rays"])
    return st


@pytest.mark.parametrize("offset", [(3000.0, -2000.0, 1000.0), (3000.0, 2000.0, 1000.0)])
def test_far_origin(tmp_path, offset):
    """Mesh, camera and light translated by (3000, -2000, 1000): max|o inv| is 10^3 - 10^4 times a
    typical t, so the absolute slack term dominates every decision.  With every y negative the
    reference's BVH build leaves that mesh one 968-face leaf (its root box starts at FLT_MIN, so
    the first split puts every face on one side): the shadow rays take the packet walk of the
    any-hit tree, the camera rays the large-leaf walk.  The second offset, all positive, gives the
    ordinary tree, and the camera rays take their packet walk too."""
    _check(_oblique(str(tmp_path), "far", offset=offset), tmp_path, nodes=1 if offset[1] < 0 else 1935)


@pytest.mark.parametrize("n", [64, 65])
def test_near_axis_camera(tmp_path, n):
    _check(_near_axis(str(tmp_path), f"axis{n}", n), tmp_path)


def test_grazing_far_light(tmp_path):
    """A point light at (1e4, 0, 0.2): shadow rays nearly parallel to the x axis, limits near 1e4."""
    # (the intensity scaled with the squared distance, so the light's term is visible in the image)
    _check(_oblique(str(tmp_path), "graze", light=(1e4, 0.0, 0.2), intensity=(1.05e10, 1.0e10, 0.95e10)), tmp_path)


def test_instanced_mesh(tmp_path):
    """transforms_textures (MeshInstances with rotations, scalings and translations) at its golden
    size: every instance-local ray recomputes -fl(o inv) and max|o inv|.  The scene against its
    golden, and its depth-0 copy -- the wavefront pipeline, whose camera and shadow rays take the
    packet walks -- under the three assertions above."""
    old = os.getcwd()
    os.chdir(SCENES)
    try:
        hs = rtgpu.HostScene(os.path.join(SCENES, "transforms_textures.xml"))
        hdr, ldr = rtgpu.DeviceScene(hs, 0).render(0)
    finally:
        os.chdir(old)
    r = ob.compare(hdr, ob.load_golden("transforms_textures"))
    assert r["rel_pass"] == 1.0, r
    assert np.array_equal(ldr, ob.clamp_ldr(hdr))
    xml = scenes.with_depth(os.path.join(SCENES, "transforms_textures.xml"), str(tmp_path / "tt_d0.xml"), 0)
    _check(xml, SCENES, fallback_cap=False)
