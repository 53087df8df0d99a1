"""Scene updates on the device (DeviceScene.update / set_camera / clone; rtg_scene_update,
rtg_scene_set_camera, rtg_scene_clone): a live scene moved to another description of the same
geometry answers bit for bit as a scene freshly created from that description.

  pairs        every pair of scene_variants.PAIRS, there and back: renders (hdr and ldr bytes) under
               flags 0, FUSED, EXACT_SHADOW and TREE, closest hits with normals, any-hit, surface and
               radiance on the new camera's rays, and the COUNT_STATS counters
  plans        ray-tree and path plans made before the update do not leak into renders after it
  lights       light counts change: the wavefront's one-light layouts and the general one, both ways
  cameras      set_camera against update, an appended camera, sizes that shrink and regrow, an orbit
               set up with camera_setup against scenes loaded from XML
  refusal      a refused update leaves the scene as it was
  stream       render, update, render on one stream see the old and the new scene in order
  replicas     a multi-replica scene is updated as a whole
  clone        shares the geometry, owns its state, outlives its source

What "equal" is compared against is always a fresh DeviceScene of the target description."""
import os

import numpy as np
import pytest

import rtgpu
import scene_variants as sv

pytestmark = pytest.mark.gpu

FUSED, TREE, EXACT, COUNT = (rtgpu.RTG_RENDER_FUSED, rtgpu.RTG_RENDER_TREE, rtgpu.RTG_RENDER_EXACT_SHADOW,
                             rtgpu.RTG_RENDER_COUNT_STATS)
FLAGS = (0, FUSED, EXACT, TREE)
INVALID, UNSUPPORTED = -1, -6

_fresh = {}


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    with sv.in_scenes():
        yield
    _fresh.clear()


@pytest.fixture(scope="module")
def xml(tmp_path_factory):
    """variant(name, edits, tag) -> path, written once per module run."""
    out = tmp_path_factory.mktemp("update_xml")
    return lambda name, edits, tag="b": sv.variant(name, out, edits, tag)


def snapshot(ds, flags=FLAGS, queries=True):
    """Everything the scene answers for camera 0, as bytes."""
    snap = {}
    for f in flags:
        hdr, ldr = ds.render(0, flags=f)
        snap["hdr", f], snap["ldr", f] = hdr.tobytes(), ldr.tobytes()
    if queries:
        rays = ds.camera_rays()
        hits, nrm = ds.trace(rays, normals=True)
        snap["rays"] = rays.tobytes()
        snap["closest"] = b"".join(hits[k].tobytes() for k in ("t", "object", "face"))
        snap["normals"] = nrm.tobytes()
        snap["any_hit"] = ds.trace(rays, any_hit=True)["object"].tobytes()
        snap["surface"] = ds.surface(rays).tobytes()
        snap["radiance"] = ds.radiance(rays, camera_eye=True).tobytes()
        ds.reset_stats()
        ds.render(0, flags=COUNT)
        snap["stats"] = ds.stats()
    return snap


def same(got, want, what):
    assert got.keys() == want.keys()
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, (what, diff)


def fresh(path, flags=FLAGS, queries=True):
    """(HostScene, snapshot of a freshly created scene), once per description and flag set."""
    key = (path, flags, queries)
    if key not in _fresh:
        hs = rtgpu.HostScene(path)
        ds = rtgpu.DeviceScene(hs, 0)
        _fresh[key] = (hs, snapshot(ds, flags, queries))
        ds.close()
    return _fresh[key]


# ---- 3. update equals fresh create
@pytest.mark.parametrize("name", sorted(sv.PAIRS))
def test_update_equals_fresh_create(name, xml):
    a, b = sv.golden(name), xml(name, sv.PAIRS[name])
    hs_a, snap_a = fresh(a)
    hs_b, snap_b = fresh(b)
    assert snap_a != snap_b, "the variant changes nothing"
    ds = rtgpu.DeviceScene(hs_a, 0)
    nodes, tris = ds.export_bvh()
    ds.update(hs_b)
    same(snapshot(ds), snap_b, name + ": a -> b")
    ds.update(hs_a)
    same(snapshot(ds), snap_a, name + ": b -> a")
    n2, t2 = ds.export_bvh()
    assert np.array_equal(nodes.view(np.uint32), n2.view(np.uint32)) and np.array_equal(tris.view(np.uint32), t2.view(np.uint32))
    # and started from B: what an update keeps of B's creation serves A
    ds2 = rtgpu.DeviceScene(hs_b, 0)
    ds2.update(hs_a)
    same(snapshot(ds2), snap_a, name + ": created as b, -> a")


# ---- 4. round trip and stale plans
ROUND_TRIPS = {
    "cornell_dielectric": ([("set", "MaxRecursionDepth", "1")], [("set", "MaxRecursionDepth", "4")]),
    "spheres_mirror": ([("set", "Materials/Material[@id='2']/MirrorReflectance", "0 0 0"),
                        ("set", "Materials/Material[@id='4']/MirrorReflectance", "0 0 0")],
                       [("set", "Materials/Material[@id='2']/MirrorReflectance", "0.7 0.7 0.7"),
                        ("set", "Materials/Material[@id='4']/MirrorReflectance", "0.7 0.7 0.7")]),
    # a path-tracing camera: the wavefront path tracer's plan
    "pt_nee": ([("set", "MaxRecursionDepth", "1")], [("set", "MaxRecursionDepth", "5"),
                                                      ("set", "Materials/Material[@id='5']/MirrorReflectance", "0.95 0.95 0.95")]),
}


@pytest.mark.parametrize("name", sorted(ROUND_TRIPS))
def test_round_trip_with_stale_plans(name, xml):
    ea, eb = ROUND_TRIPS[name]
    a, b = xml(name, ea, "rt_a"), xml(name, eb, "rt_b")
    hs_a, snap_a = fresh(a, (TREE, 0), False)
    hs_b, snap_b = fresh(b, (TREE, 0), False)
    assert snap_a["hdr", TREE] != snap_b["hdr", TREE]
    ds = rtgpu.DeviceScene(hs_a, 0)
    for _ in range(2):          # the second render runs on the plan the first one made
        same(snapshot(ds, (TREE,), False), {k: v for k, v in snap_a.items() if k[1] == TREE}, name + ": a")
    ds.update(hs_b)             # more secondary rays than A's plan has room for
    same(snapshot(ds, (TREE, 0), False), snap_b, name + ": a -> b")
    same(snapshot(ds, (TREE, 0), False), snap_b, name + ": b again")
    ds.update(hs_a)
    same(snapshot(ds, (TREE, 0), False), snap_a, name + ": b -> a")


# ---- 5. lights change count
def test_point_lights_one_two_one(xml):
    """synth_10k: the wavefront's one-light layout, the general one, and back."""
    one = sv.golden("synth_10k")
    two = xml("synth_10k", [("dup", "Lights/PointLight", [("Position", "-1.0 -0.8 1.5"), ("Intensity", "200 260 320")])], "two")
    hs1, snap1 = fresh(one)
    hs2, snap2 = fresh(two)
    ds = rtgpu.DeviceScene(hs1, 0)
    same(snapshot(ds), snap1, "as created")
    ds.update(hs2)
    same(snapshot(ds), snap2, "1 -> 2 lights")
    ds.update(hs1)
    same(snapshot(ds), snap1, "2 -> 1 lights")


def test_env_light_layouts(xml):
    """env_light: point + environment light (the three-payload layout) to two point lights (the
    general layout in buffers sized for the other), to the point light alone, and back."""
    for tag, depth in (("", []), ("flat_", [("set", "MaxRecursionDepth", "0")])):
        # at depth 0 the scene has no ray-tree children and renders on the wavefront pipeline
        a = xml("env_light", depth, tag + "a")
        two = xml("env_light", depth + [("remove", "Lights/SphericalDirectionalLight", None),
                                        ("dup", "Lights/PointLight", [("Position", "-3 4 2")])], tag + "two_points")
        lone = xml("env_light", depth + [("remove", "Lights/SphericalDirectionalLight", None)], tag + "lone")
        ds = rtgpu.DeviceScene(fresh(a)[0], 0)
        same(snapshot(ds), fresh(a)[1], "as created")
        for path in (two, lone, a, lone, two, a):
            ds.update(fresh(path)[0])
            same(snapshot(ds), fresh(path)[1], os.path.basename(path))


# ---- 6. cameras
CAM_B = [("set", "Cameras/Camera/Position", "2 3.5 9"), ("set", "Cameras/Camera/Gaze", "-0.2 -0.3 -1")]


def test_set_camera_equals_update(xml):
    a, b = sv.golden("transforms_textures"), xml("transforms_textures", CAM_B, "cam")
    hs_a, snap_a = fresh(a)
    hs_b, snap_b = fresh(b)
    assert snap_a["rays"] != snap_b["rays"]
    ds = rtgpu.DeviceScene(hs_a, 0)
    ds.set_camera(0, hs_b.camera_record(0))
    same(snapshot(ds), snap_b, "set_camera")
    ds2 = rtgpu.DeviceScene(hs_a, 0)
    ds2.update(hs_b)
    same(snapshot(ds2), snap_b, "update")
    # appended: camera 1 is B's, camera 0 still A's
    ds3 = rtgpu.DeviceScene(hs_a, 0)
    assert ds3.num_cameras() == 1
    ds3.set_camera(1, hs_b.camera_record(0))
    assert ds3.num_cameras() == 2
    hdr, ldr = ds3.render(1)
    assert hdr.tobytes() == snap_b["hdr", 0] and ldr.tobytes() == snap_b["ldr", 0]
    assert ds3.render(0)[0].tobytes() == snap_a["hdr", 0]
    with pytest.raises(rtgpu.RTGError) as e:
        ds3.set_camera(3, hs_b.camera_record(0))
    assert e.value.code == INVALID and ds3.num_cameras() == 2


def test_camera_sizes_shrink_and_regrow(xml):
    big = sv.golden("transforms_textures")
    small = xml("transforms_textures", [("set", "Cameras/Camera/ImageResolution", "96 64")], "small")
    hs_big, snap_big = fresh(big)
    hs_small, snap_small = fresh(small)
    assert hs_big.camera(0)["width"] == 200 and hs_small.camera(0)["width"] == 96
    ds = rtgpu.DeviceScene(hs_small, 0)      # buffers sized for the small image first
    same(snapshot(ds), snap_small, "as created")
    for hs, snap, what in ((hs_big, snap_big, "96x64 -> 200x150"), (hs_small, snap_small, "200x150 -> 96x64"),
                           (hs_big, snap_big, "-> 200x150 again")):
        ds.set_camera(0, hs.camera_record(0))
        same(snapshot(ds), snap, what)
    # a camera without pixels: queries take it, renders refuse it
    empty = hs_big.camera_record(0)
    empty.head.width = 0
    ds.set_camera(0, empty)
    hits = ds.trace(np.frombuffer(snap_big["rays"], rtgpu.RAY_DTYPE))
    assert b"".join(hits[k].tobytes() for k in ("t", "object", "face")) == snap_big["closest"]
    with pytest.raises(rtgpu.RTGError) as e:
        ds.render(0)
    assert e.value.code == INVALID


ORBIT = [("0 4 10", "0 -0.35 -1"), ("10 4 0", "-1 -0.35 0"), ("0 4 -10", "0 -0.35 1"), ("-10 4 0", "1 -0.35 0")]


def test_orbit_with_camera_setup(xml):
    """Four views set up with camera_setup from the numbers an XML would state equal four scenes
    loaded from four XMLs."""
    hs0 = fresh(sv.golden("transforms_textures"))[0]
    ds = rtgpu.DeviceScene(hs0, 0)
    f32 = lambda text: [np.float32(t) for t in text.split()]
    for k, (pos, gaze) in enumerate(ORBIT):
        path = xml("transforms_textures", [("set", "Cameras/Camera/Position", pos), ("set", "Cameras/Camera/Gaze", gaze)],
                   "orbit%d" % k)
        hs, snap = fresh(path, (0, TREE), True)
        cam = rtgpu.camera_setup(f32(pos), f32(gaze), f32("0 1 0"), np.float32("1.2"), 200, 150,
                                 near_plane=f32("-0.8 0.8 -0.6 0.6"), base=hs0.camera_record(0))
        assert cam.buf.raw == hs.camera_record(0).buf.raw
        ds.set_camera(0, cam)
        same(snapshot(ds, (0, TREE), True), snap, "view %d" % k)


# ---- 7. atomic refusal
def test_refused_update_changes_nothing(xml):
    hs_a, snap_a = fresh(sv.golden("transforms_textures"))
    ds = rtgpu.DeviceScene(hs_a, 0)
    other = rtgpu.HostScene("bump_normal.xml")
    needs_map = rtgpu.HostScene(xml(sv.NEEDS_MAP[0], sv.NEEDS_MAP[1], "needs_map"))
    for hs, code in ((other, INVALID), (needs_map, UNSUPPORTED), (other, INVALID)):
        with pytest.raises(rtgpu.RTGError) as e:
            ds.update(hs)
        assert e.value.code == code
        assert ds.host is hs_a and ds.num_cameras() == 1
        same(snapshot(ds), snap_a, "after a refusal (%d)" % code)
    ds.update(fresh(xml("transforms_textures", sv.PAIRS["transforms_textures"]))[0])     # and it still updates


# ---- 8. stream order
def test_stream_order(xml):
    torch = pytest.importorskip("torch")
    name = "transforms_textures"
    hs_a, snap_a = fresh(sv.golden(name))
    hs_b, snap_b = fresh(xml(name, sv.PAIRS[name]))
    ds = rtgpu.DeviceScene(hs_a, 0)
    c = hs_a.camera(0)
    bufs = [(torch.zeros((c["height"], c["width"], 3), dtype=torch.float32, device="cuda:0"),
             torch.zeros((c["height"], c["width"], 3), dtype=torch.uint8, device="cuda:0")) for _ in range(3)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = stream.cuda_stream
        ds.render_device(bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), st)
        ds.update(hs_b, stream=st)
        ds.render_device(bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), st)
        ds.update(hs_a, stream=st)
        ds.render_device(bufs[2][0].data_ptr(), bufs[2][1].data_ptr(), st)
    stream.synchronize()
    for (dh, dl), snap, what in zip(bufs, (snap_a, snap_b, snap_a), ("a", "b", "a again")):
        assert dh.cpu().numpy().tobytes() == snap["hdr", 0], what
        assert dl.cpu().numpy().tobytes() == snap["ldr", 0], what
    # the scene's own stream (host-buffer calls) follows the last update too
    same(snapshot(ds), snap_a, "host-buffer calls after the stream's updates")


# ---- 9. replicas
def test_replicas(xml):
    name = "transforms_textures"
    hs_a, snap_a = fresh(sv.golden(name))
    hs_b, snap_b = fresh(xml(name, sv.PAIRS[name]))
    ds = rtgpu.DeviceScene(hs_a, devices=[0, 0])
    hdr, ldr = ds.render(0)
    assert hdr.tobytes() == snap_a["hdr", 0]
    with pytest.raises(rtgpu.RTGError) as e:
        ds.update(hs_b, stream=12345)
    assert e.value.code == INVALID
    ds.update(hs_b)
    hdr, ldr = ds.render(0)
    assert hdr.tobytes() == snap_b["hdr", 0] and ldr.tobytes() == snap_b["ldr", 0]
    ds.set_camera(0, hs_a.camera_record(0))
    ds.update(hs_a)
    assert ds.render(0)[0].tobytes() == snap_a["hdr", 0]
    with pytest.raises(rtgpu.RTGError) as e:
        ds.clone()
    assert e.value.code == INVALID


# ---- 10. clone
@pytest.mark.parametrize("name", ["transforms_textures", "mesh_light", "env_light"])
def test_clone(name, xml):
    hs_a, snap_a = fresh(sv.golden(name))
    hs_b, snap_b = fresh(xml(name, sv.PAIRS[name]))
    src = rtgpu.DeviceScene(hs_a, 0)
    other = rtgpu.DeviceScene(hs_a, 0)
    clone = src.clone()
    assert src.shares_geometry(clone) and clone.shares_geometry(src) and src.shares_geometry(src)
    assert not src.shares_geometry(other)
    same(snapshot(clone), snap_a, "the clone as made")
    clone.update(hs_b)
    same(snapshot(clone), snap_b, "the clone updated")
    same(snapshot(src), snap_a, "the source beside it")
    for a, b in zip(src.export_bvh(), clone.export_bvh()):
        assert a.size > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    second = clone.clone()          # a clone of an updated clone starts from its state
    src.close()
    other.close()
    same(snapshot(clone), snap_b, "the clone after its source is gone")
    same(snapshot(second), snap_b, "a clone of the clone")
    second.update(hs_a)
    same(snapshot(second), snap_a, "... updated back")
    same(snapshot(clone), snap_b, "... beside the first clone")
