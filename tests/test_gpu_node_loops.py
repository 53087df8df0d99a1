"""The node loops of the two packet walks (walk_bvh_packet_lx: the camera rays' pre-order walk;
walk_wide_any_pk: the shadow rays' wide-node walk) at the smallest shapes where a restructured loop
can go wrong, at 16x8 and 37x21 (partial 8x8 waves: lanes past the image edge in both; 37 and 21 are
odd and the camera looks down -z with a symmetric near plane, so the middle column and row of the
larger frame are axis-aligned rays: a zero direction component, the lanes whose conservative value
is NaN and for which the camera loop takes its exact branch at every inner node -- asserted below
for every case but the five of OBLIQUE, whose cameras look elsewhere or from 1e38).

Every case renders through the production layout (k_frame; asserted, as test_gpu_frame_setup.py
does) and through the two-kernel layout (RTG_FRAME_KERNEL=0) and asserts
  * both images and the counting render's image equal bit for bit, and equal to the CPU oracle's bit
    for bit (the cases' material is matte, SpecularReflectance 0: no transcendental call whose last
    ulp could differ reaches the pixel),
  * the counting render's camera_rays, shadow_rays, node_visits and tri_tests equal to the oracle's.
Scenes with a leaf above kBigLeaf = 8 (copies_256, copies_300: LEAF_EXT leaves; huge_empty: a leaf of
12) cannot take k_frame (FEAT_BIGLEAF): their first stage is k_primary, which runs the same camera
loop; that is asserted instead.

Camera loop (walk_bvh_packet_lx)
  spread_1 / 2 / 3       one face (the root is a leaf: the loop ends from a leaf step), two, three
  last_pass / last_skip  a row of 37 faces along x; the last pre-order node is the rightmost leaf, the
                         face at the far end.  last_pass: the last seven faces in view, that leaf's
                         face is hit and so are others, rays descend its siblings.  last_skip: a
                         narrow view of that face from above: every hit lies in it and the
                         reference's walk visits exactly the path's 2 D + 1 nodes per ray (the root,
                         and per level the left sibling, which fails, and the right child), so every
                         lane fails every left sibling and the wave arrives by skip links alone
  copies_256 / 300       LEAF_EXT leaves
  chain                  92 levels, seen from the origin along +x, where a ray passes the boxes of
                         every level (184 node visits per ray)
  huge_empty, huge_split, subnormal   boxes that overflow and boxes of subnormals

Shadow loop (walk_wide_any_pk).  tests/wide_slots_main.cpp (host only, built here) lists each scene's
wide nodes by slot pattern; over the scenes below the test asserts nodes with one, two, three and
four children, a leaf and an inner child in every slot 0..3 and an empty slot in 1..3 (the tree
builder fills a node's slots from the front: no node of any case has an empty slot 0, or an empty
slot before a used one), and a node with four inner children below depth 4 (several pushes in one
step, popped later).
  spread_255, spread_513, tie_split   each over a floor that fills the view, so that every floor pixel
                         casts a shadow ray up through the mesh's any-hit tree
  (the slot patterns are counted over these, chain -- 17 levels of wide nodes -- and spread_1)
  light_inside           spread_255 over its floor with the light at the middle of the mesh box
  roof                   a floor under a larger roof, camera between them, light above the roof:
                         every shadow ray is occluded (host any-hit query), at the only leaf node
  open                   the floor alone, light above: no shadow ray is occluded
  pinwheel_8192 / 49152  over a floor (walk_cases.load_pinwheel_floor): shadow_fallbacks 0, and
                         positive with the step bound exceeded, as test_gpu_walk_cases.py expects

Mutated libraries (scratch builds, one decision each, memory-safe), run against this file on an
MI355X (profiles/r16_node_loops_ab.txt has the runs' summaries):
  (a) the camera loop always takes `skip` after an inner node, also where a lane passes: 21 of the
      38 cases fail on the image -- spread_2 and spread_3 at 37x21, last_pass, last_skip, subnormal,
      spread_255, spread_513, tie_split, light_inside, open, pinwheel_49152 at both sizes,
      pinwheel_8192 at 37x21.  spread_1, the copies, roof and the huge cases (a root leaf, or nothing
      in view) pass, and so does chain, where no ray hits a face in either walk.
  (b) the shadow loop drops the last child it pushed in a step: 11 of the 38 cases fail (pixels lit that the
      oracle has in shadow) -- spread_255, spread_513, tie_split, light_inside, pinwheel_49152 at both
      sizes, pinwheel_8192 at 37x21.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bvh_cases as bc
import edge_rays as er
import oracle_bind as ob
import query_util as qu
import rtgpu
import walk_cases as wc

SIZES = [(16, 8), (37, 21)]
COUNTERS = ("camera_rays", "shadow_rays", "node_visits", "tri_tests")
CSRC = os.path.join(ob.ROOT, "advanced-cpu-raytracing_amd", "csrc")
HELPER = [os.path.join(ob.ROOT, "tests", "wide_slots_main.cpp")] + [
    os.path.join(CSRC, f) for f in ("host_xml.cpp", "host_scene.cpp", "host_assets.cpp", "scene_tables.cpp", "rtg_ahb.cpp")]
f32 = np.float32


def _floor(h=1.0, z=0.0):
    return (np.array([(-h, -h, z), (h, -h, z), (h, h, z), (-h, h, z)], f32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def _roof():
    v, f = _floor()
    return np.concatenate([v, np.array([(-8, -8, 1), (8, -8, 1), (0, 12, 1)], f32)]), np.concatenate([f, [[4, 5, 6]]])


CAMERA = ["spread_1", "spread_2", "spread_3", "last_pass", "last_skip", "copies_256", "copies_300", "chain", "huge_empty",
          "huge_split", "subnormal"]
SHADOW = ["spread_255", "spread_513", "tie_split", "light_inside", "roof", "open", "pinwheel_8192", "pinwheel_49152"]
OVER_A_FLOOR = {"spread_255": "spread_255", "spread_513": "spread_513", "tie_split": "tie_split", "light_inside": "spread_255"}
# the cases whose camera does not look down -z from a finite position (no axis-aligned ray is claimed there)
OBLIQUE = ("chain", "huge_empty", "huge_split", "pinwheel_8192", "pinwheel_49152")
PATTERN_SCENES = ["spread_1", "spread_255", "spread_513", "tie_split", "chain"]


def _row(n=37, seed=5):
    """n faces of about 0.3 along x, one per unit: the BVH splits on x alone, the rightmost leaf is the
    face at the far end, and from above it every left sibling's box lies to one side."""
    rng = np.random.default_rng(seed)
    c = np.stack([np.arange(n) * 1.0, rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n)], 1)
    return bc._soup(c, rng.uniform(-0.3, 0.3, (n, 3, 3)))


def _case(name):
    if name == "roof":
        return bc.Case([_roof()])
    if name == "open":
        return bc.Case([_floor()])
    if name in ("last_pass", "last_skip"):
        return bc.Case([_row()])
    if name in OVER_A_FLOOR:
        # the mesh over a floor that fills the view: every pixel between the faces casts a shadow ray up
        # through the mesh's any-hit tree
        v, f = wc.get(OVER_A_FLOOR[name]).meshes[0]
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        ext = (hi - lo).max()
        c, r = (lo + hi) / 2, 1.25 * ext
        fv = np.array([(c[0] - r, c[1] - r, lo[2] - 1), (c[0] + r, c[1] - r, lo[2] - 1),
                       (c[0] + r, c[1] + r, lo[2] - 1), (c[0] - r, c[1] + r, lo[2] - 1)], f32)
        return bc.Case([(v, f), (fv, np.array([[0, 1, 2], [0, 2, 3]], np.int32))])
    return wc.get(name)


def _load(directory, xml):
    old = os.getcwd()
    os.chdir(str(directory))
    try:
        return rtgpu.HostScene(os.path.basename(xml))
    finally:
        os.chdir(old)


def _edit(xml, w, h, light=None, eye=None, gaze=None, near=None):
    s = open(xml).read()
    subs = [(r"<ImageResolution>[^<]*</ImageResolution>", "<ImageResolution>%d %d</ImageResolution>" % (w, h))]
    if light is not None:
        subs.append((r"<PointLight id=\"1\"><Position>[^<]*</Position>",
                     '<PointLight id="1"><Position>%s</Position>' % bc._g(light)))
    if eye is not None:
        subs.append((r"<Position>[^<]*</Position>\s*<Gaze>[^<]*</Gaze>",
                     "<Position>%s</Position><Gaze>%s</Gaze>" % (bc._g(eye), bc._g(gaze))))
    if near is not None:
        subs.append((r"<NearPlane>[^<]*</NearPlane>\s*<NearDistance>[^<]*</NearDistance>",
                     "<NearPlane>%s</NearPlane><NearDistance>%s</NearDistance>" % (bc._g(near[:4]), bc._g(near[4:]))))
    for pat, val in subs:
        s, k = re.subn(pat, val, s, count=1)
        assert k == 1, pat
    with open(xml, "w") as f:
        f.write(s)


def _last_leaf(hs):
    """(first face, count, depth) of the rightmost leaf of the single mesh's BVH: the last node in
    pre-order (a node's children are left and left + 1)."""
    nd = er.node_array(hs)
    k, depth = 0, 0
    while nd[k]["left"] >= 0:
        k, depth = int(nd[k]["left"]) + 1, depth + 1
    return int(nd[k]["first"]), int(nd[k]["count"]), depth


def prepare(directory, name, w, h):
    """The case's HostScene at w x h, and what the host can say of its premises."""
    tag = "%s_%dx%d" % (name, w, h)
    info = {}
    if name.startswith("pinwheel_"):
        hs = wc.load_pinwheel_floor(directory, name)
        xml = os.path.join(str(directory), name + "_floor.xml")
        _edit(xml, w, h)
        return _load(directory, xml), info, xml
    xml = bc.write_scene(_case(name), str(directory), tag)
    _edit(xml, w, h)
    if name in OVER_A_FLOOR:
        # camera and light as bvh_cases.write_scene places them for the mesh alone (the floor's extent
        # would move both away); light_inside: the light at the middle of the mesh box
        v = _case(name).meshes[0][0].astype(np.float64)
        c, ext = (v.min(0) + v.max(0)) / 2, (v.max(0) - v.min(0)).max()
        _edit(xml, w, h, light=c if name == "light_inside" else c + np.array([ext, ext, 3 * ext]),
              eye=c + np.array([0, 0, 1.5 * ext]), gaze=(0, 0, -1))
    elif name == "chain":
        # from the origin along +x: the faces at x = 2^k are nested in the view, and a ray passes the
        # boxes of all 92 levels
        _edit(xml, w, h, eye=(0, 0, 0), gaze=(1, 0.03, 0.06), near=(-0.2, 0.2, -0.15, 0.15, 1))
    elif name == "roof":
        _edit(xml, w, h, light=(0.2, 0.1, 3.0), eye=(0.0, 0.0, 0.5), gaze=(0, 0, -1), near=(-1, 1, -0.75, 0.75, 0.5))
    elif name == "open":
        _edit(xml, w, h, light=(0.2, 0.1, 3.0), eye=(0.0, 0.0, 2.0), gaze=(0, 0, -1), near=(-1, 1, -0.75, 0.75, 2.0))
    elif name in ("last_pass", "last_skip"):
        hs = _load(directory, xml)
        first, count, depth = _last_leaf(hs)
        info.update(last_first=first, last_count=count, last_depth=depth)
        F = qu.scene_arrays(hs)[3][first]
        c = (F["v0"].astype(np.float64) + F["v1"] + F["v2"]) / 3
        if name == "last_skip":
            # from two units above the face's centroid, a view of +-0.04 there
            _edit(xml, w, h, eye=c + np.array([0, 0, 2.0]), gaze=(0, 0, -1), near=(-0.02, 0.02, -0.015, 0.015, 1))
        else:
            # the last seven faces of the row, from four units above
            _edit(xml, w, h, eye=c + np.array([-2.5, 0, 4.0]), gaze=(0, 0, -1), near=(-0.8, 0.8, -0.2, 0.2, 1))
    return _load(directory, xml), info, xml


@pytest.fixture(scope="module")
def wide_slots(tmp_path_factory):
    """The helper program, built once."""
    out = tmp_path_factory.mktemp("wide_slots")
    exe = str(out / "wide_slots_main")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")     # for the HIP vector types' header only
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ob.ROOT, "include"), "-I" + CSRC] + HELPER + ["-o", exe, "-lz"], check=True)
    return exe


def _patterns(exe, directory, xmls):
    r = subprocess.run([exe] + [os.path.basename(x) for x in xmls], cwd=str(directory), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_slot_patterns_occur(wide_slots, tmp_path):
    """Host only (no gpu mark): what the shadow cases' any-hit trees contain."""
    xmls = [prepare(tmp_path, n, 16, 8)[2] for n in PATTERN_SCENES]
    J = _patterns(wide_slots, tmp_path, xmls)
    pats, fanout, deep_iiii = {}, np.zeros(4, np.int64), False
    for name, rec in J.items():
        print(name, rec)
        fanout += np.array(rec["fanout"])
        for p, k in rec["patterns"].items():
            pats[p] = pats.get(p, 0) + k
        deep_iiii |= rec["depth"] >= 4 and "IIII" in rec["patterns"]
    assert (fanout > 0).all(), fanout
    for slot in range(4):
        assert any(p[slot] == "L" for p in pats) and any(p[slot] == "I" for p in pats), (slot, sorted(pats))
        assert (slot == 0) != any(p[slot] == "-" for p in pats), (slot, sorted(pats))
    assert not any(re.search(r"-[LI]", p) for p in pats), sorted(pats)     # slots are filled from the front
    assert deep_iiii and J["chain_16x8"]["depth"] >= 16


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stages(ds, monkeypatch, two=False):
    if two:
        monkeypatch.setenv("RTG_FRAME_KERNEL", "0")
    try:
        ds.render(0, flags=rtgpu.RTG_RENDER_TIMING)
        return list(ds.timings())
    finally:
        monkeypatch.delenv("RTG_FRAME_KERNEL", raising=False)


def _shadow_rays(hs, ds):
    """The camera rays' hit points (host walk) towards the point light, started 1e-3 along the way."""
    rays = ds.camera_rays()
    hits = hs.trace(rays)
    hit = hits["object"] >= 0
    p = qu.origins(rays)[hit].astype(np.float64) + qu.directions(rays)[hit].astype(np.float64) * hits["t"][hit, None]
    to = wc.point_light(hs).astype(np.float64)[None] - p
    dist = np.linalg.norm(to, axis=1)
    d = to / dist[:, None]
    return rtgpu.make_rays((p + 1e-3 * d).astype(f32), d.astype(f32), tmax=(dist - 2e-3).astype(f32)), hits[hit]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", CAMERA + SHADOW)
def test_node_loops(name, w, h, tmp_path, monkeypatch):
    hs, info, _ = prepare(tmp_path, name, w, h)
    ds = rtgpu.DeviceScene(hs, 0)
    try:
        stages, two_stages = _stages(ds, monkeypatch), _stages(ds, monkeypatch, two=True)
        if wc.max_leaf(hs) > 8:
            assert stages[0] == "k_primary" and "k_frame" not in stages and stages == two_stages, stages
        else:
            assert stages == ["k_frame"] and two_stages == ["k_primary", "k_shade_shadow"], (stages, two_stages)
        base = ds.render(0)
        monkeypatch.setenv("RTG_FRAME_KERNEL", "0")
        two = ds.render(0)
        monkeypatch.delenv("RTG_FRAME_KERNEL")
        ds.reset_stats()
        counted = ds.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS)
        st = ds.stats()
        ohdr, oldr, ost = ob.render(hs)
        assert base[0].shape == (h, w, 3)
        r = ob.compare(base[0], ohdr)
        print(name, w, h, r, "differing words", int((_bits(base[0]) != _bits(ohdr)).sum()),
              {k: st[k] for k in st if st[k]}, info)
        for img, which in ((two, "two kernels"), (counted, "counted")):
            assert np.array_equal(_bits(img[0]), _bits(base[0])) and np.array_equal(img[1], base[1]), (name, which)
        assert np.array_equal(_bits(base[0]), _bits(ohdr)) and np.array_equal(base[1], oldr), (name, "oracle", r)
        for k in COUNTERS:
            assert st[k] == ost[k], (name, k, st[k], ost[k])
        assert st["camera_rays"] == w * h
        # the case's premises
        rays = ds.camera_rays()
        if (w, h) == (37, 21) and name not in OBLIQUE:
            assert (qu.directions(rays) == 0).any(), "no axis-aligned camera ray"
        if name in ("last_pass", "last_skip"):
            hits = hs.trace(rays)
            face = hits["face"][hits["object"] >= 0]
            in_last = (face >= info["last_first"]) & (face < info["last_first"] + info["last_count"])
            assert in_last.any()
            if name == "last_skip":
                assert in_last.all() and ost["node_visits"] == w * h * (2 * info["last_depth"] + 1), (ost, info)
            else:
                assert not in_last.all() and ost["node_visits"] != w * h * (2 * info["last_depth"] + 1)
        if name in ("roof", "open"):
            srays, shit = _shadow_rays(hs, ds)
            occ = hs.trace(srays, any_hit=True)["object"]
            assert srays.size > w * h // 2 and st["shadow_rays"] >= srays.size
            assert np.all(occ == (0 if name == "roof" else -1)), (name, np.unique(occ, return_counts=True))
        if name == "light_inside":
            v = _case(name).meshes[0][0]
            L = wc.point_light(hs)
            assert np.all(L > v.min(0)) and np.all(L < v.max(0)) and st["shadow_rays"] > 0
        if name in SHADOW and not name.startswith("pinwheel_"):
            assert st["shadow_wide_visits"] > 0
        if name.startswith("pinwheel_"):
            nodes = hs.anyhit_check(1)["nodes"]
            assert (nodes < 4096) == (name == "pinwheel_8192")
            assert st["shadow_rays"] == w * h and st["shadow_wide_visits"] > 0
            assert (st["shadow_fallbacks"] > 0) == (name == "pinwheel_49152"), st["shadow_fallbacks"]
    finally:
        ds.close()
