"""The CPU oracle's radiance queries (oracle_radiance_rays) against the reference's own answers on the
off-camera rays of radiance_rays.py: tests/golden/radiance_rays_<scene>.npz holds, per ray, the bits
of the colour that the reference's IntersectObjects + PerformShading (or PerPixel's miss branches)
give it under both eyes, and of its primary minT (`make_goldens.py radiance_rays`).  The oracle must
give the same bits on every kept ray; test_gpu_radiance_rays.py then holds the device to the oracle.

No GPU and no reference tree is needed: only tests/golden/ and the built oracle."""
import os

import numpy as np
import pytest

import oracle_bind as ob
import query_util as qu
import radiance_rays as rr
import rtgpu

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = rr.GOLDEN_SCENES
EYES = (False, True)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)
    _cache.clear()


def _has_bg_texture(hs):
    return qu.Desc.from_address(hs.desc).bg_texture >= 0


def _scene(name):
    if name not in _cache:
        hs = rtgpu.HostScene(name + ".xml")
        rays, ids, labels, want, dropped = rr.load_golden(name)
        got = {eye: ob.radiance(hs, rays, ids, camera_eye=eye)[0] for eye in EYES}
        for a in (rays, ids, labels, *want.values(), *got.values()):
            a.setflags(write=False)
        _cache[name] = (hs, rays, ids, labels, want, dropped, got)
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference(name):
    hs, rays, ids, labels, want, dropped, got = _scene(name)
    for eye in EYES:
        ok = rr.same_bits(got[eye], want[eye]).all(1)
        bad = np.flatnonzero(~ok)
        print(name, "camera eye" if eye else "origin eye", "rays", rays.size, "differing", bad.size,
              "rays with a NaN", int(np.isnan(got[eye]).any(1).sum()))
        assert bad.size == 0, (name, eye, [rr.NAMES[int(c)] for c in labels[bad[:8]]], rays[bad[:4]], got[eye][bad[:4]],
                               want[eye][bad[:4]].view(np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_golden_is_whole(name):
    """The golden holds the generator's rays (regenerated here from the description), at most 1 % of
    them dropped because two runs of the reference differed, and no class lost."""
    hs, rays, ids, labels, want, dropped, got = _scene(name)
    g_rays, g_ids, g_labels = rr.generate(hs)
    assert dropped.sum() <= 0.01 * g_rays.size, (name, dropped)
    assert g_rays.size == rays.size + dropped.sum()
    if dropped.sum() == 0:
        assert g_rays.tobytes() == rays.tobytes() and np.array_equal(g_ids, ids) and np.array_equal(g_labels, labels)
    cam = hs.camera(0)
    assert np.all((ids >= 0) & (ids < cam["width"] * cam["height"]))
    assert np.mean(ids == np.arange(ids.size)) < 0.01           # ids are not the ray index
    for cls, c in rr.CLASSES.items():
        n = int((labels == c).sum())
        if cls == "M":
            assert (n > 0) == rr.has_motion_blur(hs), (name, cls)
        else:
            assert n > 0 and int((g_labels == c).sum()) == n + dropped[c], (name, cls)
    assert 1000 <= rays.size <= 1500
    # probes that start inside a mirror / dielectric / conductor body and meet its inner face first
    inside, spheres = rr.inside_body_probes(hs, rays, labels)
    print(name, "probes inside specular bodies", inside.size, "specular spheres", spheres)
    if spheres or name == "scienceTree_diamond":                # (the diamond: a closed dielectric mesh)
        assert inside.size >= 5, (name, inside.size)


@pytest.mark.parametrize("name", NAMES)
def test_classes_see_something(name):
    """Per class with hits: some colours that are neither black nor the colour of a miss; class X:
    misses only, and on the background-texture scenes many colours, decided by the ids."""
    hs, rays, ids, labels, want, dropped, got = _scene(name)
    bg = qu.scene_arrays(hs)[0].astype(np.float32)
    rgbt = want[False].view(np.float32)
    hit = rgbt[:, 3].view(np.uint32) != rays["tmax"].view(np.uint32)
    for cls, c in rr.CLASSES.items():
        sel = labels == c
        if not sel.any():
            continue
        col = rgbt[sel, :3]
        lit = hit[sel] & (col != 0).any(1) & (col != bg[None]).any(1) & np.isfinite(col).all(1)
        print(name, cls, "rays", int(sel.sum()), "hits", int(hit[sel].sum()), "lit", int(lit.sum()),
              "distinct colours", len(np.unique(col.view(np.uint32), axis=0)))
        if cls == "X":
            assert not hit[sel].any()
            if _has_bg_texture(hs):
                assert len(np.unique(col.view(np.uint32), axis=0)) > 10
            else:
                assert (col == bg[None]).all()
        else:
            assert lit.sum() >= 5, (name, cls)


@pytest.mark.parametrize("name", NAMES)
def test_eye_and_length_matter(name):
    """The goldens move with what they are meant to pin: the two eyes disagree on some primary hit
    (where the scene has a specular term at all), never on t; scaled directions scale t."""
    hs, rays, ids, labels, want, dropped, got = _scene(name)
    assert np.array_equal(want[False][:, 3], want[True][:, 3])
    moved = (want[False][:, :3] != want[True][:, :3]).any(1)
    print(name, "rays whose colour depends on the eye", int(moved.sum()))
    if name not in ("edge_roof", "image_tex"):                  # no specular reflectance / a depth of 1 without mirrors
        assert moved.sum() > 20
    g = np.flatnonzero(labels == rr.CLASSES["N"]).reshape(-1, len(rr.N_SCALES))
    t = want[False][:, 3].view(np.float32)[g]
    both = np.isfinite(t).all(1)
    assert both.sum() > 5
    for k in (1, 3, 4):                                         # power-of-two scales: exact where the oracle says so
        exact = t[both, k] * rr.N_SCALES[k] == t[both, 0]
        print(name, "scale", float(rr.N_SCALES[k]), "t scales exactly on", int(exact.sum()), "of", int(both.sum()))
        assert np.allclose(t[both, k] * rr.N_SCALES[k], t[both, 0], rtol=1e-4)
        assert exact.sum() > 0


@pytest.mark.parametrize("name", NAMES)
def test_tmax_cut(name):
    """Class T as the reference decides it: tmax = t misses (IntersectFace's and the sphere's t < minT
    are strict) with the miss colour and tmax's own bits; the float above hits at t with the colour
    of the unbounded ray (where the reference's box test lets it); the float below and t / 2 cut that hit too."""
    hs, rays, ids, labels, want, dropped, got = _scene(name)
    g = np.flatnonzero(labels == rr.CLASSES["T"]).reshape(-1, len(rr.T_COLUMNS))
    assert g.shape[0] >= 20
    w = want[False]
    tmax = rays["tmax"].view(np.uint32)
    t_inf = w[g[:, 4], 3]
    assert np.array_equal(tmax[g[:, 0]], t_inf)                 # the group was built around this hit
    assert np.array_equal(w[g[:, 0], 3], tmax[g[:, 0]])         # cut at t: a miss, t = tmax
    # next above: the hit, with the unbounded ray's colour -- or, on a few rays, still a miss: the
    # reference's box test (shape.hpp:78-100, tmin < minT) drops a box whose rounded entry distance
    # is an ulp beyond the distance of the face in it
    above = w[g[:, 1], 3] == t_inf
    print(name, "next-above rays that hit", int(above.sum()), "of", above.size)
    assert above.sum() >= 0.75 * above.size
    assert np.array_equal(w[g[~above, 1], 3], tmax[g[~above, 1]])
    assert np.array_equal(w[g[above, 1]], w[g[above, 4]])
    for col in (0, 2, 3):
        # a cut primary ray either misses or meets something nearer: never the hit at t
        t = w[g[:, col], 3].view(np.float32)
        assert np.all(t <= rays["tmax"][g[:, col]])
        assert np.all((w[g[:, col], 3] == tmax[g[:, col]]) | (t < t_inf.view(np.float32)))
    missed = w[g[:, 0], 3] == tmax[g[:, 0]]
    if not _has_bg_texture(hs):
        bg = qu.scene_arrays(hs)[0].astype(np.float32).view(np.uint32)
        assert np.array_equal(w[g[missed, 0], :3], np.broadcast_to(bg, (int(missed.sum()), 3)))
    objs = hs.trace(rays[g[:, 4]])["object"]
    kinds = qu.scene_arrays(hs)[1]["kind"]
    print(name, "T groups", g.shape[0], "objects", len(np.unique(objs)), "of", len(kinds))
    assert len(np.unique(objs)) >= min(len(kinds), 3)
    if qu.RTG_OBJ_INSTANCE in kinds:
        assert np.any(kinds[objs] == qu.RTG_OBJ_INSTANCE)


def test_time_is_inherited(tmp_path):
    """motion_mirror (radiance_rays.write_motion_mirror), which test_gpu_radiance_rays.py compares
    device against oracle: the fixture does what it is for.  Class M's four times of a group give
    different colours below a primary hit on the static mirror floor -- only the reflected ray meets
    the moving objects -- and so do many other rays when their time is set to 0."""
    hs = rtgpu.HostScene(rr.write_motion_mirror(tmp_path))
    rays, ids, labels = rr.generate(hs)
    want, _ = ob.radiance(hs, rays, ids)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    floor = hs.trace(rays)["object"] == 0
    g = np.flatnonzero(labels == rr.CLASSES["M"]).reshape(-1, len(rr.M_TIMES))
    on_floor = floor[g].all(1) & (bits(want[g][:, :, 3]) == bits(want[g][:, :1, 3])).all(1)
    differs = (bits(want[g][:, 1:, :3]) != bits(want[g][:, :1, :3])).any((1, 2))
    print("motion_mirror M groups", g.shape[0], "on the floor", int(on_floor.sum()), "colour moves with time",
          int((on_floor & differs).sum()))
    assert (on_floor & differs).sum() >= 1
    zero = rays.copy()
    zero["time"] = 0
    w0, _ = ob.radiance(hs, zero, ids)
    moved = (bits(w0[:, :3]) != bits(want[:, :3])).any(1)
    print("motion_mirror rays whose colour depends on time", int(moved.sum()), "of them primary hits on the floor",
          int((moved & floor).sum()))
    assert (moved & floor).sum() >= 10
