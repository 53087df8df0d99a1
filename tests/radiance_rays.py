"""Seeded off-camera rays for the radiance queries (test_radiance_rays_oracle.py,
test_gpu_radiance_rays.py and the recipe `make_goldens.py radiance_rays`): rays that no camera of the
scene produces, on which the shading reads what a camera ray never varies -- the direction's
length, an eye that is not the camera, origins on and inside the geometry, back faces, a bounded
primary ray, the motion-blur time as given, a pixel id that is not the ray's index.  A helper module
like edge_rays.py, not a conftest.

    rays, ids, labels = generate(hs)    # RAY_DTYPE array, int32 pixel id and int8 class per ray

Every construction is done in float32 on the description's own objects.

  P probe    origins uniform in the scene box, and at the centres of sphere objects and the centroids
             of mesh objects (inside the dielectric / conductor / mirror bodies where a scene has
             them); directions uniform on the sphere, unit length
  N length   groups of 5: a P ray, then its direction scaled by 0.25, 3, 2^-10 and 2^10 (N_SCALES)
  S surface  origins on a face (vertex, edge midpoint, centroid) and the same moved by
             +n and by -n * ShadowRayEpsilon (just behind the face, just inside a closed body's
             skin); directions over the +n hemisphere, and -- where the ray meets
             something -- in the face's plane and along -n
  B back     rays that reach a face's centroid from behind, and rays within 0.1 degree of a face's
             plane towards its centroid
  T tmax     groups of 5 around a known host hit at t: tmax = t, the float above, the float below,
             t / 2 and inf (T_COLUMNS), dealt over the scene's objects (transformed ones, instances
             and large-leaf meshes among them)
  M time     groups of 4: a ray towards a moving object at time 0, 0.25, 0.75, 1 - 2^-24 (M_TIMES);
             only on scenes with motion blur
  X miss     rays the host walk finds nothing on

Pixel ids are random over camera 0's image in every class, so that keys and background lookups never
coincide with the ray's index.  No non-finite rays (edge_rays class G covers them; their colour is
unspecified).
"""
import os

import numpy as np

import edge_rays as er
import query_util as qu
import rtgpu

CLASSES = {"P": 0, "N": 1, "S": 2, "B": 3, "T": 4, "M": 5, "X": 6}
NAMES = {v: k for k, v in CLASSES.items()}
f32 = np.float32
N_SCALES = np.array([1.0, 0.25, 3.0, 2.0 ** -10, 2.0 ** 10], f32)
T_COLUMNS = ("t", "above", "below", "half", "inf")
M_TIMES = np.array([0.0, 0.25, 0.75, 1.0 - 2.0 ** -24], f32)
GRAZE_DEG = 0.1
# the scenes with a golden (tests/golden/radiance_rays_<scene>.npz, `make_goldens.py radiance_rays`)
GOLDEN_SCENES = ["simple", "spheres_mirror", "cornell_dielectric", "cornell_conductors", "brdf_lights", "image_tex",
                 "transforms_textures", "bump_normal", "scienceTree_diamond", "edge_roof", "deep_mirrors_9",
                 "deep_mirrors_32", "deep_glass_12"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    """A scene's golden: rays (RAY_DTYPE), ids, labels, {camera_eye: (n, 4) uint32 -- the bits of the
    reference's r, g, b and primary minT}, rays dropped per class."""
    z = np.load(os.path.join(GOLDEN, f"radiance_rays_{name}.npz"), allow_pickle=False)
    rays = z["rays"].view(rtgpu.RAY_DTYPE).reshape(-1)
    want = {eye: np.concatenate([z[key], z["t_bits"][:, None]], 1) for eye, key in ((False, "rgb_origin"), (True, "rgb_camera"))}
    return rays, z["ids"], z["labels"], want, z["dropped"]


def same_bits(got, want):
    """Per value: equal bits, or a NaN on both sides whatever its payload."""
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return (got == want) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))


def write_motion_mirror(directory, dof_motion_xml="dof_motion.xml"):
    """dof_motion with a mirror floor and a depth of 2, written into `directory`: the one scene in
    which rays below the primary one meet moving objects, so that the time the tree inherits shows.
    Returns the path."""
    text = open(dof_motion_xml).read()
    text = text.replace("<MaxRecursionDepth>1<", "<MaxRecursionDepth>2<")
    text = text.replace('<Material id="1">', '<Material id="1" type="mirror">\n'
                        '            <MirrorReflectance>0.7 0.7 0.7</MirrorReflectance>')
    assert 'type="mirror"' in text and "Depth>2<" in text
    path = os.path.join(str(directory), "motion_mirror.xml")
    with open(path, "w") as f:
        f.write(text)
    return path


# rtg_material of include/rtgpu.h
MAT_DTYPE = np.dtype([("id", "<i4"), ("type", "<i4"), ("brdf", "<i4"), ("pad0", "<i4"), ("f", "<f4", 22)])
assert MAT_DTYPE.itemsize == 104
SPECULAR_TYPES = (0, 1, 2)                    # RTG_MAT_MIRROR, RTG_MAT_DIELECTRIC, RTG_MAT_CONDUCTOR


def inside_body_probes(hs, rays, labels):
    """(indices of the class-P rays that start at the centre of a mirror / dielectric / conductor
    object and meet that same object first -- its inner face --, number of sphere objects of such a
    material): the probes that run the tree's enter / exit logic from the inside."""
    d = qu.Desc.from_address(hs.desc)
    mats = qu._array(d.materials, d.num_materials, MAT_DTYPE)
    _, objs, _, _ = qu.scene_arrays(hs)
    _, owner = er.world_faces(hs)
    centres = object_centres(hs)
    P = np.flatnonzero(labels == CLASSES["P"])
    o, first = qu.origins(rays[P]), hs.trace(rays[P])["object"]
    found, spheres, j = [], 0, 0
    for k, ob in enumerate(objs):
        if not (ob["kind"] == qu.RTG_OBJ_SPHERE or np.any(owner == k)):
            continue
        if mats["type"][ob["material"]] in SPECULAR_TYPES:
            spheres += int(ob["kind"] == qu.RTG_OBJ_SPHERE)
            found.append(P[(o == centres[j]).all(1) & (first == k)])
        j += 1
    return (np.concatenate(found) if found else np.zeros(0, np.int64)), spheres


def has_motion_blur(hs):
    return bool(np.any(qu.scene_arrays(hs)[1]["motion_blur"]))


def object_centres(hs):
    """World centre of every sphere object and centroid of every mesh object (float32 (n, 3))."""
    _, objs, _, _ = qu.scene_arrays(hs)
    W, owner = er.world_faces(hs)
    out = []
    for k, ob in enumerate(objs):
        if ob["kind"] == qu.RTG_OBJ_SPHERE:
            out.append((ob["transform"].reshape(4, 4) @ np.append(ob["center"].astype(np.float64), 1.0))[:3])
        elif np.any(owner == k):
            out.append(W[owner == k].astype(np.float64).reshape(-1, 3).mean(0))
    return np.asarray(out, f32).reshape(-1, 3)


def scene_box(hs):
    """The padded float32 box of edge_rays.generate: world vertices and sphere extents."""
    _, objs, _, _ = qu.scene_arrays(hs)
    W, _ = er.world_faces(hs)
    pts = [W.reshape(-1, 3)]
    for ob in objs[objs["kind"] == qu.RTG_OBJ_SPHERE]:
        c = (ob["transform"].reshape(4, 4) @ np.append(ob["center"].astype(np.float64), 1.0))[:3].astype(f32)
        pts += [(c - ob["radius"])[None], (c + ob["radius"])[None]]
    pts = np.concatenate(pts).astype(f32)
    lo, hi = pts.min(0), pts.max(0)
    pad = np.maximum((hi - lo) * f32(0.25), f32(0.5))
    return (lo - pad).astype(f32), (hi + pad).astype(f32)


def _normals(v0, v1, v2):
    nrm = np.cross((v1 - v0).astype(np.float64), (v2 - v0).astype(np.float64))
    nl = np.linalg.norm(nrm, axis=1, keepdims=True)
    return (nrm / np.where(nl > 0, nl, 1)).astype(f32)


def _normalised(d):
    d = np.asarray(d, f32)
    ln = np.sqrt((d * d).sum(1, dtype=f32)).astype(f32)
    return (d / np.where(ln > 0, ln, 1)[:, None]).astype(f32)


def generate(hs, seed=20270, scale=1.0):
    """(rays, ids, labels) for a HostScene: about 1 150 to 1 300 rays at scale 1, the classes of this module's
    docstring in the order of CLASSES.  `scale` multiplies every class's count."""
    rng = np.random.default_rng(seed)
    _, objs, meshes, faces = qu.scene_arrays(hs)
    W, owner = er.world_faces(hs)
    eps = er.shadow_epsilon(hs)
    lo, hi = scene_box(hs)
    cam = hs.camera(0)
    npix = cam["width"] * cam["height"]

    def cnt(n, mult=1):
        return max(mult, int(round(n * scale / mult)) * mult)

    def inside(n):
        return (lo + (hi - lo) * rng.random((n, 3)).astype(f32)).astype(f32)

    sets = []          # (class, origins, directions, tmax or None, time or None)

    def add(cls, o, d, tmax=None, time=None):
        o = np.asarray(o, f32).reshape(-1, 3)
        d = np.asarray(d, f32).reshape(-1, 3)
        assert o.shape == d.shape
        bc = lambda a: None if a is None else np.broadcast_to(np.asarray(a, f32), (len(o),)).copy()
        sets.append((cls, o, d, bc(tmax), bc(time)))

    # ---- P: probes ----------------------------------------------------------------------------
    centres = object_centres(hs)
    nP = cnt(192)
    oP, dP = inside(nP), er._unit(rng, nP)
    if len(centres):
        nC = cnt(48)
        oC = centres[np.arange(nC) % len(centres)]
        oP, dP = np.concatenate([oC, oP]), np.concatenate([er._unit(rng, nC), dP])
    add("P", oP, dP)

    # ---- N: direction length ------------------------------------------------------------------
    nN = cnt(48)
    hitP = hs.trace(rtgpu.make_rays(oP, dP))["object"] >= 0    # three in four on rays that hit something,
    pools = [np.flatnonzero(hitP), np.flatnonzero(~hitP)]      # centres and box origins alike
    want = [min(len(pools[0]), nN - min(nN // 4, len(pools[1]))), 0]
    want[1] = nN - want[0]
    pick = np.sort(np.concatenate([pl[np.arange(w) * len(pl) // max(w, 1)] for pl, w in zip(pools, want)]))
    assert len(pick) == nN
    add("N", np.repeat(oP[pick], len(N_SCALES), 0),
        (np.repeat(dP[pick], len(N_SCALES), 0) * np.tile(N_SCALES, nN)[:, None]).astype(f32))

    # ---- S: surface origins (edge_rays class D) -------------------------------------------------
    if len(W):
        nF = cnt(24, 2)
        fp = rng.integers(len(W), size=nF)
        v0, v1, v2 = W[fp, 0], W[fp, 1], W[fp, 2]
        nrm = _normals(v0, v1, v2)
        starts = [v0, ((v0 + v1) * f32(0.5)).astype(f32), (((v0 + v1) + v2) / f32(3.0)).astype(f32)]
        starts += [(s + sg * nrm * eps).astype(f32) for sg in (f32(1), f32(-1)) for s in starts[:3]]
        e1, e2 = (v1 - v0).astype(f32), (v2 - v0).astype(f32)
        for j, s in enumerate(starts):
            h = er._unit(rng, nF)
            flip = (h * nrm).sum(1) < 0
            h[flip] = -h[flip]
            add("S", s, h)                                     # over the hemisphere
            inpl = [e1, e2, (e1 + e2).astype(f32), (e1 - e2).astype(f32), -e1][j % 5]
            # in the face's own plane, and straight back: where the host walk finds something on them
            # (a surface origin that sees nothing is a miss like any other: class X's business)
            for so, sd in ((s[:nF // 2], inpl[:nF // 2]), (s[nF // 2:], -nrm[nF // 2:])):
                seen = hs.trace(rtgpu.make_rays(so, sd))["object"] >= 0
                if seen.any():
                    add("S", so[seen], sd[seen])

    # ---- B: back faces and grazing rays ---------------------------------------------------------
    if len(W):
        nB = cnt(80)
        fp = rng.integers(len(W), size=nB)
        v0, v1, v2 = W[fp, 0], W[fp, 1], W[fp, 2]
        nrm = _normals(v0, v1, v2)
        c = (((v0 + v1) + v2) / f32(3.0)).astype(f32)
        size = np.sqrt(((v1 - v0) ** 2).sum(1)).astype(f32)
        h = (size * (f32(0.05) + f32(1.5) * rng.random(nB).astype(f32) ** 2)).astype(f32)
        side = ((v1 - v0) * (rng.random(nB).astype(f32) - f32(0.5))[:, None]
                + (v2 - v0) * (rng.random(nB).astype(f32) - f32(0.5))[:, None]).astype(f32)
        o = (c - nrm * h[:, None] + side * f32(0.2)).astype(f32)
        d = _normalised(c - o)
        assert np.all((d * nrm).sum(1) > 0)                    # from behind
        add("B", o, d)
        fp = rng.integers(len(W), size=nB)
        v0, v1, v2 = W[fp, 0], W[fp, 1], W[fp, 2]
        nrm = _normals(v0, v1, v2)
        c = (((v0 + v1) + v2) / f32(3.0)).astype(f32)
        mix = rng.random(nB).astype(f32)
        e = _normalised((v1 - v0) * (mix - f32(0.5))[:, None] + (v2 - v0) * (f32(1) - mix)[:, None])
        L = (np.sqrt(((v1 - v0) ** 2).sum(1)) * (f32(0.5) + f32(2.5) * rng.random(nB))).astype(f32)
        off = (L * f32(np.tan(np.radians(GRAZE_DEG))) * (f32(2) * rng.random(nB).astype(f32) - f32(1))).astype(f32)
        o = (c + e * L[:, None] + nrm * off[:, None]).astype(f32)
        add("B", o, _normalised(c - o))

    # ---- M: time, towards the moving objects ---------------------------------------------------
    moving = [k for k, ob in enumerate(objs) if np.any(ob["motion_blur"])]
    if moving:
        nM = cnt(24)
        allc, kk = [], 0
        for k, ob in enumerate(objs):                          # object_centres' order
            if ob["kind"] == qu.RTG_OBJ_SPHERE or np.any(owner == k):
                if k in moving:
                    allc.append(centres[kk] + f32(0.5) * ob["motion_blur"].astype(f32))
                kk += 1
        target = np.asarray(allc, f32)[np.arange(nM) % len(allc)]
        o = inside(nM)
        d = _normalised((target - o) + f32(0.15) * er._unit(rng, nM))
        add("M", np.repeat(o, len(M_TIMES), 0), np.repeat(d, len(M_TIMES), 0), time=np.tile(M_TIMES, nM))

    # ---- X: misses -------------------------------------------------------------------------------
    nX = cnt(100)
    away = inside(4 * nX)
    mid = ((lo + hi) * f32(0.5)).astype(f32)
    cand_o = np.concatenate([inside(4 * nX), away])
    cand_d = np.concatenate([er._unit(rng, 4 * nX), _normalised((away - mid) + f32(0.3) * er._unit(rng, 4 * nX))])
    miss = np.flatnonzero(hs.trace(rtgpu.make_rays(cand_o, cand_d))["object"] < 0)[:nX]
    if len(miss):
        add("X", cand_o[miss], cand_d[miss])

    # ---- T: tmax around known host hits, dealt over the objects ---------------------------------
    base_o = np.concatenate([s[1] for s in sets if s[0] in "PB"])
    base_d = np.concatenate([s[2] for s in sets if s[0] in "PB"])
    hit = hs.trace(rtgpu.make_rays(base_o, base_d))
    good = np.flatnonzero((hit["object"] >= 0) & np.isfinite(hit["t"]) & (hit["t"] > 0))
    nT = cnt(32)
    good = rng.permutation(good)
    by_obj = [good[hit["object"][good] == k] for k in np.unique(hit["object"][good])]
    chosen, r = [], 0
    while len(chosen) < min(nT, len(good)):
        for g in by_obj:
            if r < len(g) and len(chosen) < nT:
                chosen.append(g[r])
        r += 1
    for i in chosen:
        t = f32(hit["t"][i])
        tm = np.array([t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf)), t * f32(0.5), np.inf], f32)
        add("T", np.repeat(base_o[i][None], len(tm), 0), np.repeat(base_d[i][None], len(tm), 0), tm)

    order = sorted(range(len(sets)), key=lambda j: CLASSES[sets[j][0]])
    o = np.concatenate([sets[j][1] for j in order])
    d = np.concatenate([sets[j][2] for j in order])
    n = len(o)
    labels = np.concatenate([np.full(len(sets[j][1]), CLASSES[sets[j][0]], np.int8) for j in order])
    rays = rtgpu.make_rays(o, d)
    rays["tmax"] = np.concatenate([np.full(len(sets[j][1]), np.inf, f32) if sets[j][3] is None else sets[j][3]
                                   for j in order])
    # times: a few values only (0, the largest, sixteenths), the M groups' as constructed
    time = (rng.integers(16, size=n) / 16.0).astype(f32)
    time[0::7] = 0.0
    time[3::7] = er.TIME_MAX
    given = np.concatenate([np.zeros(len(sets[j][1]), bool) if sets[j][4] is None else np.ones(len(sets[j][1]), bool)
                            for j in order])
    time[given] = np.concatenate([sets[j][4] for j in order if sets[j][4] is not None]) if given.any() else []
    # the rays of an N or T group differ in length / tmax only
    for cls, k in (("N", len(N_SCALES)), ("T", len(T_COLUMNS))):
        g = np.flatnonzero(labels == CLASSES[cls]).reshape(-1, k)
        time[g] = time[g[:, :1]]
    rays["time"] = time
    ids = rng.integers(npix, size=n).astype(np.int32)
    assert np.all((rays["time"] >= 0) & (rays["time"] < 1))
    assert np.all(np.isfinite(qu.origins(rays))) and np.all(np.isfinite(qu.directions(rays)))
    return rays, ids, labels
