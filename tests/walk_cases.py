"""Cases, seeded ray sets and comparison helpers that pin the BVH *walks* (test_walk_cases_host.py,
test_gpu_walk_cases.py, test_ahb.py, the edge-ray suites and the `walk_rays` recipe of
tests/golden/make_goldens.py) on the adversarial meshes of bvh_cases.py and on the walk-only cases
below.  A helper module like query_util.py, not a conftest.

Walk-only cases (generated at test time, never recorded as BVH goldens -- they are not in
bvh_cases.NAMES: their BVH goldens would exceed make_goldens.BVH_MAX_BYTES):

  pinwheel_<n>          n = 8 192 and 49 152.  Triangle i has the vertices (-1 - a, -1 - b, z_i),
                        (1 + c, -1.5 - d, z_i), (-1.5 - e, 1 + f, z_i - 1/256) with z_i = -i and seeded
                        jitters a..f in [0, 0.4).  Every face box -- and so every node box of the
                        reference's BVH and of the any-hit trees -- contains the z axis, and no
                        face touches it: the hypotenuse x + y = -0.5 (jittered: at most -0.1) passes
                        the origin on the far side, at a distance of at least 0.07.  A ray up or down
                        the axis therefore passes every box of the tree and meets no face.  Unit
                        spacing keeps the reference's leaves at about three faces (no large leaf, so
                        not FEAT_BIGLEAF: the scene takes the wide any-hit walk), and the default
                        any-hit tree has about n / 6 wide nodes: below walk_wide_any_pk's
                        RTG_PK_MAX_STEPS = 4096 for n = 8 192, above it for n = 49 152.  The tests
                        assert these premises from the host before they rely on them.
  pinwheel_<n>_blocked  the same and one face across the axis at z = -n - 1/2, below the last layer.

An any-hit tree that overflows the walk's 64-entry stack (RTG_PK_STACK): not found.  The packet
pushes only inner children (leaf slots are tested in place), at most three per wide node it
descends, and only those whose boxes some lane passes: to hold more than 64 entries a ray needs a
path of at least 22 wide nodes whose inner siblings it pierces all along.  Tried through
anyhit_check(1)["depth"], on the host: the pinwheels, where the axis rays pierce every sibling
box, reach depth 6 at 8 192 faces and 8 at 49 152 (the binned SAH cuts the stack into balanced
runs, so the depth is about log4 of the size: 22 levels of full fan-out would take 4^22 leaves);
`chain`, 92 levels in the reference's BVH, has depth 31 collapsed (mode 0) and 17 in the default
tree, but only 30 wide nodes in all -- a comb with one inner child per level pushes nothing --;
coincident copies (copies_300) are one leaf slot per 255 faces.  A comb whose every level has a
second inner child pierced by the same ray takes boxes that grow along the ray, and the SAH then
puts the large ones together near the root; no generator that defeats that was found.  The
stack-full branch of walk_wide_any_pk is therefore reached by no test, and none claims it.

Ray sets, all seeded:

  edge    edge_rays.generate(hs) as it is
  aimed   from a seeded origin outside the mesh box towards a point inside a seeded face whose
          barycentrics are all at least 0.05, and the same rays with tmax = 0.5 t and 1.5 t of
          the host's own answer: max(1 024, 8 per face) rays a case (the pinwheels stay at 4 096,
          where 8 per face would be 393 216 rays).  Two choices in the construction come from what
          float32 can carry, found with the host walk (which equals the reference bit for bit) on
          a first version that drew origins on a sphere of 1.5 to 3 box radii:
            * the direction is at least 14.5 degrees off the face's plane (|cos| to its normal
              >= 0.25, redrawn otherwise): the float32 t of a ray that skims its face is
              conditioned like 1 / cos, and spread_2 missed the brute force's 1e-4 on t (1.8e-4);
            * the origin lies just outside the box -- the point where the ray enters it, moved
              back by one to three of the face's longest edges: the float32 barycentrics carry an
              error of about 2^-24 |origin - face| / |edge|, which from hundreds of units off the
              lattice's faces of 1/128 (or thousands off the pinwheels') is far above the brute
              force's grazing band of 1e-5, and the walk then disagreed about a neighbouring face
              on 3 of 28 112 rays.  `chain` alone (faces of 2^-44 to 2^47 in one box; over such
              distances the face test's determinants overflow) starts its rays that near the face
              itself, inside the box, and aims at the faces whose edges are below 2^40 (on the
              larger ones |edge|^2 |vertex - origin| is beyond FLT_MAX for any origin off the
              centroid, and the reference itself misses them).
  light   from each bvh_cases.face_rays origin to the scene's point light, tmax = the distance:
          the shadow rays a render casts (the pinwheels: a seeded 2 048 of them, each crossing
          most of the stack's boxes)
  axis    (pinwheels) 256 rays within 0.05 of the axis, up and down, with direction components
          across the axis of 1e-8 .. 2e-7 (not zero: a zero component would send the ray to the
          reference walk at once): unbounded, and with tmax just short of and just past the blocker
"""
import os

import numpy as np

import bvh_cases as bc
import edge_rays as er
import query_util as qu
import rtgpu

f32 = np.float32

PINWHEEL_SIZES = (8192, 49152)
WALK_ONLY = tuple(f"pinwheel_{n}{b}" for n in PINWHEEL_SIZES for b in ("", "_blocked"))
# the cases whose reference answers are recorded (tests/golden/walk_rays_<case>.npz)
RECORDED = ("copies_9", "copies_17", "copies_255", "copies_256", "copies_300", "nested_256", "chain", "empty_half",
            "tie_split", "zeros_shuffled", "subnormal", "huge_empty", "several")
# (label, any_hit, coherent, normals): every ds.trace variant
VARIANTS = [("trace", False, False, False), ("coherent", False, True, False), ("normals", False, False, True),
            ("normals+coherent", False, True, True), ("any_hit", True, False, False),
            ("any_hit+coherent", True, True, False)]
MAX_CALL = 4096
# ray-set labels beyond edge_rays.CLASSES (one int8 label space for the goldens)
SETS = dict(er.CLASSES, aimed=16, aimed_short=17, aimed_long=18, light=19)
SET_NAMES = {v: k for k, v in SETS.items()}
AIMED_MIN, AIMED_PER_FACE, AIMED_CAP = 1024, 8, 32768
AIMED_WALK_ONLY = 4096
LIGHT_WALK_ONLY = 2048
AIMED_MIN_COS = 0.25
# faces from 2^-44 to 2^47 in one box: the aimed rays start near their face, not outside the box
BOX_TOO_LARGE = ("chain",)
GRAZING_CAP = 0.01
T_REL = 1e-4


# ---- cases ------------------------------------------------------------------------------------

def pinwheel_size(name):
    return int(name.split("_")[1])


def pinwheel_blocker_z(n):
    return -float(n) - 0.5


def pinwheel(n, blocked=False, seed=77):
    rng = np.random.default_rng(seed * 100003 + n)
    j = rng.uniform(0.0, 0.4, (n, 6))
    z = -np.arange(n, dtype=np.float64)
    v = np.empty((n, 3, 3))
    v[:, 0] = np.stack([-1 - j[:, 0], -1 - j[:, 1], z], 1)
    v[:, 1] = np.stack([1 + j[:, 2], -1.5 - j[:, 3], z], 1)
    v[:, 2] = np.stack([-1.5 - j[:, 4], 1 + j[:, 5], z - 1.0 / 256], 1)
    if blocked:
        zb = pinwheel_blocker_z(n)
        v = np.concatenate([v, np.array([[(-3, -3, zb), (3, -3, zb), (0, 3, zb)]], np.float64)])
    v = v.astype(f32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def is_walk_only(name):
    return name in WALK_ONLY


def get(name):
    """The bvh_cases.Case of a bvh_cases name or of a walk-only name."""
    if name in bc.CASES:
        return bc.get(name)
    assert name in WALK_ONLY, name
    return bc.Case([pinwheel(pinwheel_size(name), name.endswith("_blocked"))])


# bvh_cases.write_scene looks at the whole mesh box from twice its extent away, which on these
# cases leaves every face smaller than a pixel (the 64 x 48 frame shows the background alone):
# (camera position, the point it looks at) for the walks' renders
CLOSE_UPS = {"nested_256": ((0.5, 0.3, 6.0), (0.0, 0.1, 0.0)),
             "lattice": ((400.02, 0.14, 0.4), (400.0, 0.125, 0.0)),
             "lattice_uv": ((400.02, 0.14, 0.4), (400.0, 0.125, 0.0)),
             "several": ((22.0, 20.0, 40.0), (16.0, 16.0, 16.0))}
for _name in WALK_ONLY:
    CLOSE_UPS[_name] = ((12.0, 9.0, -4.0), (0.0, 0.0, -8.0))        # the stack's top layers from the side


def load(directory, name, device_bvh=False):
    """Write the case's scene (bvh_cases.write_scene; the camera of CLOSE_UPS where the case has
    one) into `directory` and load it."""
    import re
    xml = os.path.join(str(directory), name + ".xml")
    if not os.path.exists(xml):
        bc.write_scene(get(name), str(directory), name)
        if name in CLOSE_UPS:
            eye, at = (np.array(p, np.float64) for p in CLOSE_UPS[name])
            s, k = re.subn(r"<Position>[^<]*</Position>\s*<Gaze>[^<]*</Gaze>",
                           "<Position>%s</Position><Gaze>%s</Gaze>" % (bc._g(eye), bc._g(at - eye)), open(xml).read(), count=1)
            assert k == 1
            with open(xml, "w") as f:
                f.write(s)
    old = os.getcwd()
    os.chdir(str(directory))
    try:
        return rtgpu.HostScene(name + ".xml", device_bvh=device_bvh)
    finally:
        os.chdir(old)


FLOOR_HALF = 0.5


def load_pinwheel_floor(directory, name):
    """pinwheel_<n>[_blocked] over a small floor, for the step-bound renders: the stack (and the
    blocker at z = -n - 1/2) as mesh 1, a square floor of two faces at z = -n - 2 as mesh 2, the
    point light on the axis at z = 2 above the stack, and the camera between blocker and floor,
    looking down at the floor's middle from a little off the axis (no pixel's floor point lies on
    the axis itself, where a zero direction component would send its shadow ray to the reference
    walk for another reason).  The shadow ray of a floor point within about 0.1 of the axis runs
    up the axis through every node box of the stack's any-hit tree; those further out meet one
    of the lowest layers.  Returns the HostScene."""
    import re
    n = pinwheel_size(name)
    zf, h = -float(n) - 2.0, FLOOR_HALF
    floor = (np.array([(-h, -h, zf), (h, -h, zf), (h, h, zf), (-h, h, zf)], f32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    case = bc.Case([pinwheel(n, name.endswith("_blocked")), floor])
    tag = name + "_floor"
    xml = bc.write_scene(case, str(directory), tag)
    s = open(xml).read()
    eye = (0.0137, -0.4, zf + 0.8)
    gaze = tuple(-c for c in (eye[0], eye[1], 0.8))
    for pat, val in ((r"<Position>[^<]*</Position>\s*<Gaze>[^<]*</Gaze>\s*<Up>[^<]*</Up>",
                      "<Position>%r %r %r</Position><Gaze>%r %r %r</Gaze><Up>0 0 1</Up>" % (eye + gaze)),
                     (r"<NearPlane>[^<]*</NearPlane>\s*<NearDistance>[^<]*</NearDistance>",
                      "<NearPlane>-0.25 0.25 -0.1875 0.1875</NearPlane><NearDistance>1</NearDistance>"),
                     (r"<PointLight id=\"1\"><Position>[^<]*</Position>", '<PointLight id="1"><Position>0 0 2</Position>')):
        s, k = re.subn(pat, val, s, count=1)
        assert k == 1, pat
    with open(xml, "w") as f:
        f.write(s)
    old = os.getcwd()
    os.chdir(str(directory))
    try:
        return rtgpu.HostScene(tag + ".xml")
    finally:
        os.chdir(old)


def max_leaf(hs):
    """The largest leaf of the description's BVH (faces)."""
    nd = er.node_array(hs)
    leaves = nd[nd["left"] < 0]
    return int(leaves["count"].max()) if len(leaves) else 0


def point_light(hs):
    """Position (float32[3]) of the description's first point light (rtg_point_light: position,
    intensity)."""
    d = qu.Desc.from_address(hs.desc)
    assert d.num_point_lights >= 1
    return qu._array(d.point_lights, 1, np.dtype([("position", "<f4", 3), ("intensity", "<f4", 3)]))[0]["position"]


# ---- ray sets ---------------------------------------------------------------------------------

def aimed_count(name, n_faces):
    if is_walk_only(name):
        return AIMED_WALK_ONLY
    return min(max(AIMED_MIN, AIMED_PER_FACE * n_faces), AIMED_CAP)


def aimed_base(hs, name, seed=20270):
    """(rays, face) -- the unbounded aimed rays and the world face (edge_rays.world_faces order)
    each was aimed at.  Computed in float64 and rounded once."""
    W, _ = er.world_faces(hs)
    n = aimed_count(name, len(W))
    rng = np.random.default_rng(seed)
    face = rng.integers(len(W), size=n)
    if name in BOX_TOO_LARGE:
        # |edge|^2 |vertex - origin| must stay below FLT_MAX in the face test's determinants: faces
        # whose longest edge is below 2^40 (the larger ones are hit by bvh_cases.face_rays alone)
        w64 = W.astype(np.float64)
        ok = np.flatnonzero(np.max([np.linalg.norm(w64[:, a] - w64[:, b], axis=1)
                                    for a, b in ((0, 1), (1, 2), (2, 0))], 0) < 2.0 ** 40)
        face = ok[rng.integers(len(ok), size=n)]
    # barycentrics at least 0.05 from every edge: 0.05 + 0.85 * a point of the unit simplex
    u = rng.dirichlet((1.0, 1.0, 1.0), size=n) * 0.85 + 0.05
    w = W[face].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        target = (w * u[:, :, None]).sum(1)
    pts = W.reshape(-1, 3).astype(np.float64)
    pts = pts[np.all(np.isfinite(pts), 1)]
    lo, hi = pts.min(0), pts.max(0)
    with np.errstate(over="ignore", invalid="ignore"):
        normal = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        longest = np.max([np.linalg.norm(w[:, a] - w[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], 0)
    direction = np.zeros((n, 3))
    todo = np.arange(n)
    for _ in range(64):
        d = rng.normal(size=(todo.size, 3))
        direction[todo] = d / np.linalg.norm(d, axis=1, keepdims=True)
        with np.errstate(over="ignore", invalid="ignore"):
            steep = np.abs((direction[todo] * normal[todo]).sum(1)) >= AIMED_MIN_COS
        todo = todo[~(steep | ~np.isfinite(normal[todo]).all(1))]
        if not todo.size:
            break
    assert not todo.size
    # back along the ray out of the mesh box (the slab exit), and on by one to three of the face's
    # longest edges
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        s = np.where(direction > 0, (target - lo) / direction, (target - hi) / direction)     # >= 0, inf for d = 0
        back = np.where(np.isfinite(s), s, np.inf).min(1) + longest * rng.uniform(1.0, 3.0, n)
        origin = target - direction * back[:, None]
    if name in BOX_TOO_LARGE:
        # no float32 ray from outside this box can tell its small faces apart, and the face test's
        # determinants overflow over such distances: from near the face, inside the box
        origin = target - direction * (longest * rng.uniform(1.0, 3.0, n))[:, None]
    return rtgpu.make_rays(origin.astype(f32), direction.astype(f32)), face


def aimed_rays(hs, name, seed=20270):
    """(rays, labels, face): the aimed rays, then the same with tmax = 0.5 t and 1.5 t of the host
    walk's own hit (tmax stays infinite where the host misses)."""
    base, face = aimed_base(hs, name, seed)
    t = hs.trace(base)["t"]
    short, long_ = base.copy(), base.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        short["tmax"] = (t * f32(0.5)).astype(f32)
        long_["tmax"] = (t * f32(1.5)).astype(f32)
    rays = np.concatenate([base, short, long_])
    labels = np.repeat(np.array([SETS["aimed"], SETS["aimed_short"], SETS["aimed_long"]], np.int8), base.size)
    return rays, labels, np.tile(face, 3)


def light_rays(hs, cap=0):
    """From each bvh_cases.face_rays origin to the point light, tmax = the distance, the direction
    normalised (float64, rounded once); rays whose origin or direction is not finite are left out.
    cap: a seeded choice of that many (the pinwheels: each of these rays crosses most of the
    stack's boxes, and one per face would be 49 152 of them per query variant)."""
    W, owner = er.world_faces(hs)
    o, _ = bc.face_rays(W, owner)
    L = point_light(hs).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        d = L[None] - o.astype(np.float64)
        dist = np.linalg.norm(d, axis=1)
        d /= dist[:, None]
    ok = np.flatnonzero(np.all(np.isfinite(o), 1) & np.all(np.isfinite(d), 1) & np.isfinite(dist.astype(f32)) & (dist > 0))
    if cap and ok.size > cap:
        ok = np.sort(np.random.default_rng(20274).choice(ok, cap, replace=False))
    return rtgpu.make_rays(o[ok], d[ok].astype(f32), tmax=dist[ok].astype(f32))


def axis_rays(n, seed=20271, count=256):
    """(rays, up, kind) for pinwheel_<n>: `count` rays within 0.05 of the z axis -- origins within
    0.03, a drift of less than 0.015 over the stack --, half down from z = 1 and half up from
    z = -n - 3, each three times: kind 0 unbounded, 1 tmax just short of the blocker's plane,
    2 just past it (factors 1 -+ 2^-10 on the distance to z = pinwheel_blocker_z(n))."""
    rng = np.random.default_rng(seed + n)
    ang, rad = rng.uniform(0, 2 * np.pi, count), 0.03 * np.sqrt(rng.random(count))
    up = np.arange(count) % 2 == 1
    o = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.where(up, -float(n) - 3.0, 1.0)], 1)
    across = rng.uniform(1e-8, 2e-7, (count, 2)) * np.where(rng.random((count, 2)) < 0.5, -1.0, 1.0)
    d = np.concatenate([across, np.where(up, 1.0, -1.0)[:, None]], 1)
    assert np.all(np.hypot(o[:, 0], o[:, 1]) + (n + 4) * np.hypot(across[:, 0], across[:, 1]) < 0.05)
    t_block = np.abs(pinwheel_blocker_z(n) - o[:, 2])                # d.z = +-1
    base = rtgpu.make_rays(o.astype(f32), d.astype(f32))
    short, past = base.copy(), base.copy()
    short["tmax"] = (t_block * (1 - 2.0 ** -10)).astype(f32)
    past["tmax"] = (t_block * (1 + 2.0 ** -10)).astype(f32)
    return (np.concatenate([base, short, past]), np.tile(up, 3), np.repeat(np.arange(3), count))


def blocker_face(hs, n):
    """The blocker's index into faces[] of a host-built pinwheel_<n>_blocked (BVH order)."""
    faces = qu.scene_arrays(hs)[3]
    at = np.flatnonzero(faces["v0"][:, 2] == f32(pinwheel_blocker_z(n)))
    assert at.size == 1
    return int(at[0])


def ray_sets(hs, name, edge=True):
    """The case's (rays, labels): edge (classes A-G), aimed, light."""
    parts, labels = [], []
    if edge:
        r, l = er.generate(hs)
        parts.append(r), labels.append(l)
    r, l, _ = aimed_rays(hs, name)
    parts.append(r), labels.append(l)
    r = light_rays(hs, LIGHT_WALK_ONLY if is_walk_only(name) else 0)
    parts.append(r), labels.append(np.full(r.size, SETS["light"], np.int8))
    return np.concatenate(parts), np.concatenate(labels)


# ---- float64 brute force ----------------------------------------------------------------------

def world_objects(hs):
    """objects / meshes / faces of the description with every translated instance turned into a
    plain mesh of world-space faces, so that query_util.brute_force (identity transforms only)
    covers it: a translation by small integers of float32 vertices is exact in float64.  Returns
    (objects, meshes, faces, orig): orig[i] is the description's face index of faces[i] (what a hit
    on it reports)."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    objs, meshes = objs.copy(), meshes.copy()
    extra, orig = [], [np.arange(len(faces))]
    base = len(faces)
    ident = np.eye(4).reshape(-1)
    for k in range(len(objs)):
        if np.array_equal(objs[k]["inv_transform"], ident):
            continue
        M = objs[k]["transform"].reshape(4, 4)
        assert np.array_equal(M[:3, :3], np.eye(3)), "a translation only"
        m = meshes[objs[k]["mesh"]]
        F = faces[m["face_offset"]:m["face_offset"] + m["face_count"]].copy()
        for key in ("v0", "v1", "v2"):
            F[key] = (F[key].astype(np.float64) + M[:3, 3]).astype(f32)
        nm = np.zeros(1, qu.MESH_DTYPE)
        nm["face_offset"], nm["face_count"] = base, len(F)
        meshes = np.concatenate([meshes, nm])
        objs[k]["mesh"] = len(meshes) - 1
        objs[k]["inv_transform"] = ident
        extra.append(F)
        orig.append(np.arange(m["face_offset"], m["face_offset"] + m["face_count"]))
        base += len(F)
    return objs, meshes, np.concatenate([faces] + extra), np.concatenate(orig)


def brute_force_nearest_two(objs, meshes, faces, o, d, edge=1e-5, chunk=64):
    """query_util.brute_force's arithmetic and predicate, face-major in blocks: per ray the nearest
    hit (t, object, face index into `faces`), the second nearest t over all faces, and the
    grazing flag.  (The per-face Python loop of query_util.brute_force over all rays takes an
    hour on the larger cases; test_walk_cases_host.py checks this function against it, and
    against multihit_scenes.brute_force_all, on small ones.)"""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    n = len(o)
    dd = (d * d).sum(1)
    t1, t2 = np.full(n, np.inf), np.full(n, np.inf)
    k1, f1 = np.full(n, -1), np.full(n, -1)
    grazing = np.zeros(n, bool)
    for k, ob in enumerate(objs):
        assert ob["kind"] != qu.RTG_OBJ_SPHERE
        m = meshes[ob["mesh"]]
        for b in range(int(m["face_offset"]), int(m["face_offset"] + m["face_count"]), chunk):
            e = min(b + chunk, int(m["face_offset"] + m["face_count"]))
            F = faces[b:e]
            v0, v1, v2 = (F[x].astype(np.float64)[:, None, :] for x in ("v0", "v1", "v2"))   # (c, 1, 3)
            # only the rays whose line passes the block's bounding sphere (with a margin far above
            # the `edge` band around a face): the others are inside or near none of its faces
            pts = np.concatenate([v0, v1, v2]).reshape(-1, 3)
            with np.errstate(all="ignore"):
                c = (pts.min(0) + pts.max(0)) / 2
                R = np.sqrt(((pts - c) ** 2).sum(1).max()) * 1.01
                oc = c[None] - o
                along = (oc * d).sum(1)
                far = (oc * oc).sum(1) - along * along / dd > R * R
            r = np.flatnonzero(~far) if np.isfinite(R) else np.arange(n)    # (a NaN compares false: kept)
            if not r.size:
                continue
            e1, e2 = v1 - v0, v2 - v0
            with np.errstate(all="ignore"):
                p = np.cross(d[r][None], e2)                                # (c, m, 3)
                det = (p * e1).sum(2)
                s = o[r][None] - v0
                beta = (s * p).sum(2) / det
                qv = np.cross(s, e1)
                gamma = (d[r][None] * qv).sum(2) / det
                tf = (qv * e2).sum(2) / det
                third = 1.0 - beta - gamma
                inside = (det != 0.0) & (beta >= 0.0) & (gamma >= 0.0) & (third >= 0.0) & (tf > 0.0)
                near = (det != 0.0) & (tf > 0.0) & (beta > -edge) & (gamma > -edge) & (third > -edge) & \
                    (np.minimum(np.minimum(np.abs(beta), np.abs(gamma)), np.abs(third)) < edge)
            grazing[r] |= near.any(0)
            tf = np.where(inside, tf, np.inf)
            for row in np.flatnonzero(inside.any(1)):                       # faces in order: ties keep the first
                t = tf[row]
                better = t < t1[r]
                t2[r] = np.where(better, t1[r], np.minimum(t2[r], t))
                k1[r] = np.where(better, k, k1[r])
                f1[r] = np.where(better, b + row, f1[r])
                t1[r] = np.where(better, t, t1[r])
    return t1, k1, f1, t2, grazing


def check_brute_force(name, hs, rays, hits):
    """Closest hits `hits` of `rays` against the float64 brute force, test_query_host.py's
    criterion: hit / miss and the object agree on every ray that is not grazing, t within T_REL
    relative (of max(1, |t|)); the face agrees wherever the float64 answer is unique, i.e. the
    next hit is more than T_REL relative behind (which leaves coincident copies out by
    construction).  Grazing: barycentrics within 1e-5 of an edge of some face, or the nearest
    hit within T_REL relative of tmax; at most GRAZING_CAP of the rays.  Returns the figures."""
    objs, meshes, faces, orig = world_objects(hs)
    # (the three tmax variants of an aimed ray share one line: computed once)
    od = np.concatenate([qu.origins(rays), qu.directions(rays)], 1)
    _, first, inverse = np.unique(od.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    t1, k1, f1, t2, grazing = (a[inverse] for a in brute_force_nearest_two(objs, meshes, faces, od[first, :3], od[first, 3:]))
    tmax = rays["tmax"].astype(np.float64)
    scale = np.maximum(1.0, np.abs(t1))
    with np.errstate(invalid="ignore"):
        grazing = grazing | (np.isfinite(t1) & (np.abs(t1 - tmax) <= T_REL * np.abs(t1)))
        expect = t1 < tmax
    share = float(grazing.mean())
    print(name, "aimed rays", rays.size, "grazing", int(grazing.sum()), "share %.5f" % share)
    assert share <= GRAZING_CAP, (name, share)          # a condition on the rays, not a tolerance
    keep = ~grazing
    want_obj = np.where(expect, k1, -1)
    bad = np.flatnonzero(keep & (hits["object"] != want_obj))
    assert bad.size == 0, (name, "object", bad[:8], rays[bad[:4]], hits[bad[:4]], want_obj[bad[:4]], t1[bad[:4]])
    hit = keep & expect
    rel = np.abs(hits["t"][hit].astype(np.float64) - t1[hit]) / scale[hit]
    assert np.all(rel <= T_REL), (name, "t", float(rel.max()))
    unique = hit & ((t2 - t1) > T_REL * np.abs(t1))
    bad = np.flatnonzero(unique & (hits["face"] != orig[np.maximum(f1, 0)]))
    assert bad.size == 0, (name, "face", bad[:8], rays[bad[:4]], hits[bad[:4]], orig[f1[bad[:4]]])
    miss = keep & ~expect
    assert np.all(hits["face"][miss] == -1) and np.all(hits["t"][miss].view(np.uint32) == rays["tmax"][miss].view(np.uint32))
    return {"rays": int(rays.size), "grazing": int(grazing.sum()), "grazing_share": share, "hits": int(hit.sum()),
            "unique_faces": int(unique.sum()), "max_rel_t": float(rel.max()) if rel.size else 0.0}


# ---- comparisons ------------------------------------------------------------------------------

def check_host_equals_reference(name, rays, labels, g, hits, occ, label_names=None):
    """The host walk's closest hits and occlusion booleans against the reference's recorded answers
    g (has_hit, t_bits, position, occluded): the hit flag, the bits of t, the object (= the
    reference's loop position) and the occlusion boolean, on every ray, nothing left out."""
    names = label_names or er.NAMES

    def _names(rows):
        return [(int(i), names[int(labels[i])]) for i in rows[:8]]

    ref_hit = g["has_hit"] != 0
    bad = np.flatnonzero((hits["object"] >= 0) != ref_hit)
    assert bad.size == 0, (name, "hit flag", _names(bad), rays[bad[:4]], hits[bad[:4]])
    bad = np.flatnonzero(hits["t"].view(np.uint32) != g["t_bits"])
    assert bad.size == 0, (name, "t bits", _names(bad), rays[bad[:4]], hits[bad[:4]], g["t_bits"][bad[:4]])
    bad = np.flatnonzero(hits["object"] != g["position"])
    assert bad.size == 0, (name, "object", _names(bad), hits[bad[:4]], g["position"][bad[:4]])
    bad = np.flatnonzero((occ == 0) != (g["occluded"] != 0))
    assert bad.size == 0, (name, "occlusion", _names(bad), rays[bad[:4]])
    assert set(np.unique(occ)) <= {0, -1}


def device_pool(hs, ds, rays, labels):
    """A pool of rays -- `rays`, then the scene's camera rays -- with the host walk's answers on it
    (rays are independent, so any submission's expected bytes are a gather from the pool)."""
    pool = np.concatenate([rays, ds.camera_rays()])
    h_hits, h_nrm = hs.trace(pool, normals=True)
    h_occ = hs.trace(pool, any_hit=True)
    sc = {"hs": hs, "ds": ds, "labels": labels, "pool": pool, "hits": h_hits, "nrm": h_nrm, "occ": h_occ,
          "n_edge": rays.size}
    for a in (labels, pool, h_hits, h_nrm, h_occ):
        a.setflags(write=False)
    return sc


def compare_device(name, cls, mix, sc, idx, ds=None):
    """Every variant of ds.trace on the pool rays `idx` against the host walk's answers, raw
    bytes, at most MAX_CALL rays per call."""
    idx = np.asarray(idx)
    ds = ds or sc["ds"]
    for b in range(0, idx.size, MAX_CALL):
        sel = idx[b:b + MAX_CALL]
        part = np.ascontiguousarray(sc["pool"][sel])
        for label, any_hit, coherent, normals in VARIANTS:
            where = (name, "class " + cls, mix, label)
            got = ds.trace(part, any_hit=any_hit, coherent=coherent, normals=normals)
            hits, nrm = got if normals else (got, None)
            if any_hit:                       # the occlusion boolean (the t field is not part of the answer)
                want = sc["occ"][sel]
                bad = np.flatnonzero(hits["object"] != want["object"])
            else:
                want = sc["hits"][sel]
                bad = np.flatnonzero((hits.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(1))
            assert bad.size == 0, (where, "first differing rays (lane, pool index; edge rays are below %d)" % sc["n_edge"],
                                   list(zip(((b + bad[:8]) % 64).tolist(), sel[bad[:8]].tolist())), part[bad[:4]],
                                   "device", hits[bad[:4]], "host", want[bad[:4]])
            if any_hit:
                assert set(np.unique(hits["object"])) <= {0, -1}, where
            if normals:
                h_nrm = sc["nrm"][sel]
                badn = np.flatnonzero((nrm.view(np.uint32) != h_nrm.view(np.uint32)).any(1))
                assert badn.size == 0, (where, "normals", sel[badn[:8]], part[badn[:4]], nrm[badn[:4]], h_nrm[badn[:4]])
    return idx.size


def one_per_wave(edge, n_edge, n_cam, rng):
    """Waves of 63 consecutive camera rays and one edge ray: lane 0 in even waves, lane 63 in odd
    ones."""
    m = edge.size
    out = n_edge + (rng.integers(n_cam, size=m)[:, None] + np.arange(64)[None]) % n_cam
    out[np.arange(m), np.where(np.arange(m) % 2 == 0, 0, 63)] = edge
    return out.reshape(-1)


def half_waves(edge, n_edge, n_cam, rng):
    """Edge and camera rays in alternate lanes: 32 edge lanes per wave."""
    m = edge.size
    out = np.empty(2 * m, np.int64)
    out[0::2] = edge
    out[1::2] = n_edge + (rng.integers(n_cam) + np.arange(m)) % n_cam
    return out


def mixes(name, cls, sc, edge, rng, ds=None):
    """The rays `edge` of the pool alone, at one lane per 64 and at 32 lanes per 64."""
    n_edge, n_cam = sc["n_edge"], sc["pool"].size - sc["n_edge"]
    n = compare_device(name, cls, "alone", sc, edge, ds)
    n += compare_device(name, cls, "1 edge lane per 64", sc, one_per_wave(edge, n_edge, n_cam, rng), ds)
    n += compare_device(name, cls, "32 edge lanes per 64", sc, half_waves(edge, n_edge, n_cam, rng), ds)
    return n
