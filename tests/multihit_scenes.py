"""Helpers of the multi-hit query tests (test_multihit_host.py, test_gpu_multihit.py): a generated
layered scene with an analytic answer, its rays, and a float64 brute force that returns every hit.
A helper module like query_util.py, not a conftest.

The layered scene (identity transforms, inline vertex data):

  object 0   one mesh of 12 square sheets at z = -1 ... -12, each an 8 x 8 grid of quads on
             [-4, 4]^2 (128 triangles a sheet, 1 536 faces: a BVH with depth)
  object 1   a second mesh that repeats the z = -5 sheet: the same vertices in the same order, so
             every hit on it ties exactly with object 0's
  2, 3, 4    spheres of radius 1, 2, 3 around (0, 0, -20), behind sheet 12

A ray from z = 0 straight down -z with x, y off the grid lines and the quads' diagonals meets
sheet j at t = j (sheet 5 twice: object 0, then object 1) and then the six sphere roots
20 -+ sqrt(r^2 - x^2 - y^2).
"""
import os

import numpy as np

import query_util as qu
import rtgpu

SHEETS = 12
GRID = 8
HALF = 4.0
TIE_SHEET = 5
SPHERE_Z = -20.0
RADII = (1.0, 2.0, 3.0)
FACES_PER_SHEET = 2 * GRID * GRID


def write_layered(tmp_path) -> str:
    """Write layered.xml into tmp_path and return its path."""
    n = GRID + 1
    xs = np.linspace(-HALF, HALF, n)
    verts, faces0, faces1 = [], [], []
    for s in range(1, SHEETS + 1):
        base = len(verts) + 1                       # vertex ids are 1-based
        for j in range(n):
            for i in range(n):
                verts.append((float(xs[i]), float(xs[j]), -float(s)))
        sheet = []
        for j in range(GRID):
            for i in range(GRID):
                a = base + j * n + i
                b, c, d = a + 1, a + n + 1, a + n
                sheet += [(a, b, c), (a, c, d)]
        faces0 += sheet
        if s == TIE_SHEET:
            faces1 = list(sheet)
    centre = len(verts) + 1
    verts.append((0.0, 0.0, SPHERE_Z))
    vtxt = "\n".join("        %r %r %r" % v for v in verts)

    def ftxt(fs):
        return "\n".join("                %d %d %d" % f for f in fs)

    spheres = "\n".join(
        f'        <Sphere id="{i + 1}"><Material>1</Material><Center>{centre}</Center><Radius>{r!r}</Radius></Sphere>'
        for i, r in enumerate(RADII))
    xml = f"""<Scene>
    <BackgroundColor>0 0 0</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>0.3 0.2 3</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>1</NearDistance>
            <ImageResolution>64 48</ImageResolution>
            <ImageName>layered.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>0 0 5</Position><Intensity>1000 1000 1000</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>1 1 1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
    </Materials>
    <VertexData>
{vtxt}
    </VertexData>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
{ftxt(faces0)}
            </Faces>
        </Mesh>
        <Mesh id="2">
            <Material>1</Material>
            <Faces>
{ftxt(faces1)}
            </Faces>
        </Mesh>
{spheres}
    </Objects>
</Scene>
"""
    path = os.path.join(str(tmp_path), "layered.xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def load_layered(tmp_path):
    """The layered scene as a HostScene (no textures or PLY files: the directory does not matter)."""
    hs = rtgpu.HostScene(write_layered(tmp_path))
    _, objs, meshes, _ = qu.scene_arrays(hs)
    assert [int(k) for k in objs["kind"]] == [qu.RTG_OBJ_MESH, qu.RTG_OBJ_MESH] + [qu.RTG_OBJ_SPHERE] * 3
    assert [int(c) for c in meshes["face_count"]] == [SHEETS * FACES_PER_SHEET, FACES_PER_SHEET]
    return hs


def axis_points(n, seed, radius=0.6):
    """n seeded (x, y) inside all three spheres' silhouette, at least 0.05 from every grid line
    and from both diagonals of their quad."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x, y = rng.uniform(-radius, radius, 2)
        fx, fy = x - np.floor(x), y - np.floor(y)
        if min(fx, 1 - fx, fy, 1 - fy, abs(fx - fy), abs(fx + fy - 1)) >= 0.05 and np.hypot(x, y) < radius:
            out.append((x, y))
    return np.array(out, np.float32)


def axis_rays(xy, z0=0.0, down=True, tmax=np.inf):
    """Rays from (x, y, z0) along -z (or +z)."""
    o = np.concatenate([xy, np.full((len(xy), 1), z0, np.float32)], 1)
    d = np.tile(np.array([0, 0, -1 if down else 1], np.float32), (len(xy), 1))
    return rtgpu.make_rays(o, d, tmax=tmax)


def axis_answer(xy):
    """The analytic list of the rays axis_rays(xy) in float64: (t, object, sheet, face) per ray,
    19 entries; sheet is 0 and face -1 / -2 for the sphere roots (the root the reference
    selects -- the near one, the origin being outside -- first)."""
    rows = []
    for x, y in np.asarray(xy, np.float64):
        row = []
        for s in range(1, SHEETS + 1):
            row.append((float(s), 0, s, 0))
            if s == TIE_SHEET:
                row.append((float(s), 1, s, 0))
        roots = []
        for k, r in enumerate(RADII):
            h = np.sqrt(r * r - x * x - y * y)
            roots += [(-SPHERE_Z - h, 2 + k, 0, -1), (-SPHERE_Z + h, 2 + k, 0, -2)]
        rows.append(row + sorted(roots))
    return rows


def slanted_rays(n, seed):
    """n seeded slanted rays through the layered scene: half start between sheets 5 and 6 and head
    down to a point of the plane z = -20 (seven sheets, then the spheres for most), half start
    below the spheres and head up through them into the sheets.  (No ray meets the duplicated
    sheet within its first nine hits: an exact tie is a near tie, which the brute-force test
    leaves out.)"""
    rng = np.random.default_rng(seed)
    h = n // 2
    o1 = np.stack([rng.uniform(-3, 3, h), rng.uniform(-3, 3, h), rng.uniform(-5.9, -5.1, h)], 1)
    p1 = np.stack([rng.uniform(-3.5, 3.5, h), rng.uniform(-3.5, 3.5, h), np.full(h, SPHERE_Z)], 1)
    m = n - h
    o2 = np.stack([rng.uniform(-3, 3, m), rng.uniform(-3, 3, m), rng.uniform(-30, -24, m)], 1)
    ang, rad = rng.uniform(0, 2 * np.pi, m), 0.9 * np.sqrt(rng.random(m))
    p2 = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(m, SPHERE_Z)], 1)
    o = np.concatenate([o1, o2])
    d = np.concatenate([p1, p2]) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rtgpu.make_rays(o, d)


def brute_force_all(objs, meshes, faces, o, d, edge=1e-5):
    """query_util.brute_force returning every hit: all faces and both roots of every sphere in
    float64, no BVH (identity transforms only).  Returns (hits, grazing): hits[i] is ray i's list
    of (t, object) with t > 0 in ascending t (ties in object order); grazing as brute_force's,
    taken over all faces and spheres."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    n = len(o)
    grazing = np.zeros(n, bool)
    ident = np.eye(4).reshape(-1)
    found = []                                       # (ray indices, t, object) per face / root
    for k, ob in enumerate(objs):
        assert np.array_equal(ob["inv_transform"], ident), "brute force handles identity transforms only"
        if ob["kind"] == qu.RTG_OBJ_SPHERE:
            c, r = ob["center"].astype(np.float64), float(ob["radius"])
            oc = o - c
            a = (d * d).sum(1)
            b = 2.0 * (d * oc).sum(1)
            cc = (oc * oc).sum(1) - r * r
            disc = b * b - 4.0 * a * cc
            grazing |= np.abs(disc) < edge * b * b
            sq = np.sqrt(np.maximum(disc, 0.0))
            for t in ((-b - sq) / (2.0 * a), (-b + sq) / (2.0 * a)):
                idx = np.flatnonzero((disc > 0.0) & (t > 0.0))
                found.append((idx, t[idx], np.full(idx.size, k)))
            continue
        m = meshes[ob["mesh"]]
        for F in faces[m["face_offset"]:m["face_offset"] + m["face_count"]]:
            v0, v1, v2 = (F[x].astype(np.float64) for x in ("v0", "v1", "v2"))
            e1, e2 = v1 - v0, v2 - v0
            p = np.cross(d, e2)
            det = p @ e1
            with np.errstate(divide="ignore", invalid="ignore"):
                s = o - v0
                beta = (s * p).sum(1) / det
                qv = np.cross(s, e1)
                gamma = (d * qv).sum(1) / det
                tf = (qv @ e2) / det
            third = 1.0 - beta - gamma
            inside = (det != 0.0) & (beta >= 0.0) & (gamma >= 0.0) & (third >= 0.0) & (tf > 0.0)
            near = (det != 0.0) & (tf > 0.0) & (beta > -edge) & (gamma > -edge) & (third > -edge) & \
                (np.minimum(np.minimum(np.abs(beta), np.abs(gamma)), np.abs(third)) < edge)
            grazing |= near
            idx = np.flatnonzero(inside)
            found.append((idx, tf[idx], np.full(idx.size, k)))
    ray = np.concatenate([f[0] for f in found])
    t = np.concatenate([f[1] for f in found])
    obj = np.concatenate([f[2] for f in found])
    order = np.lexsort((obj, t, ray))
    hits = [[] for _ in range(n)]
    for i, tt, kk in zip(ray[order], t[order], obj[order]):
        hits[int(i)].append((float(tt), int(kk)))
    return hits, grazing
