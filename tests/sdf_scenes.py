"""Helpers of the crossing-count and signed-distance tests (test_crossings_host.py,
test_gpu_crossings.py): a generated scene of closed shapes with an analytic inside, the grazing
flags of multihit_scenes.brute_force_all carried over to transformed objects, and the interpolated
height of closest_util's height field.  A helper module like multihit_scenes.py, not a conftest.

The closed-shapes scene (inline vertex data, every mesh wound outwards):

  object 0   a box [-1, 1]^3, each side a 4 x 4 grid of quads (192 triangles)
  object 1   a hollow shell around (-6, 0, 0): an outer box [-2, 2]^3 and, in the same mesh, an
             inner box [-1, 1]^3 wound inwards (the cavity's normals point into the cavity)
  object 2   an instance of object 0's mesh under two rotations, uniform scale 0.8 and a translation
  object 3   a sphere of radius 1 at (0, 5, 0)
(the loader's order: meshes, instances, spheres)

No two shapes overlap, so a point is inside the scene's solid exactly when it is inside an odd
number of the five surfaces: the shell's cavity is outside.
"""
import numpy as np

import closest_util as cu
import multihit_scenes as ms
import query_util as qu
import rtgpu

SHELL_CENTRE = np.array([-6.0, 0.0, 0.0])
SPHERE_CENTRE = np.array([0.0, 5.0, 0.0])
COPY_SCALE = 0.8
COPY_ROTATIONS = ((30.0, 0.0, 1.0, 0.0), (-20.0, 1.0, 0.0, 0.0))          # degrees, axis
COPY_TRANSLATION = (5.0, 0.0, 1.0)
DEFAULT_DIR = np.array(rtgpu.SDF_DEFAULT_DIRECTION, np.float32)


def _box(verts, centre, half, n, inwards=False):
    """Append the vertices of a box of n x n quads per side to verts; returns its faces (1-based
    ids), each wound so that its normal points out of the box (into it with inwards)."""
    faces = []
    ts = np.linspace(-half, half, n + 1)
    for axis in range(3):
        for sign in (1.0, -1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3      # e_u x e_v = e_axis
            if sign < 0:
                u, v = v, u
            base = len(verts) + 1
            for j in range(n + 1):
                for i in range(n + 1):
                    p = np.array(centre, np.float64)
                    p[axis] += sign * half
                    p[u] += ts[i]
                    p[v] += ts[j]
                    verts.append(tuple(float(x) for x in p))
            for j in range(n):
                for i in range(n):
                    a = base + j * (n + 1) + i
                    b, c, d = a + 1, a + n + 2, a + n + 1
                    faces += [(a, c, b), (a, d, c)] if inwards else [(a, b, c), (a, c, d)]
    return faces


def write_closed(directory, name="closed"):
    verts = []
    box = _box(verts, (0, 0, 0), 1.0, 4)
    shell = _box(verts, SHELL_CENTRE, 2.0, 4) + _box(verts, SHELL_CENTRE, 1.0, 4, inwards=True)
    centre = len(verts) + 1
    verts.append(tuple(float(x) for x in SPHERE_CENTRE))
    xml = cu._HEAD % name + f"""    <VertexData>
{cu._vtxt(verts)}
    </VertexData>
    <Transformations>
        <Translation id="1">%r %r %r</Translation>
        <Scaling id="1">{COPY_SCALE!r} {COPY_SCALE!r} {COPY_SCALE!r}</Scaling>
        <Rotation id="1">%r %r %r %r</Rotation>
        <Rotation id="2">%r %r %r %r</Rotation>
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
{cu._ftxt(box)}
            </Faces>
        </Mesh>
        <Mesh id="2">
            <Material>1</Material>
            <Faces>
{cu._ftxt(shell)}
            </Faces>
        </Mesh>
        <Sphere id="3"><Material>1</Material><Center>{centre}</Center><Radius>1.0</Radius></Sphere>
        <MeshInstance id="4" baseMeshId="1">
            <Material>1</Material>
            <Transformations>r1 r2 s1 t1</Transformations>
        </MeshInstance>
    </Objects>
</Scene>
""" % (COPY_TRANSLATION + COPY_ROTATIONS[0] + COPY_ROTATIONS[1])
    return cu._write(directory, name, xml)


def load_closed(directory, device_bvh=False):
    hs = cu.load(write_closed(directory), device_bvh=device_bvh)
    if not device_bvh:
        _, objs, meshes, _ = qu.scene_arrays(hs)
        assert [int(k) for k in objs["kind"]] == [qu.RTG_OBJ_MESH, qu.RTG_OBJ_MESH, qu.RTG_OBJ_INSTANCE, qu.RTG_OBJ_SPHERE]
        assert [int(c) for c in meshes["face_count"]] == [192, 384]
    return hs


def closed_points(hs, n, seed):
    """n seeded float32 points, uniform in the bounds of the scene's world-space vertices."""
    v = cu.World(hs).vertices()
    return np.random.default_rng(seed).uniform(v.min(0), v.max(0), (n, 3)).astype(np.float32)


def closed_inside(hs, xyz):
    """Per point, in float64: (inside an odd number of the surfaces, how many it is inside of)."""
    _, objs, _, _ = qu.scene_arrays(hs)
    p = np.asarray(xyz, np.float64)
    count = (np.abs(p).max(1) < 1.0).astype(int)
    q = p - SHELL_CENTRE
    count += (np.abs(q).max(1) < 2.0).astype(int) + (np.abs(q).max(1) < 1.0).astype(int)
    count += (np.linalg.norm(p - SPHERE_CENTRE, axis=1) < 1.0).astype(int)
    inv = objs[2]["inv_transform"].reshape(4, 4).astype(np.float64)
    local = p @ inv[:3, :3].T + inv[:3, 3]
    count += (np.abs(local).max(1) < 1.0).astype(int)
    return (count & 1) == 1, count


def grazing(hs, o, d):
    """multihit_scenes.brute_force_all's grazing flags for the rays (o, d) on a scene whose objects
    may be transformed: object by object, the rays carried into the object's space in float64 (a
    barycentric coordinate and a sphere's discriminant ratio do not change under an affine map)
    and the object's record given the identity.  Also returns every ray's float64 hit count."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    flags = np.zeros(len(o), bool)
    count = np.zeros(len(o), int)
    for k in range(len(objs)):
        one = objs[k:k + 1].copy()
        inv = one[0]["inv_transform"].reshape(4, 4).astype(np.float64)
        one["inv_transform"][0] = np.eye(4).reshape(-1)
        hits, g = ms.brute_force_all(one, meshes, faces, o @ inv[:3, :3].T + inv[:3, 3], d @ inv[:3, :3].T)
        flags |= g
        count += np.array([len(h) for h in hits])
    return flags, count


class Grid:
    """closest_util.write_grid's height field (heights along y over the x-z plane) as a function:
    the height of the triangulated surface above (x, z), in float64."""

    def __init__(self):
        verts, _ = cu._height_field(cu.GRID_N, 4.0, 0.05, 7)
        self.n, self.half = cu.GRID_N, 4.0
        self.h = np.array([v[1] for v in verts], np.float64).reshape(self.n + 1, self.n + 1)      # [j (z), i (x)]
        self.range = float(self.h.max() - self.h.min())

    def height(self, x, z):
        cell = 2.0 * self.half / self.n
        fu = (np.asarray(x, np.float64) + self.half) / cell
        fv = (np.asarray(z, np.float64) + self.half) / cell
        i = np.clip(np.floor(fu).astype(int), 0, self.n - 1)
        j = np.clip(np.floor(fv).astype(int), 0, self.n - 1)
        u, v = fu - i, fv - j
        ha, hb, hc, hd = self.h[j, i], self.h[j, i + 1], self.h[j + 1, i + 1], self.h[j + 1, i]
        # _height_field's faces (a, c, b) and (a, d, c): the diagonal a - c
        return np.where(u >= v, ha + u * (hb - ha) + v * (hc - hb), ha + v * (hd - ha) + u * (hc - hd))
