"""Helpers of the closest-point tests (test_closest_host.py, test_gpu_closest.py): a float64 brute
force over every face and sphere of a scene, the points the tests ask about, and two generated
scenes -- `grid`, a height field of well-shaped faces, and `moved`, a mesh, an instance and spheres
under composite transforms."""
import os

import numpy as np

import query_util as qu
import rtgpu

# |dist - d64| <= TOL * S, S the largest world-coordinate magnitude involved: 16 ulp of S.  The
# float32 region-based test measured 5.9 ulp of S against float64 on well-shaped triangles.
TOL = 2.0 ** -20


# ---------------------------------------------------------------------------
# The scene in world space, float64
# ---------------------------------------------------------------------------
class World:
    """Per object: ("mesh", face_offset, tri (F, 3, 3) float64 world vertices) or
    ("sphere", centre (3,), radius), from query_util.scene_arrays."""

    def __init__(self, hs):
        _, objs, meshes, faces = qu.scene_arrays(hs)
        self.prims = []
        for ob in objs:
            M = ob["transform"].reshape(4, 4).astype(np.float64)
            if ob["kind"] == qu.RTG_OBJ_SPHERE:
                c = M[:3, :3] @ ob["center"].astype(np.float64) + M[:3, 3]
                s = abs(np.linalg.det(M[:3, :3])) ** (1.0 / 3.0)
                self.prims.append(("sphere", c, float(ob["radius"]) * s))
            else:
                m = meshes[ob["mesh"]]
                F = faces[m["face_offset"]:m["face_offset"] + m["face_count"]]
                tri = np.stack([F["v0"], F["v1"], F["v2"]], 1).astype(np.float64)        # (F, 3, 3)
                tri = tri @ M[:3, :3].T + M[:3, 3]
                self.prims.append(("mesh", int(m["face_offset"]), tri))

    def vertices(self):
        out = [p[2].reshape(-1, 3) for p in self.prims if p[0] == "mesh"]
        out += [np.stack([p[1] - p[2], p[1] + p[2]]) for p in self.prims if p[0] == "sphere"]
        return np.concatenate(out)

    def triangles(self):
        t = [p[2] for p in self.prims if p[0] == "mesh"]
        return np.concatenate(t) if t else np.zeros((0, 3, 3))

    def sphere_centres(self):
        return np.array([p[1] for p in self.prims if p[0] == "sphere"]).reshape(-1, 3)


def _segment_d2(p, a, b):
    """Squared distance of points p to segments a-b, arrays (..., 3) that broadcast."""
    ab = b - a
    l2 = (ab * ab).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l2 > 0.0, ((p - a) * ab).sum(-1) / l2, 0.0)
    t = np.clip(t, 0.0, 1.0)
    d = p - (a + ab * t[..., None])
    return (d * d).sum(-1)


def _tri_d(p, a, b, c):
    """Distance from p to the triangles (a, b, c), arrays (..., 3) that broadcast: the nearest of
    the three edges and, where the projection falls inside, the plane."""
    d2 = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
    nrm = np.cross(b - a, c - a)
    n2 = (nrm * nrm).sum(-1)
    inside = (n2 > 0.0)
    for u, v in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(v - u, p - u) * nrm).sum(-1) >= 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = ((p - a) * nrm).sum(-1)
        plane = np.where(inside, h * h / n2, np.inf)
    return np.sqrt(np.minimum(d2, plane))


def tri_distance(p, tri):
    """Every point p (n, 3) against every triangle tri (F, 3, 3): float64 (n, F)."""
    p = np.asarray(p, np.float64)[:, None, :]
    return _tri_d(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])


def tri_distance_pairs(p, tri):
    """Point i against triangle i: float64 (n,)."""
    return _tri_d(np.asarray(p, np.float64), tri[:, 0], tri[:, 1], tri[:, 2])


def brute_force(world, pts, chunk=256):
    """The exact distance from every point to the scene: float64 (n,)."""
    pts = np.asarray(pts, np.float64)
    best = np.full(len(pts), np.inf)
    for prim in world.prims:
        if prim[0] == "sphere":
            best = np.minimum(best, np.abs(np.linalg.norm(pts - prim[1], axis=1) - prim[2]))
        else:
            tri = prim[2]
            for f in range(0, len(tri), chunk):
                best = np.minimum(best, tri_distance(pts, tri[f:f + chunk]).min(1))
    return best


def primitive_distance(world, pts, obj, face):
    """The float64 distance from point i to the primitive (obj[i], face[i]) (a global face index,
    -1 for a sphere); inf where obj[i] < 0."""
    pts = np.asarray(pts, np.float64)
    out = np.full(len(pts), np.inf)
    for k, prim in enumerate(world.prims):
        idx = np.flatnonzero(obj == k)
        if not idx.size:
            continue
        if prim[0] == "sphere":
            assert (face[idx] == -1).all()
            out[idx] = np.abs(np.linalg.norm(pts[idx] - prim[1], axis=1) - prim[2])
        else:
            local = face[idx] - prim[1]
            assert (local >= 0).all() and (local < len(prim[2])).all(), "face outside its object's mesh"
            out[idx] = tri_distance_pairs(pts[idx], prim[2][local])
    return out


# ---------------------------------------------------------------------------
# Points
# ---------------------------------------------------------------------------
def points_for(world, seed, total=4000, max_faces=256):
    """About `total` float32 points (n, 3): uniform in the scene's box inflated by half its size;
    every vertex, edge midpoint and centroid of up to max_faces faces; those centroids lifted along
    the face normal by 1e-6 to 1; sphere centres; a few points at 1e6."""
    rng = np.random.default_rng(seed)
    v = world.vertices()
    lo, hi = v.min(0), v.max(0)
    size = np.maximum(hi - lo, 1e-3)
    parts = []
    tri = world.triangles()
    if len(tri):
        tri = tri[np.unique(np.linspace(0, len(tri) - 1, min(max_faces, len(tri))).astype(int))]
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        cen = (a + b + c) / 3.0
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), 0.0)
        lift = 10.0 ** rng.uniform(-6.0, 0.0, (len(tri), 1)) * rng.choice([-1.0, 1.0], (len(tri), 1))
        parts += [a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2, cen, cen + nrm * lift]
    if len(world.sphere_centres()):
        parts.append(world.sphere_centres())
    parts.append(np.array([[1e6, 0, 0], [0, -1e6, 0], [1e6, 1e6, 1e6], [-1e6, 3.0, -1e6]]))
    fixed = sum(len(x) for x in parts)
    parts.insert(0, rng.uniform(lo - size / 2, hi + size / 2, (max(total - fixed, 1000), 3)))
    return np.concatenate(parts).astype(np.float32)


def scale_of(world, pts):
    """S per point: the largest coordinate magnitude among the scene's vertices and that point
    (never above the issue's single S over all the points, so the bound is no wider)."""
    return np.maximum(np.abs(world.vertices()).max(), np.abs(np.asarray(pts, np.float64)).max(1))


# ---------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------
_HEAD = """<Scene>
    <BackgroundColor>0 0 0</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>0.5 5 5</Position>
            <Gaze>0 -1 -0.9</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>2</NearDistance>
            <ImageResolution>64 48</ImageResolution>
            <ImageName>%s.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>0 8 5</Position><Intensity>1000 1000 1000</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>1 1 1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
    </Materials>
"""

GRID_N = 32


def _height_field(n, half, amp, seed):
    """(verts, faces): an n x n cell height field over [-half, half]^2, 2 n^2 faces, ids 1-based.
    Cells are squares of side 2 half / n with heights within amp: right triangles tilted a little."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-half, half, n + 1)
    h = rng.uniform(-amp, amp, (n + 1, n + 1))
    verts = [(float(xs[i]), float(h[j, i]), float(xs[j])) for j in range(n + 1) for i in range(n + 1)]
    faces = []
    for j in range(n):
        for i in range(n):
            a = 1 + j * (n + 1) + i
            b, c, d = a + 1, a + n + 2, a + n + 1
            faces += [(a, c, b), (a, d, c)]
    return verts, faces


def _write(directory, name, xml):
    path = os.path.join(str(directory), name + ".xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def _vtxt(verts):
    return "\n".join("        %r %r %r" % tuple(v) for v in verts)


def _ftxt(faces):
    return "\n".join("                %d %d %d" % tuple(f) for f in faces)


def write_grid(directory, name="grid"):
    """A 32 x 32 height field, 2 048 well-shaped faces, one identity mesh."""
    verts, faces = _height_field(GRID_N, 4.0, 0.05, 7)
    assert len(faces) == 2048
    xml = _HEAD % name + f"""    <VertexData>
{_vtxt(verts)}
    </VertexData>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
{_ftxt(faces)}
            </Faces>
        </Mesh>
    </Objects>
</Scene>
"""
    return _write(directory, name, xml)


# `moved`: transformations of the two placements (the second for rtg_scene_update: same geometry)
MOVED = {
    "a": dict(t=[(1.5, 0.5, -1.0), (-2.0, 1.0, 2.0), (3.0, 2.0, 1.0)], s=[(1.5, 0.7, 1.1), (0.6, 1.2, 0.9), (1.7, 1.7, 1.7)],
              r=[(35, 0, 1, 0), (-20, 1, 0, 0), (50, 0, 0, 1)]),
    "b": dict(t=[(-1.0, 0.8, 0.5), (2.5, 0.5, -2.0), (-3.0, 2.5, 0.0)], s=[(0.8, 1.4, 1.2), (1.3, 0.7, 1.1), (0.9, 0.9, 0.9)],
              r=[(-50, 0, 1, 0), (30, 1, 0, 0), (15, 0, 0, 1)]),
}


def write_moved(directory, name="moved", placement="a", sphere_scaling="s3"):
    """A mesh under rotation plus non-uniform scale, an instance of it under another composite
    (composed with the mesh's own), a uniformly scaled and rotated sphere, an identity sphere.
    sphere_scaling: the scaled sphere's scaling ("s1": non-uniform, an ellipsoid)."""
    verts, faces = _height_field(8, 1.0, 0.2, 11)
    c1, c2 = len(verts) + 1, len(verts) + 2
    verts += [(0.0, 0.0, 0.0), (-3.0, 1.0, -2.0)]
    P = MOVED[placement]
    tr = "\n".join(f'        <Translation id="{i + 1}">%r %r %r</Translation>' % t for i, t in enumerate(P["t"]))
    sc = "\n".join(f'        <Scaling id="{i + 1}">%r %r %r</Scaling>' % s for i, s in enumerate(P["s"]))
    ro = "\n".join(f'        <Rotation id="{i + 1}">%r %r %r %r</Rotation>' % r for i, r in enumerate(P["r"]))
    xml = _HEAD % name + f"""    <VertexData>
{_vtxt(verts)}
    </VertexData>
    <Transformations>
{tr}
{sc}
{ro}
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Transformations>s1 r1 t1</Transformations>
            <Faces>
{_ftxt(faces)}
            </Faces>
        </Mesh>
        <MeshInstance id="2" baseMeshId="1">
            <Material>1</Material>
            <Transformations>r2 s2 r3 t2</Transformations>
        </MeshInstance>
        <Sphere id="3"><Material>1</Material><Transformations>{sphere_scaling} r1 t3</Transformations><Center>{c1}</Center><Radius>0.75</Radius></Sphere>
        <Sphere id="4"><Material>1</Material><Center>{c2}</Center><Radius>0.5</Radius></Sphere>
    </Objects>
</Scene>
"""
    return _write(directory, name, xml)


def load(path, device_bvh=False):
    """HostScene of a generated scene (it refers to no other file)."""
    return rtgpu.HostScene(str(path), device_bvh=device_bvh)


def u32(a):
    """NEAREST_DTYPE records as raw words, (n, 8)."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 8)


def same(got, want, what):
    g, w = u32(got), u32(want)
    bad = np.flatnonzero((g != w).any(1))
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:4]], want[bad[:4]])
