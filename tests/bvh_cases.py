"""Adversarial meshes for the BVH build (test_bvh_build_host.py, test_gpu_bvh_cases.py and the
`bvh` recipe of tests/golden/make_goldens.py), generated deterministically.  A helper module like
query_util.py, not a conftest.

    case = CASES[name]()            # Case: meshes [(verts float32 (nv, 3), faces int (nf, 3) 0-based)],
                                    # an optional instance and optional texture coordinates
    xml = write_scene(case, directory, name)   # a minimal scene: one camera, one point light, one
                                               # matte material; vertices written with %.9g

Every test first checks that the values survive the loader bit for bit (check_round_trip), the
-0.0 and subnormal cases included: they do, as written, so nothing had to be rescaled.

No case has a zero-area face.  What each case is for:

  spread_<n>        1, 2, 3, 63, 64, 65, 255, 256, 257, 513 well-spread faces: the scans with
                    n = 1, the wave-uniform and mixed paths of the child-box reduction
  copies_<n>        n copies of one triangle, n in 2, 8, 9, 16, 17, 254, 255, 256, 300: all centroids are equal
                    and above the split, so every face is big, the root stays a leaf in the order the
                    swap loop leaves behind, and the leaf word crosses the 254 / 255 packing boundary;
                    8 / 9 and 16 / 17 sit either side of the walks' large-leaf and deferred-leaf
                    thresholds (kBigLeaf, kDeferLeaf)
  nested_256        256 different triangles whose centroids share x = the split: as copies_256, but
                    the order the loop leaves behind shows in the face records
  lattice           one cell for every big / small pattern of length 2..8 with both halves non-empty
                    (494 cells, 3514 faces): cell k holds tiny dyadic triangles whose centroid is
                    exactly (k, +-1/8, -i/64) for the cell's i-th face (stacked in z, the smaller
                    above the larger, so that every face is the first hit of a ray from just above
                    it; z plays no part in any split); x splits isolate the cells and the cell's
                    node splits on y.  The arrival order at that node depends on the x history alone,
                    so the signs are assigned in a second pass from the arrival order the model reports
  empty_half        every face small at an inner node (a sliver stretches the box, its centroid
                    stays below the split), and the mirror image with every face big
  tie_axis_*        node boxes with lenX == lenY == lenZ, lenX == lenY > lenZ, lenY == lenZ > lenX,
                    lenX == lenZ > lenY
  tie_split         centroids exactly equal to the split: they go right
  zeros_<order>     box minima and maxima that are +0.0 / -0.0, in three parse orders: the zero a
                    child box keeps is the first seen, the mesh box keeps the last
  chain             102 faces at x = 2^k and x = -2^k: 92 levels, one or two splitting nodes each
  huge_empty        coordinates near 3e38: the root's length overflows to inf, the split is inf and
                    every face is small
  huge_split        the same with centroids that overflow to +-inf themselves
  subnormal         40 faces of subnormal coordinates (multiples of 2^-145) and one ordinary face that
                    takes the root's other half, so that a node's box and split are subnormal
  negative          a mesh wholly in the negative octant: the mesh box's max corner stays FLT_MIN
  several           meshes of 1, 2 and 257 faces and the lattice in one scene, and an instance of the
                    257-face mesh: non-zero face and node offsets
  lattice_uv        the lattice with texture coordinates and the normal map of the bump_normal
                    fixture (face_uv, face_v12)
"""
import functools
import hashlib
import os
import shutil

import numpy as np

import bvh_model

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NORMAL_MAP = os.path.join(HERE, "golden", "scenes", "inputs", "normalmap.ppm")


class Case:
    def __init__(self, meshes, instance=None, uv=False):
        self.meshes = [(np.ascontiguousarray(v, f32), np.ascontiguousarray(f, np.int32)) for v, f in meshes]
        self.instance = instance        # (mesh index, (tx, ty, tz)) or None
        self.uv = uv

    def vertex_sha256(self):
        h = hashlib.sha256()
        for v, f in self.meshes:
            h.update(v.view(np.uint32).tobytes())
            h.update(f.astype("<i4").tobytes())
        return h.hexdigest()


def _soup(centres, offsets):
    """One triangle per centre: its own three vertices centre + offsets[i] (n, 3, 3)."""
    v = (np.asarray(centres, np.float64)[:, None, :] + np.asarray(offsets, np.float64)).astype(f32).reshape(-1, 3)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def spread(n, seed=1, lo=-4.0, hi=4.0, size=0.35):
    rng = np.random.default_rng(seed * 1000 + n)
    return _soup(rng.uniform(lo, hi, (n, 3)), rng.uniform(-size, size, (n, 3, 3)))


def _centred(cx, cy, cz, h, hy=None, dz=0.0):
    """A triangle whose float32 centroid is exactly (cx, cy, cz) for dyadic arguments: the sums
    (a + b) + c are exact multiples of three."""
    hy = h if hy is None else hy
    return [(cx - h, cy - hy, cz - dz), (cx + h, cy - hy, cz - dz), (cx, cy + 2 * hy, cz + 2 * dz)]


def copies(n):
    # centroid (8/3, 1/3, 0): x is the long axis, the split is 2 and every copy is big
    v = np.array([(0, 0, 0), (4, 0, 0), (4, 1, 0)], f32)
    return v, np.tile(np.array([[0, 1, 2]], np.int32), (n, 1))


def nested(n):
    # centroid (0, 0, -k): face k spans x in [-(k + 1), k + 1], so the split is 0 = every centroid's x;
    # the larger faces lie below the smaller, so each is the first hit of a ray from just above it
    tri = [_centred(0.0, 0.0, -float(k), float(k + 1), 0.25) for k in range(n)]
    return _soup(np.zeros((n, 3)), np.array(tri))


def lattice_patterns():
    return [tuple(bool((bits >> i) & 1) for i in range(L)) for L in range(2, 9) for bits in range(1, 2 ** L - 1)]


def _lattice(signs):
    """signs[k][i]: True puts face i of cell k at y = +1/8 (big at the cell's y split)."""
    tri = []
    for k, cell in enumerate(signs):
        for i, s in enumerate(cell):
            tri.append(_centred(float(k), 0.125 if s else -0.125, -i / 64.0, (i + 1) / 128.0))
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


@functools.lru_cache(maxsize=None)
def _lattice_signs():
    pats = lattice_patterns()
    start = np.cumsum([0] + [len(p) for p in pats])
    first = bvh_model.build(*_lattice([[i % 2 == 0 for i in range(len(p))] for p in pats]))   # placeholder signs
    cell_node = {}
    for node, faces in first.arrivals.items():
        k = int(np.searchsorted(start, faces[0], side="right")) - 1
        if len(faces) == len(pats[k]) and set(faces) == set(range(start[k], start[k + 1])) and k not in cell_node:
            cell_node[k] = node                     # the first node that holds exactly cell k: its y split
    assert len(cell_node) == len(pats)
    signs = []
    for k, p in enumerate(pats):
        s = [None] * len(p)
        for at, face in enumerate(first.arrivals[cell_node[k]]):
            s[face - start[k]] = p[at]
        signs.append(s)
    return signs


def lattice():
    return _lattice(_lattice_signs())


def empty_half():
    tri = []
    for i in range(9):      # low group: tiny faces at y in [0, 1/2] and a sliver up to y = 10
        tri.append(_centred(0.25 + i / 16.0, 0.125 + (i % 4) / 16.0, i / 32.0, 1 / 32.0))
    tri.append([(0.375, 0.0, 0.0), (0.625, 0.0, 0.0), (0.5, 10.0, 0.25)])          # centroid y = 10/3 < 5
    for i in range(9):      # mirror image: tiny faces at y in [9.5, 10] and a sliver down to y = 0
        tri.append(_centred(8.25 + i / 16.0, 9.875 - (i % 4) / 16.0, i / 32.0, 1 / 32.0))
    tri.append([(8.375, 10.0, 0.0), (8.625, 10.0, 0.0), (8.5, 0.0, 0.25)])         # centroid y = 20/3 >= 5
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


def tie_axis(ext):
    """16 faces inside a box of exactly `ext`, pinned by a face at each of two opposite corners."""
    rng = np.random.default_rng(sum(int(e * 8) * 31 ** j for j, e in enumerate(ext)))
    e = np.array(ext, np.float64)
    tri = [[(0, 0, 0), (e[0] / 8, 0, e[2] / 16), (0, e[1] / 8, e[2] / 8)],
           [tuple(e), (e[0] * 7 / 8, e[1], e[2] * 15 / 16), (e[0], e[1] * 7 / 8, e[2] * 7 / 8)]]
    for _ in range(14):
        c = np.round(rng.uniform(0.15, 0.85, 3) * e * 64) / 64
        tri.append((c + np.round(rng.uniform(-0.1, 0.1, (3, 3)) * e * 64) / 64).tolist())
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


def tie_split():
    # the root spans x in [0, 8] exactly, y and z stay within 1: the split is 4
    tri = [_centred(0.25, 0.5, 0.0, 0.25, 0.125), _centred(7.75, 0.5, 0.0, 0.25, 0.125)]
    for i, cx in enumerate([4, 1, 4, 7, 4, 2, 6, 4, 3, 5, 4, 2, 6, 4]):
        tri.append(_centred(float(cx), 0.25 + (i % 5) / 8.0, (i % 3) / 8.0, 0.125, 0.0625, 0.03125))
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


def zeros(order):
    """24 faces: the even ones (y < 12) span x in [-1, +-0], the odd ones (y >= 16) x in [+-0, 1],
    all of them z in [+-0, 1/4], the sign of each zero taken from the face's number; `order`
    permutes the parse order."""
    tri = []
    for i in range(24):
        zx = -0.0 if (i * 5 + 1) % 3 == 0 else 0.0
        za = -0.0 if (i // 2) % 2 == 0 else 0.0
        zb = -0.0 if (i * 7) % 4 < 2 else 0.0
        y = float(i // 2) if i % 2 == 0 else 16.0 + i // 2
        if i % 2 == 0:
            tri.append([(-1.0, y, za), (zx, y, zb), (-0.5, y + 0.5, 0.25)])
        else:
            tri.append([(zx, y, za), (1.0, y, zb), (0.5, y + 0.5, 0.25)])
    tri = np.array(tri)
    perm = {"forward": np.arange(24), "reversed": np.arange(24)[::-1],
            "shuffled": np.random.default_rng(6).permutation(24)}[order]
    v = tri[perm].astype(f32).reshape(-1, 3)
    assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def chain():
    tri = []
    # (2^-44 .. 2^47: beyond that the face test's own determinants underflow or overflow, and a
    # face could no longer be hit)
    for k in range(-44, 48):
        c = 2.0 ** k
        tri.append(_centred(c, 0.0, 0.0, c / 8, c / 16, c / 32))
    for k in range(38, 48):
        c = -(2.0 ** k)
        tri.append(_centred(c, 0.0, 0.0, -c / 8, -c / 16, -c / 32))
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


def huge(split):
    # x near -3e38 and, for `split`, +3e38 (centroid sums overflow to +-inf) or +1e38 (they do not)
    rng = np.random.default_rng(38 + split)
    xs = [-3e38] * 6 + [3e38 if split else 1e38] * 6
    tri = []
    for i, x in enumerate(xs):
        o = rng.uniform(-1e36, 1e36, (3, 3))
        tri.append((np.array([x, (i % 3) * 1e37, (i % 2) * 1e37]) + o).tolist())
    return _soup(np.zeros((len(tri), 3)), np.array(tri))


def subnormal():
    rng = np.random.default_rng(145)
    c = rng.integers(4000, 60000, (40, 3)).astype(np.float64)
    o = rng.integers(-2000, 2001, (40, 3, 3)).astype(np.float64)
    v, f = _soup(c * 2.0 ** -145, o * 2.0 ** -145)
    assert np.all(np.abs(v) < np.finfo(f32).tiny) and np.all(v != 0)
    # the mesh box's max corner starts at FLT_MIN, above every subnormal: alone, these faces would
    # all be small at the root.  One ordinary face far away takes the root's right half, and the
    # left child's box and split are subnormal arithmetic
    anchor = np.array([(1, 1, 1), (1.5, 1, 1.25), (1, 1.5, 1.5)], f32)
    return np.concatenate([v, anchor]), np.arange(len(v) + 3, dtype=np.int32).reshape(-1, 3)


def negative():
    return spread(48, seed=9, lo=-8.0, hi=-1.0, size=0.3)


def several():
    v257, f257 = spread(257, seed=3)
    return Case([spread(1, seed=2), spread(2, seed=2), (v257 + f32(16.0), f257), lattice()],
                instance=(2, (32, -8, 4)))


def _case(fn, *a):
    return lambda: Case([fn(*a)])


CASES = {}
for _n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 513):
    CASES[f"spread_{_n}"] = _case(spread, _n)
for _n in (2, 8, 9, 16, 17, 254, 255, 256, 300):
    CASES[f"copies_{_n}"] = _case(copies, _n)
CASES["nested_256"] = _case(nested, 256)
CASES["lattice"] = _case(lattice)
CASES["empty_half"] = _case(empty_half)
for _name, _ext in (("xyz", (8, 8, 8)), ("xy", (8, 8, 4)), ("yz", (4, 8, 8)), ("xz", (8, 4, 8))):
    CASES[f"tie_axis_{_name}"] = _case(tie_axis, _ext)
CASES["tie_split"] = _case(tie_split)
for _o in ("forward", "reversed", "shuffled"):
    CASES[f"zeros_{_o}"] = _case(zeros, _o)
CASES["chain"] = _case(chain)
CASES["huge_empty"] = _case(huge, 0)
CASES["huge_split"] = _case(huge, 1)
CASES["subnormal"] = _case(subnormal)
CASES["negative"] = _case(negative)
CASES["several"] = several
CASES["lattice_uv"] = lambda: Case([lattice()], uv=True)
NAMES = list(CASES)
# the cases whose copies coincide: a ray at one of them is answered by the first in the final order
COINCIDENT = tuple(n for n in NAMES if n.startswith("copies_"))
# the cases on which the intersection arithmetic itself overflows or underflows (a determinant of
# differences near 1e36, or of subnormals, is inf or 0): no ray is required to hit there
UNHITTABLE = ("huge_empty", "huge_split", "subnormal")


@functools.lru_cache(maxsize=None)
def get(name):
    return CASES[name]()


def _g(row):
    return " ".join("%.9g" % x for x in row)


def write_scene(case, directory, name):
    """Write <directory>/<name>.xml (and inputs/normalmap.ppm for a textured case); returns the path.
    Load it with the current directory at `directory`."""
    verts = np.concatenate([v for v, _ in case.meshes])
    finite = verts[np.all(np.isfinite(verts), 1)].astype(np.float64)
    lo, hi = finite.min(0), finite.max(0)
    centre = (lo + hi) / 2
    ext = float(np.clip((hi - lo).max(), 1e-30, 1e30))
    if case.instance:
        ext *= 2
    cam = centre + np.array([0.0, 0.0, 2 * ext])
    light = centre + np.array([ext, ext, 3 * ext])
    power = 1000 * float(np.clip(ext * ext, 1e-30, 1e30))
    objects, base = [], 1
    for k, (v, f) in enumerate(case.meshes):
        faces = "\n                ".join("%d %d %d" % tuple(r) for r in (f + base))
        tex = "\n            <Textures>1</Textures>" if case.uv else ""
        objects.append(f"""        <Mesh id="{k + 1}">
            <Material>1</Material>{tex}
            <Faces>
                {faces}
            </Faces>
        </Mesh>""")
        base += len(v)
    xform = textures = texcoords = ""
    if case.instance:
        k, t = case.instance
        xform = f"""    <Transformations>
        <Translation id="1">{_g(t)}</Translation>
    </Transformations>
"""
        objects.append(f"""        <MeshInstance id="{len(case.meshes) + 1}" baseMeshId="{k + 1}">
            <Material>1</Material>
            <Transformations>t1</Transformations>
        </MeshInstance>""")
    if case.uv:
        os.makedirs(os.path.join(directory, "inputs"), exist_ok=True)
        shutil.copyfile(NORMAL_MAP, os.path.join(directory, "inputs", "normalmap.ppm"))
        textures = """    <Textures>
        <Images>
            <Image id="1">normalmap.ppm</Image>
        </Images>
        <TextureMap id="1" type="image">
            <ImageId>1</ImageId>
            <DecalMode>replace_normal</DecalMode>
            <Interpolation>nearest</Interpolation>
        </TextureMap>
    </Textures>
"""
        uv = np.stack([(np.arange(len(verts)) % 7) / 8.0, (np.arange(len(verts)) % 5) / 4.0], 1)
        texcoords = "    <TexCoordData>\n        " + "\n        ".join(_g(r) for r in uv) + "\n    </TexCoordData>\n"
    vdata = "\n        ".join(_g(r) for r in verts)
    xml = f"""<Scene>
    <MaxRecursionDepth>0</MaxRecursionDepth>
    <BackgroundColor>10 20 30</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>{_g(cam)}</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>2</NearDistance>
            <ImageResolution>64 48</ImageResolution>
            <ImageName>{name}.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>{_g(light)}</Position><Intensity>{_g([power] * 3)}</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>0.8 0.7 0.6</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
    </Materials>
{textures}    <VertexData>
        {vdata}
    </VertexData>
{texcoords}{xform}    <Objects>
{chr(10).join(objects)}
    </Objects>
</Scene>
"""
    path = os.path.join(directory, name + ".xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def mesh_face_vertices(case):
    """Per mesh (nf, 3, 3) float32: the generated vertices of every face in parse order."""
    return [v[f] for v, f in case.meshes]


def check_round_trip(case, faces, meshes):
    """The description's face vertices (query_util.scene_arrays; a host-built description holds
    them in BVH order, so pass one loaded with device_bvh=True: parse order) equal the generated
    float32 bits."""
    assert len(meshes) == len(case.meshes)
    for m, want in zip(meshes, mesh_face_vertices(case)):
        F = faces[m["face_offset"]:m["face_offset"] + m["face_count"]]
        got = np.stack([F["v0"], F["v1"], F["v2"]], 1)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the loader changed a vertex"


def face_rays(world, owner):
    """One ray per world-space face (edge_rays.world_faces): from the centroid pushed out along the
    normal by 2^-10 of the longest edge, aimed straight back.  Returns (origins, directions) float32;
    computed in float64 and rounded once."""
    w = world.astype(np.float64)
    c = w.sum(1) / 3.0
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        edge = np.max([np.linalg.norm(w[:, a] - w[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], 0)
    d = edge * 2.0 ** -10
    with np.errstate(over="ignore", invalid="ignore"):
        return (c + n * d[:, None]).astype(f32), (-n).astype(f32)
