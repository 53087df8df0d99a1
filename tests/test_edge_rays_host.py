"""The host walk (rtg_desc_trace_rays, HostScene.trace) on the edge rays of edge_rays.py, against
the reference's own answers: tests/golden/edge_rays_<scene>.npz holds the rays, their class and
what the reference's Shape::Intersect loops returned for them (make_goldens.py `edge_rays`:
refdriver rays, run twice).  Zero disagreements, no grazing exclusions: here the host walk is
compared with the reference's own float32 arithmetic, not with float64.

objects[] of a description is in the reference's loop order (scene.meshes -- meshes, light meshes,
instances and triangles, all Shapes of that one list --, then scene.spheres; scene.triangles stays
empty), so the golden's loop position is the object index as it stands.

Classes dropped because two runs of the reference differed: none.  Class G (non-finite rays): the
reference returns on all of them, so it is stored.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import edge_rays as er
import oracle_bind as ob
import query_util as qu
import rtgpu
import walk_cases as wc

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = ["simple", "spheres", "transforms_textures", "cornell_dielectric", "mesh_light", "dof_motion", "edge_lattice",
         "edge_roof"]


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def load_golden(name):
    z = np.load(os.path.join(ob.GOLDEN, f"edge_rays_{name}.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["rays"] = g["rays"].view(rtgpu.RAY_DTYPE).reshape(-1)
    for a in g.values():
        a.setflags(write=False)
    return g


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_reference(name):
    g = load_golden(name)
    rays, labels = g["rays"], g["labels"]
    assert rays.size >= 1500 and rays.size == labels.size
    hs = rtgpu.HostScene(name + ".xml")
    hits = hs.trace(rays)
    occ = hs.trace(rays, any_hit=True)["object"]
    ref_hit = g["has_hit"] != 0
    # the reference's own bookkeeping: a miss keeps tmax, a hit names a shape of the lists
    tmax_bits = rays["tmax"].view(np.uint32)
    assert np.array_equal(g["t_bits"][~ref_hit], tmax_bits[~ref_hit])
    assert np.all(g["position"][ref_hit] >= 0) and np.all(g["position"][~ref_hit] == -1)

    print(f"{name}: class  rays  hits  misses  occluded")
    for c in sorted(er.NAMES):
        s = labels == c
        nh, no = int(ref_hit[s].sum()), int((g["occluded"][s] != 0).sum())
        print(f"{name}:   {er.NAMES[c]}   {int(s.sum()):5d} {nh:5d} {int(s.sum()) - nh:6d} {no:8d}")
        assert s.sum() > 0, (name, er.NAMES[c])
        assert nh < s.sum(), (name, er.NAMES[c], "no miss")
        # a NaN or an infinity in the ray makes every acceptance of the reference false on these
        # scenes (class G cannot produce a hit); every other class must hold hits too
        if er.NAMES[c] != "G":
            assert nh > 0, (name, er.NAMES[c], "no hit")

    if name in ("edge_lattice", "edge_roof"):
        # class B also in the translated instance's frame: local origin coordinate exactly 0 (where
        # o * rcp(d) is NaN, not an infinity) on a +-0 local axis, -0 among them
        _, objs, _, _ = qu.scene_arrays(hs)
        inst = objs[objs["kind"] == qu.RTG_OBJ_INSTANCE][0]
        B = rays[labels == er.CLASSES["B"]]
        lo, ld = er.host_local(inst, qu.origins(B), 1.0), er.host_local(inst, qu.directions(B), 0.0)
        zero = (lo == 0) & (ld == 0)
        minus = zero & np.signbit(ld)
        print(name, "class B rays with a local 0 / +-0 axis under the instance:", int(zero.any(1).sum()),
              "of them -0:", int(minus.any(1).sum()))
        assert zero.any(1).sum() >= 32 and minus.any(1).sum() >= 8

    wc.check_host_equals_reference(name, rays, labels, g, hits, occ)


def _det3(c0, c1, c2):
    """Determinant of the matrices with columns c0, c1, c2 ((n, 3) integer arrays)."""
    return (c0[:, 0] * (c1[:, 1] * c2[:, 2] - c2[:, 1] * c1[:, 2])
            + c0[:, 1] * (c2[:, 0] * c1[:, 2] - c1[:, 0] * c2[:, 2])
            + c0[:, 2] * (c1[:, 0] * c2[:, 1] - c1[:, 1] * c2[:, 0]))


def test_lattice_exact_rational():
    """`edge_lattice`: classes C and E restricted to rays whose direction components are all
    nonzero powers of two.  Geometry, origins and directions are dyadic with a few bits, so every
    float32 operation of IntersectFace on them is exact (detA = +-d.z on faces in a z plane: a
    power of two), and the answer can be had in exact rational arithmetic: all coordinates times
    4 are integers (determinants as Python integers, no rounding), t and its comparison with
    tmax as fractions.Fraction.  Predicate: detA != 0, beta >= 0, gamma >= 0, beta + gamma <= 1,
    0 < t < tmax.  Rays whose exact discriminant on the sphere is >= 0 are left out (the check
    is over the faces); that is decided in integers too, not by the walk under test."""
    g = load_golden("edge_lattice")
    rays, labels = g["rays"], g["labels"]
    hs = rtgpu.HostScene("edge_lattice.xml")
    _, objs, meshes, _ = qu.scene_arrays(hs)
    W, owner = er.world_faces(hs)
    sel = np.flatnonzero(er.is_pow2_dir(rays) & ((labels == er.CLASSES["C"]) | (labels == er.CLASSES["E"])))
    assert sel.size >= 100
    S = 4

    def ints(a):
        v = np.asarray(a, np.float64) * S
        assert np.array_equal(v, np.round(v)) and np.all(np.abs(v) < 2 ** 20)
        return v.astype(np.int64).astype(object)                # Python integers: no overflow

    v0, v1, v2 = ints(W[:, 0]), ints(W[:, 1]), ints(W[:, 2])
    e1, e2 = v0 - v1, v0 - v2
    sph = objs[objs["kind"] == qu.RTG_OBJ_SPHERE]
    assert len(sph) == 1 and np.array_equal(sph[0]["inv_transform"], np.eye(4).reshape(-1))
    cen, rad = ints(sph[0]["center"]), int(float(sph[0]["radius"]) * S)
    first_face = {}
    off = 0
    for k, ob_ in enumerate(objs):
        if ob_["kind"] != qu.RTG_OBJ_SPHERE:
            first_face[k] = (off, meshes[ob_["mesh"]]["face_offset"])
            off += meshes[ob_["mesh"]]["face_count"]
    hits = hs.trace(rays[sel])
    checked = n_hit = n_tie = 0
    for j, i in enumerate(sel):
        o = ints(qu.origins(rays[i:i + 1])[0])
        d = ints(qu.directions(rays[i:i + 1])[0])
        oc = o - cen
        a_, b_, c_ = int(d @ d), 2 * int(d @ oc), int(oc @ oc) - rad * rad
        if b_ * b_ - 4 * a_ * c_ >= 0:
            continue
        n = len(W)
        dd = np.broadcast_to(d, (n, 3))
        s = v0 - o
        D = _det3(e1, e2, dd)
        nb, ng, nt = _det3(s, e2, dd), _det3(e1, s, dd), _det3(e1, e2, s)
        tmax = float(rays["tmax"][i])
        best, tied = None, []
        for f in range(n):
            Df = D[f]
            if Df == 0:
                continue
            sg = 1 if Df > 0 else -1
            if nb[f] * sg < 0 or ng[f] * sg < 0 or (nb[f] + ng[f]) * sg > Df * sg or nt[f] * sg <= 0:
                continue
            t = Fraction(int(nt[f]), int(Df))                   # (d scaled like the points: t is unscaled)
            if np.isnan(tmax) or not (np.isinf(tmax) and tmax > 0 or t < Fraction(tmax)):
                continue
            if best is None or t < best:
                best, tied = t, [f]
            elif t == best:
                tied.append(f)
        h = hits[j]
        checked += 1
        if best is None:
            assert h["object"] == -1, (int(i), rays[i], h)
            continue
        n_hit += 1
        n_tie += len(tied) > 1
        assert h["object"] >= 0, (int(i), rays[i], h, float(best))
        assert Fraction(float(h["t"])) == best, (int(i), rays[i], h, float(best))
        assert int(h["object"]) in first_face, (int(i), h)
        w0, f0 = first_face[int(h["object"])]
        assert w0 + int(h["face"]) - int(f0) in tied, (int(i), rays[i], h, tied)
    print("edge_lattice exact: rays", checked, "of", sel.size, "hits", n_hit, "with tied faces", n_tie)
    assert checked >= sel.size // 2 and 0 < n_hit < checked and n_tie > 0
