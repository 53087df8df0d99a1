"""A numpy MODEL of the leaf-exact closest-hit packet walk (csrc/rtg_walk.hpp: walk_bvh_packet_lx;
DESIGN.md §2 "Leaf-exact walks").  It models the device code and does not run it.

The lemma: in the reference's pre-order walk a ray tests the faces of leaf L iff L's own box passes
BoundingBox::doesIntersectWith at the minT the ray holds when pre-order reaches L -- parent boxes
contain their children's, the test is monotone in the box and in minT, and minT never rises.  So a
walk may take any decision at inner nodes that keeps every box the exact test keeps.

  1. precondition, on every fixture scene's node table: each child box lies inside its parent's,
     compared as float32 values;
  2. on three small fixtures, for the edge rays of edge_rays.py (the reference's own recorded set,
     every class, no ray left out) and seeded camera rays: the restated reference walk (object
     loop, instance boxes, spheres, motion-blur offsets; float32 operation by operation) returns
     HostScene.trace's (t, object, face) bit for bit, and so does the leaf-exact walk under every
     inner-node policy a lane can meet in a wave:
       own    the lane's own conservative value (slab_cons_pk on slab_cons_ray's constants) --
              or, off the fast path / |o inv| not finite / value NaN, its own exact decision;
              with the reciprocal correctly rounded and moved one ulp either way (v_rcp_f32's
              bits are not known: up to 1.5 ulp off, beyond its 1 ulp);
       all    every inner node descends (other lanes of the wave drag the lane everywhere);
       mixed  a seeded coin per (ray, inner node) ORed onto `own` (dragged through some subtrees).
"""
import glob
import os

import numpy as np
import pytest

import edge_rays as er
import oracle_bind as ob
import query_util as qu
import rtgpu

F = np.float32
SCENES = os.path.join(ob.GOLDEN, "scenes")
ALL_SCENES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SCENES, "*.xml")))
MODEL_SCENES = ["edge_lattice", "edge_roof", "transforms_textures"]
N_CAMERA = 1536

# --- constants of csrc/rtg_isect.hpp and csrc/rtg_walk.hpp
TINY = F(1e-30)
CONS_BIAS = F(2.0 ** -22)        # slab_cons_ray: e_k = 2^-22 |o_k inv_k|
CONS_REL = F(2.0 ** -20)         # slab_cons_pk: 1 - 2^-20; minTc = minT (1 + 2^-20)
CONS_OK = F(2.0 ** 100)          # SlabCons::ok
FAST_LO, FAST_HI = F(2.0 ** -60), F(2.0 ** 60)


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


def preorder(nd):
    """(order, skip, parent) of one mesh's node records: order[i] = record of pre-order position i,
    skip[i] = the position after i's subtree, parent[i] = position of i's parent (-1: root)."""
    order, skip, parent = [], [], []
    stack = [(0, -1)]
    while stack:
        k, p = stack.pop()
        if k < 0:                                   # close the subtree opened at position p
            skip[p] = len(order)
            continue
        pos = len(order)
        order.append(k)
        skip.append(-1)
        parent.append(p)
        stack.append((-1, pos))
        if nd["left"][k] >= 0:
            stack.append((int(nd["left"][k]) + 1, pos))
            stack.append((int(nd["left"][k]), pos))
    return np.array(order), np.array(skip), np.array(parent)


@pytest.mark.parametrize("name", ALL_SCENES)
def test_child_boxes_lie_inside_their_parents(name):
    hs = rtgpu.HostScene(name + ".xml")
    _, _, meshes, _ = qu.scene_arrays(hs)
    nodes = er.node_array(hs)
    n_pairs = 0
    for m in meshes:
        nd = nodes[m["node_offset"]:m["node_offset"] + m["node_count"]]
        if len(nd) == 0:
            continue
        order, skip, parent = preorder(nd)
        assert len(order) == len(nd) and skip[0] == len(nd)          # every record, once
        ch = np.flatnonzero(parent >= 0)
        lo, hi = nd["bmin"][order], nd["bmax"][order]
        assert lo.dtype == F and hi.dtype == F
        assert not np.isnan(lo).any() and not np.isnan(hi).any()
        assert np.all(lo[ch] >= lo[parent[ch]]) and np.all(hi[ch] <= hi[parent[ch]]), name
        n_pairs += len(ch)
    print(name, "child / parent pairs", n_pairs)


# ----------------------------------------------------------------------------- float32 restatements
def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def box_hit(lo, hi, o, d, minT):
    """BoundingBox::doesIntersectWith: true divisions, the x slab by comparison, y / z by fmin / fmax.
    lo / hi: (3,) box; o, d: (n, 3)."""
    with np.errstate(all="ignore"):
        t1 = ((lo - o) / d).astype(F)
        t2 = ((hi - o) / d).astype(F)
        swap = t1[:, 0] > t2[:, 0]
        tmin = np.where(swap, t2[:, 0], t1[:, 0])
        tmax = np.where(swap, t1[:, 0], t2[:, 0])
        for k in (1, 2):
            tmin = np.fmax(tmin, np.fmin(t1[:, k], t2[:, k]))
            tmax = np.fmin(tmax, np.fmax(t1[:, k], t2[:, k]))
        return (tmax > 0) & (tmax >= tmin) & (tmin < minT)


def cons_ray(o, d, shift):
    """slab_cons_ray + kc: (inv, a, b, usable); shift in {-1, 0, 1}: the reciprocal's ulp."""
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
        if shift:
            inv = np.nextafter(inv, F(np.inf) if shift > 0 else F(-np.inf)).astype(F)
        p = (o * inv).astype(F)
        e = np.copysign((CONS_BIAS * np.abs(p)).astype(F), inv).astype(F)
        a = (-p - e).astype(F)
        b = (-p + e).astype(F)
        ad = np.abs(d)
        fast = np.all((ad >= FAST_LO) & (ad <= FAST_HI), axis=1)
        ok = np.max(np.abs(p), axis=1) <= CONS_OK               # (NaN: false, as fmaxf(...) <= does)
        ok &= ~np.isnan(p).any(axis=1)
    return inv, a, b, fast & ok


def cons_value(lo, hi, inv, a, b, minTc):
    """slab_cons_pk (v_minimum3_f32: NaN-propagating)."""
    with np.errstate(all="ignore"):
        t1 = fma(lo, inv, a)
        t2 = fma(hi, inv, b)
        tmin = np.fmax(np.fmax(np.fmin(t1[:, 0], t2[:, 0]), np.fmin(t1[:, 1], t2[:, 1])), np.fmin(t1[:, 2], t2[:, 2]))
        tmax = np.fmin(np.fmin(np.fmax(t1[:, 0], t2[:, 0]), np.fmax(t1[:, 1], t2[:, 1])), np.fmax(t1[:, 2], t2[:, 2]))
        c1 = (tmax + TINY).astype(F)
        c2 = ((tmax - fma(tmin, F(1.0) - CONS_REL, -TINY)).astype(F) + TINY).astype(F)
        c3 = (minTc - tmin).astype(F)
        return np.minimum(np.minimum(c1, c2), c3)               # np.minimum propagates NaN


def det3(m00, m01, m02, m10, m11, m12, m20, m21, m22):
    first = m00 * (m11 * m22 - m12 * m21)
    second = m10 * (m02 * m21 - m01 * m22)
    third = m20 * (m01 * m12 - m11 * m02)
    return first + second + third


def face_hit(Fc, o, d, minT):
    """Mesh::IntersectFace on one face for (n,) rays: (accepted, t).  The early outs only skip work
    in the reference; as masks they give the same acceptance."""
    with np.errstate(all="ignore"):
        v0, v1, v2 = Fc["v0"], Fc["v1"], Fc["v2"]
        e1 = (v0 - v1).astype(F)
        e2 = (v0 - v2).astype(F)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        detA = det3(e1[0], e2[0], dx, e1[1], e2[1], dy, e1[2], e2[2], dz)
        sx, sy, sz = v0[0] - o[:, 0], v0[1] - o[:, 1], v0[2] - o[:, 2]
        beta = det3(sx, e2[0], dx, sy, e2[1], dy, sz, e2[2], dz) / detA
        gama = det3(e1[0], sx, dx, e1[1], sy, dy, e1[2], sz, dz) / detA
        t = det3(e1[0], e2[0], sx, e1[1], e2[1], sy, e1[2], e2[2], sz) / detA
        assert t.dtype == F and detA.dtype == F
        ok = (detA != 0) & ~(beta < 0) & ~((gama < 0) | (gama + beta > 1)) & (t > 0) & (t < minT)
    return ok, t


def sphere_hit(ob_, o, d, minT):
    with np.errstate(all="ignore"):
        oc = (o - ob_["center"]).astype(F)
        dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        r = F(ob_["radius"])
        c = dot(oc, oc) - (r * r)
        b = F(2) * dot(d, oc)
        a = dot(d, d)
        delta = b * b - (F(4) * a * c)
        neg = delta < 0
        delta = np.sqrt(delta)
        a = (2.0 * a.astype(np.float64)).astype(F)
        t1 = (-b + delta) / a
        t2 = (-b - delta) / a
        t = np.where(t1 < t2, np.where(t1 > 0, t1, t2), np.where(t2 < t1, np.where(t2 > 0, t2, t1), t2))
        assert t.dtype == F
        return ~neg & (t < minT) & (t > 0), t


class Mesh:
    def __init__(self, nd, faces):
        self.order, self.skip, _ = preorder(nd)
        self.lo, self.hi = nd["bmin"][self.order], nd["bmax"][self.order]
        self.leaf = nd["left"][self.order] < 0
        self.first, self.count = nd["first"][self.order], nd["count"][self.order]
        self.faces = faces


def walk(mesh, o, d, minT, policy, shift=0, rng=None):
    """One mesh's walk for (n,) local rays, the nodes in pre-order, a lane's state as masks.
    policy "ref": the reference (a failed box hides its subtree: `blocked` until its skip);
    "own" / "all" / "mixed": the leaf-exact walk -- no lane state beyond minT.
    Returns (minT, face) with face = -1 where no face was accepted."""
    n = len(o)
    minT = minT.copy()
    face = np.full(n, -1, np.int64)
    blocked = np.zeros(n, np.int64)                  # ref: the lane sits out positions below this
    if policy in ("own", "mixed"):
        inv, a, b, usable = cons_ray(o, d, shift)
    for i in range(len(mesh.order)):
        lo, hi = mesh.lo[i], mesh.hi[i]
        if policy == "ref":
            act = blocked <= i
            if not act.any():
                continue
            p = act & box_hit(lo, hi, o, d, minT)
            blocked = np.where(act & ~p, mesh.skip[i], blocked)
        elif not mesh.leaf[i]:
            # inner decisions move the wave, never a lane: nothing to record.  What the model checks
            # is that a lane's own conservative "no" is never wrong (own / mixed): below.
            if policy == "all":
                continue
            with np.errstate(all="ignore"):
                minTc = (minT * (F(1.0) + CONS_REL)).astype(F)
            cv = cons_value(lo, hi, inv, a, b, np.where(usable, minTc, F(np.nan)))
            exact = box_hit(lo, hi, o, d, minT)
            keep = np.where(np.isnan(cv), exact, cv > 0)
            if policy == "mixed":
                keep |= rng.random(n) < 0.5
            # a lane whose inner test fails may still be walked through the subtree by its wave;
            # where the WAVE is this lane alone the subtree is skipped: model that, the strictest case
            blocked = np.where((blocked <= i) & ~keep, mesh.skip[i], blocked)
            continue
        else:
            p = box_hit(lo, hi, o, d, minT)
            if policy != "all":
                p &= blocked <= i                    # a subtree the lane's own wave-of-one skipped
            if policy == "own":
                # (not what the device does -- a leaf takes the exact test alone -- but the same
                # property: a conservative "no" is never wrong, at a leaf box either)
                with np.errstate(all="ignore"):
                    minTc = (minT * (F(1.0) + CONS_REL)).astype(F)
                cv = cons_value(lo, hi, inv, a, b, np.where(usable, minTc, F(np.nan)))
                p &= np.isnan(cv) | (cv > 0)
        if mesh.leaf[i] and p.any():
            for f in range(int(mesh.first[i]), int(mesh.first[i]) + int(mesh.count[i])):
                ok, t = face_hit(mesh.faces[f], o, d, minT)
                ok &= p
                minT = np.where(ok, t, minT).astype(F)
                face = np.where(ok, f, face)
    return minT, face


def trace(hs, rays, policy, shift=0, seed=0):
    """IntersectObjects restated (host_query.cpp trace_one): (t, object, face)."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    nodes = er.node_array(hs)
    rng = np.random.default_rng(seed)
    o, d = qu.origins(rays).astype(F), qu.directions(rays).astype(F)
    time = rays["time"].astype(F)
    n = len(rays)
    minT = rays["tmax"].astype(F).copy()
    obj = np.full(n, -1, np.int64)
    face = np.full(n, -1, np.int64)
    cache = {}
    for k, ob_ in enumerate(objs):
        blur = bool(np.any(ob_["motion_blur"] != 0))          # (the flag is set for a nonzero vector)
        mbv = (ob_["motion_blur"][None, :] * time[:, None]).astype(F)

        def local(oo):
            lo_, ld_ = er.host_local(ob_, oo, 1.0), er.host_local(ob_, d, 0.0)
            return ((lo_ + mbv).astype(F) if blur else lo_), ld_

        if ob_["kind"] == qu.RTG_OBJ_SPHERE:
            lo_, ld_ = local(o)
            ok, t = sphere_hit(ob_, lo_, ld_, minT)
            minT = np.where(ok, t, minT).astype(F)
            obj = np.where(ok, k, obj)
            face = np.where(ok, -1, face)
            continue
        m = meshes[ob_["mesh"]]
        go = np.ones(n, bool)
        if ob_["kind"] == qu.RTG_OBJ_INSTANCE:
            wo = (o + mbv).astype(F) if blur else o
            go = box_hit(ob_["bbox_min"], ob_["bbox_max"], wo, d, minT)
            o = np.where(go[:, None], o, wo)                   # a miss leaves the offset on the ray
        lo_, ld_ = local(o)
        if ob_["kind"] == qu.RTG_OBJ_MESH:
            go &= box_hit(ob_["bbox_min"], ob_["bbox_max"], lo_, ld_, minT)
        if m["node_count"] <= 0 or not go.any():
            continue
        mi = int(ob_["mesh"])
        if mi not in cache:
            cache[mi] = Mesh(nodes[m["node_offset"]:m["node_offset"] + m["node_count"]],
                             faces[m["face_offset"]:m["face_offset"] + m["face_count"]])
        sel = np.flatnonzero(go)
        t, f = walk(cache[mi], lo_[sel], ld_[sel], minT[sel], policy, shift, rng)
        got = f >= 0
        minT[sel] = np.where(got, t, minT[sel])
        obj[sel] = np.where(got, k, obj[sel])
        face[sel] = np.where(got, m["face_offset"] + f, face[sel])
    return minT, obj, face


def model_rays(hs, name):
    z = np.load(os.path.join(ob.GOLDEN, f"edge_rays_{name}.npz"), allow_pickle=False)
    edge = z["rays"].view(rtgpu.RAY_DTYPE).reshape(-1).copy()
    labels = z["labels"]
    cam = qu.numpy_camera_rays(qu.camera_record(hs))
    pick = np.random.default_rng(12).permutation(len(cam))[:N_CAMERA]
    return np.concatenate([edge, cam[np.sort(pick)]]), labels


@pytest.fixture(scope="module", params=MODEL_SCENES)
def case(request):
    """The scene, its rays and the two shared references, computed once."""
    name = request.param
    hs = rtgpu.HostScene(name + ".xml")
    rays, labels = model_rays(hs, name)
    assert set(np.unique(labels)) == set(er.NAMES), name             # every edge class, none left out
    host = hs.trace(rays)
    ref = trace(hs, rays, "ref")
    for a in (rays, host) + ref:
        a.setflags(write=False)
    return name, hs, rays, host, ref


def _same(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2], b[2]))


def test_restated_reference_is_the_host_walk(case):
    name, hs, rays, host, ref = case
    hits = int((ref[1] >= 0).sum())
    print(name, "rays", len(rays), "hits", hits)
    assert 0 < hits < len(rays)
    assert np.array_equal(ref[0].view(np.uint32), host["t"].view(np.uint32))
    assert np.array_equal(ref[1], host["object"])
    assert np.array_equal(ref[2], host["face"])


@pytest.mark.parametrize("policy,shift", [("own", 0), ("own", 1), ("own", -1), ("all", 0), ("mixed", 0)])
def test_leaf_exact_walk_is_the_reference_walk(case, policy, shift):
    name, hs, rays, host, ref = case
    got = trace(hs, rays, policy, shift, seed=5)
    bad = np.flatnonzero((got[0].view(np.uint32) != ref[0].view(np.uint32)) | (got[1] != ref[1]) | (got[2] != ref[2]))
    assert bad.size == 0, (name, policy, shift, bad[:8], rays[bad[:4]], [g[bad[:4]] for g in got], [r[bad[:4]] for r in ref])
    assert _same(got, ref)
