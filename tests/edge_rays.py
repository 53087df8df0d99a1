"""Seeded edge rays for the ray queries (test_edge_rays_host.py, test_gpu_edge_rays.py and the
recipe of tests/golden/make_goldens.py): the rays on which the walks' fast decisions are not
"sure" and the division form has to answer.  A helper module like query_util.py, not a conftest.

    rays, labels = generate(hs)         # RAY_DTYPE array, int8 class per ray (CLASSES)

Every construction is done in float32 on the description's own objects, faces and BVH node
records, so the special values are exact: a zero is a zero, a box plane is that plane bit for bit.

  A axis       one or two direction components +0.0 / -0.0, origins in general position
  B plane      as A, and the origin coordinate on a zero axis equals a box plane of the description
               (object boxes, inner nodes, leaves, the FLT_MIN maxima, zero-thickness boxes): in
               the world frame for object boxes and the nodes of objects under the identity, and
               in the local frame of transformed objects (local_plane_rays), planes at exactly 0
               among them
  C vertex     rays at mesh vertices, edge midpoints and points shared by several faces: from
               general origins, axis-parallel, and with power-of-two direction components
  D surface    origins on a face (vertex, edge midpoint, centroid) and the same moved by
               n * ShadowRayEpsilon; directions over the hemisphere, in the face's plane, along -n
  E tmax       rays with a known host hit at t: tmax = t, its two neighbours, 0, -0, -1, the
               smallest subnormal, FLT_MAX, inf, NaN
  F magnitude  direction components at 2^-60 / 2^60 and one ulp either side, subnormal components,
               directions scaled by 2^-10 / 2^10, origins at 1e6, o * rcp(d) overflowing
  G nonfinite  a NaN or +-inf in one origin or direction component
"""
import ctypes

import numpy as np

import query_util as qu
import rtgpu

CLASSES = {"A": 0, "B": 1, "C": 2, "D": 3, "E": 4, "F": 5, "G": 6}
NAMES = {v: k for k, v in CLASSES.items()}
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("first", "<i4"), ("count", "<i4"),
                       ("pad0", "<i4")])
assert NODE_DTYPE.itemsize == 40
f32 = np.float32
FLT_MIN = np.finfo(f32).tiny
FLT_MAX = np.finfo(f32).max
DENORM_MIN = np.array([1], np.uint32).view(f32)[0]
TIME_MAX = f32(1.0) - f32(2.0 ** -24)
_IDENT = np.eye(4).reshape(-1)


def node_array(hs):
    """The description's BVH node records (mesh-local boxes) as a NumPy copy."""
    d = qu.Desc.from_address(hs.desc)
    return qu._array(d.nodes, d.num_nodes, NODE_DTYPE)


def shadow_epsilon(hs):
    return f32(qu.Desc.from_address(hs.desc).shadow_epsilon)


def world_faces(hs):
    """(v0, v1, v2) float32 (n, 3) of every mesh object's faces in world space (exact for identity
    and dyadic translations, rounded once otherwise) and the owning object per face."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    out, owner = [], []
    for k, ob in enumerate(objs):
        if ob["kind"] == qu.RTG_OBJ_SPHERE:
            continue
        m = meshes[ob["mesh"]]
        F = faces[m["face_offset"]:m["face_offset"] + m["face_count"]]
        M = ob["transform"].reshape(4, 4)
        v = np.stack([F["v0"], F["v1"], F["v2"]], 1).astype(np.float64)          # (n, 3, 3)
        w = v @ M[:3, :3].T + M[:3, 3]
        out.append(w.astype(f32))
        owner.append(np.full(len(F), k, np.int32))
    if not out:
        return np.zeros((0, 3, 3), f32), np.zeros(0, np.int32)
    return np.concatenate(out), np.concatenate(owner)


def box_planes(hs):
    """(axis, value) float32 planes of the description's boxes that a world ray meets unchanged:
    the boxes of objects and the node boxes of meshes under the identity transform (the node
    boxes of transformed objects are targeted in their own frame by local_plane_rays).  The
    FLT_MIN maxima among them get a share of class B of their own where a scene has any
    (`spheres`, `transforms_textures` and `synth_10k` have none in a world-frame box)."""
    _, objs, meshes, _ = qu.scene_arrays(hs)
    nodes = node_array(hs)
    boxes = []
    for ob in objs:
        if ob["kind"] == qu.RTG_OBJ_SPHERE:
            continue
        ident = np.array_equal(ob["inv_transform"], _IDENT)
        if ident or ob["kind"] == qu.RTG_OBJ_INSTANCE:
            boxes.append((ob["bbox_min"], ob["bbox_max"]))          # (an instance's box is a world box)
        if ident:
            m = meshes[ob["mesh"]]
            for nd in nodes[m["node_offset"]:m["node_offset"] + m["node_count"]]:
                boxes.append((nd["bmin"], nd["bmax"]))
    return [(np.asarray(a, f32), np.asarray(b, f32)) for a, b in boxes]


def host_local(ob, v, w):
    """The local_ray product of the host walk and the reference (matrix.hpp:56-81) on (n, 3)
    float32 rows: the row-major double inverse transform, accumulated left to right in double,
    narrowed to float32 -- signed zeros as they come out."""
    m = ob["inv_transform"]
    v = np.asarray(v, f32).astype(np.float64)
    rows = [((m[4 * r] * v[:, 0] + m[4 * r + 1] * v[:, 1]) + m[4 * r + 2] * v[:, 2]) + m[4 * r + 3] * np.float64(w)
            for r in range(3)]
    return np.stack(rows, 1).astype(f32)


def local_plane_rays(hs, rng, n=160):
    """Class B in the frame of transformed objects: world rays whose LOCAL origin coordinate on a
    +-0 LOCAL direction axis equals a plane of one of the object's node boxes -- a third of them a
    plane at exactly 0, where o * rcp(d) is 0 * inf = NaN and not an infinity.  Built in the
    local frame, pushed through the object's transform and kept only where host_local brings
    both values back bit for bit (always under dyadic translations; seldom under a rotation).
    Returns (origins, directions, object index per ray)."""
    _, objs, meshes, _ = qu.scene_arrays(hs)
    nodes = node_array(hs)
    cand = [k for k, ob in enumerate(objs) if ob["kind"] != qu.RTG_OBJ_SPHERE
            and not np.array_equal(ob["inv_transform"], _IDENT) and not np.any(ob["motion_blur"])]
    O, D, K = [], [], []
    for i in range(n if cand else 0):
        k = cand[i % len(cand)]
        ob = objs[k]
        m = meshes[ob["mesh"]]
        nd = nodes[m["node_offset"]:m["node_offset"] + m["node_count"]]
        M = ob["transform"].reshape(4, 4)
        lo_, hi_ = nd["bmin"].astype(f32), nd["bmax"].astype(f32)
        at0 = np.argwhere((lo_ == 0) | (hi_ == 0))              # (node, axis) with a plane at 0
        if i % 3 == 0 and len(at0):
            j, ax = at0[rng.integers(len(at0))]
            p = f32(0.0)
        else:
            j, ax = rng.integers(len(nd)), rng.integers(3)
            p = (lo_ if i % 2 else hi_)[j, ax]
        span = np.where(np.isfinite(hi_[j] - lo_[j]), hi_[j] - lo_[j], 0).astype(f32)
        L = (lo_[j] + span * rng.random(3).astype(f32)).astype(f32)
        L[ax] = p
        dl = _unit(rng, 1)[0]
        neg = (i // 2) % 2 == 1                                 # the axis' zero is -0
        if neg and i % 4 == 2:                                  # every other component negative too: the -0
            dl = -np.abs(dl)                                    # survives a product whose last term is -0
        others = [a for a in range(3) if a != ax]
        if i % 5 == 4:                                          # along a local axis
            dl[others[0]] = f32(-0.0) if neg else f32(0.0)
            dl[others[1]] = f32(-1.0) if neg or i % 10 == 4 else f32(1.0)
        dl[ax] = f32(-0.0) if neg else f32(0.0)
        if i % 8 < 6:                                           # start off the geometry, so that faces in
            L = (L - f32(2.0) * dl).astype(f32)                 # the plane's boxes are hit at t > 0
            L[ax] = p
        o = (M[:3, :3] @ L.astype(np.float64) + M[:3, 3]).astype(f32)
        d = dl if np.array_equal(M[:3, :3], np.eye(3)) else (M[:3, :3] @ dl.astype(np.float64)).astype(f32)
        back_o, back_d = host_local(ob, o[None], 1.0)[0], host_local(ob, d[None], 0.0)[0]
        if back_o[ax] == p and back_d[ax] == 0 and np.all(np.isfinite(o)):
            O.append(o), D.append(d), K.append(k)
    if not O:
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, np.int64)
    return np.stack(O), np.stack(D), np.array(K)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.astype(f32)


def _zero_axes(rng, n, d):
    """Direction rows with one or two components set to +0.0 or -0.0; returns the mask too."""
    d = d.copy()
    mask = np.zeros((n, 3), bool)
    for i in range(n):
        two = i % 2 == 1
        k = rng.permutation(3)[:2 if two else 1]
        mask[i, k] = True
        zero = f32(-0.0) if (i // 2) % 2 else f32(0.0)
        d[i, k] = zero
        if two:                                               # the third component: +-1 exactly
            j = [a for a in range(3) if a not in k][0]
            d[i, j] = f32(1.0) if d[i, j] >= 0 else f32(-1.0)
    return d, mask


def _times(rng, n):
    t = np.minimum(rng.random(n).astype(f32), TIME_MAX)
    t[0::7] = 0.0
    t[3::7] = TIME_MAX
    return t


def is_pow2_dir(rays):
    """Rays whose three direction components are all nonzero powers of two (the rays the
    rational check of test_edge_rays_host.py covers)."""
    d = qu.directions(rays)
    mant = d.view(np.uint32) & np.uint32(0x007FFFFF)
    expo = (d.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
    return ((mant == 0) & (expo > 0) & (expo < 255)).all(1)


def generate(hs, seed=20260, with_nonfinite=True):
    """(rays, labels) for a HostScene: about 2 048 rays, the classes of this module's docstring."""
    rng = np.random.default_rng(seed)
    _, objs, meshes, faces = qu.scene_arrays(hs)
    W, owner = world_faces(hs)
    eps = shadow_epsilon(hs)

    # the scene box: world vertices and sphere extents, in float32
    pts = [W.reshape(-1, 3)]
    for ob in objs[objs["kind"] == qu.RTG_OBJ_SPHERE]:
        c = (ob["transform"].reshape(4, 4) @ np.append(ob["center"].astype(np.float64), 1.0))[:3].astype(f32)
        pts += [(c - ob["radius"])[None], (c + ob["radius"])[None]]
    pts = np.concatenate(pts).astype(f32)
    lo, hi = pts.min(0), pts.max(0)
    pad = np.maximum((hi - lo) * f32(0.25), f32(0.5))
    lo, hi = (lo - pad).astype(f32), (hi + pad).astype(f32)

    def inside(n):
        return (lo + (hi - lo) * rng.random((n, 3)).astype(f32)).astype(f32)

    sets = []          # (class, origins, directions, tmax or None)

    def add(cls, o, d, tmax=None):
        o = np.asarray(o, f32).reshape(-1, 3)
        d = np.asarray(d, f32).reshape(-1, 3)
        assert o.shape == d.shape
        sets.append((cls, o, d, None if tmax is None else np.broadcast_to(np.asarray(tmax, f32), (len(o),))))

    # ---- A: axis ----------------------------------------------------------------------------
    nA = 256
    dA, _ = _zero_axes(rng, nA, _unit(rng, nA))
    add("A", inside(nA), dA)

    # ---- B: plane ---------------------------------------------------------------------------
    boxes = box_planes(hs)
    nB = 320
    oB, dB = inside(nB), _unit(rng, nB)
    dB, maskB = _zero_axes(rng, nB, dB)
    planeB = np.zeros(nB, f32)
    axisB = np.zeros(nB, np.int64)
    thin = [b for b in boxes if np.any(b[0] == b[1])]
    tiny = [b for b in boxes if np.any(b[1] == FLT_MIN)]        # the FLT_MIN maxima of the reference's build
    for i in range(nB if boxes else 0):
        in_thin = bool(thin) and i % 4 == 3
        on_tiny = bool(tiny) and i % 8 == 5
        pool = thin if in_thin else tiny if on_tiny else boxes
        bmin, bmax = pool[rng.integers(len(pool))]
        zero_axes = np.flatnonzero(maskB[i])
        k = zero_axes[0]
        if on_tiny:                                            # the zero axis is one with that maximum
            kt = np.flatnonzero(bmax == FLT_MIN)[0]
            if not maskB[i, kt]:
                dB[i, kt], dB[i, k] = dB[i, k], dB[i, kt]
                maskB[i, kt], maskB[i, k] = True, False
            k = kt
        if in_thin:                                            # lie inside a zero-thickness box
            flat = np.flatnonzero(bmin == bmax)
            k = flat[0]
            if not maskB[i, k]:                                # move the zero onto the flat axis
                dB[i, k], dB[i, zero_axes[0]] = dB[i, zero_axes[0]], dB[i, k]
                maskB[i, k], maskB[i, zero_axes[0]] = True, maskB[i, k]
        p = bmax[k] if on_tiny else (bmin if i % 2 else bmax)[k]
        if i % 3 == 0:                                         # start within the box's other extents
            span = np.where(np.isfinite(bmax - bmin), bmax - bmin, 0).astype(f32)
            oB[i] = (bmin + span * rng.random(3).astype(f32)).astype(f32)
        oB[i, k] = p
        planeB[i], axisB[i] = p, k
    rows = np.arange(nB)
    # by construction: (plane - o) == 0 and d == 0 on that axis, for the box the plane came from
    if boxes:
        assert np.all((planeB - oB[rows, axisB]) == 0) and np.all(dB[rows, axisB] == 0)
        add("B", oB, dB)
    # the same in the local frame of transformed objects (a generator of its own: the other
    # classes' rays do not depend on how many of these survive)
    oL, dL, _ = local_plane_rays(hs, np.random.default_rng(seed + 1))
    if len(oL):
        add("B", oL, dL)

    # ---- C: vertex / edge -------------------------------------------------------------------
    if len(W):
        verts, counts = np.unique(W.reshape(-1, 3), axis=0, return_counts=True)
        shared = verts[counts >= 2] if np.any(counts >= 2) else verts
        pick = rng.integers(len(W), size=64)
        mids = ((W[pick, 0] + W[pick, 1]) * f32(0.5)).astype(f32)
        mids2 = ((W[pick, 1] + W[pick, 2]) * f32(0.5)).astype(f32)
        targets = np.concatenate([verts[rng.integers(len(verts), size=48)], shared[rng.integers(len(shared), size=48)],
                                  mids[:32], mids2[:32]]).astype(f32)
        nT = len(targets)
        # general origins: the direction is the rounded difference, un-normalised and normalised
        o = inside(nT)
        d = (targets - o).astype(f32)
        add("C", o, d)
        ln = np.sqrt((d * d).sum(1, dtype=f32)).astype(f32)
        add("C", o[::2], (d[::2] / ln[::2, None]).astype(f32))
        # axis-parallel, from both sides, the two other components +0.0 / -0.0
        for side, step in ((1, f32(2.0)), (-1, f32(4.0))):
            t = targets[::2]
            k = rng.integers(3, size=len(t))
            o = t.copy()
            o[np.arange(len(t)), k] = (t[np.arange(len(t)), k] + f32(side) * step).astype(f32)
            d = np.full((len(t), 3), f32(0.0) if side > 0 else f32(-0.0), f32)
            d[np.arange(len(t)), k] = f32(-side)
            add("C", o, d)
        # power-of-two components, no zero: o = target - m d, exact on dyadic geometry
        t = targets
        e = rng.integers(-1, 2, size=(nT, 3))
        sgn = np.where(rng.random((nT, 3)) < 0.5, -1.0, 1.0)
        d = (sgn * np.exp2(e)).astype(f32)
        m = np.exp2(rng.integers(0, 3, size=nT)).astype(f32)
        add("C", (t - m[:, None] * d).astype(f32), d)

    # ---- D: surface origin ------------------------------------------------------------------
    if len(W):
        nF = 40
        pick = rng.integers(len(W), size=nF)
        v0, v1, v2 = W[pick, 0], W[pick, 1], W[pick, 2]
        nrm = np.cross((v1 - v0).astype(np.float64), (v2 - v0).astype(np.float64))
        nl = np.linalg.norm(nrm, axis=1, keepdims=True)
        nrm = (nrm / np.where(nl > 0, nl, 1)).astype(f32)
        ident = np.array([np.array_equal(objs[k]["inv_transform"], _IDENT) for k in owner[pick]])
        fidx = np.concatenate([np.arange(meshes[o_["mesh"]]["face_offset"],
                                         meshes[o_["mesh"]]["face_offset"] + meshes[o_["mesh"]]["face_count"])
                               for o_ in objs if o_["kind"] != qu.RTG_OBJ_SPHERE])
        nrm[ident] = faces["n"][fidx[pick[ident]]]              # the description's own normal where it is the world's
        starts = [v0, ((v0 + v1) * f32(0.5)).astype(f32), (((v0 + v1) + v2) / f32(3.0)).astype(f32)]
        starts += [(s + nrm * eps).astype(f32) for s in starts]
        e1, e2 = (v1 - v0).astype(f32), (v2 - v0).astype(f32)
        for j, s in enumerate(starts):
            h = _unit(rng, nF)
            flip = (h * nrm).sum(1) < 0
            h[flip] = -h[flip]
            add("D", s, h)                                     # over the hemisphere
            inpl = [e1, e2, (e1 + e2).astype(f32), (e1 - e2).astype(f32), -e1][j % 5]
            add("D", s[:nF // 2], inpl[:nF // 2])              # in the face's own plane
            add("D", s[nF // 2:], -nrm[nF // 2:])              # straight back

    # ---- F: magnitude -----------------------------------------------------------------------
    nb = 16
    specials = [f32(2.0 ** -60), np.nextafter(f32(2.0 ** -60), f32(0)), np.nextafter(f32(2.0 ** -60), f32(1)),
                f32(2.0 ** 60), np.nextafter(f32(2.0 ** 60), f32(0)), np.nextafter(f32(2.0 ** 60), f32(np.inf)),
                DENORM_MIN, f32(1e-40), f32(FLT_MIN)]
    for j, sv in enumerate(specials):
        o, d = inside(nb), _unit(rng, nb)
        k = rng.integers(3, size=nb)
        d[np.arange(nb), k] = np.where(np.arange(nb) % 2 == 0, sv, -sv).astype(f32)
        add("F", o, d)
    for sc in (f32(2.0 ** -10), f32(2.0 ** 10)):
        add("F", inside(nb), (_unit(rng, nb) * sc).astype(f32))
    far = inside(2 * nb)
    far[np.arange(2 * nb), rng.integers(3, size=2 * nb)] = np.where(np.arange(2 * nb) % 2 == 0, 1e6, -1e6).astype(f32)
    add("F", far, (inside(2 * nb) - far).astype(f32))
    o, d = inside(2 * nb), _unit(rng, 2 * nb)                   # o * rcp(d) overflows, d in the fast range
    k = rng.integers(3, size=2 * nb)
    o[np.arange(2 * nb), k] = np.where(np.arange(2 * nb) % 2 == 0, 2.0 ** 70, -(2.0 ** 70)).astype(f32)
    d[np.arange(2 * nb), k] = np.where(np.arange(2 * nb) % 4 < 2, 2.0 ** -60, -(2.0 ** -60)).astype(f32)
    add("F", o, d)

    # ---- G: non-finite ----------------------------------------------------------------------
    if with_nonfinite:
        for val in (f32(np.nan), f32(np.inf), f32(-np.inf)):
            for comp in range(6):
                o, d = inside(5), _unit(rng, 5)
                d[3], _ = _zero_axes(rng, 1, d[3:4])
                (o if comp < 3 else d)[:, comp % 3] = val
                add("G", o, d)

    # ---- E: tmax around known host hits -----------------------------------------------------
    base_o = np.concatenate([s[1] for s in sets if s[0] in "ACD"])
    base_d = np.concatenate([s[2] for s in sets if s[0] in "ACD"])
    probe = rtgpu.make_rays(base_o, base_d)
    hit = hs.trace(probe)
    good = np.flatnonzero((hit["object"] >= 0) & np.isfinite(hit["t"]) & (hit["t"] > 0))
    p2 = good[is_pow2_dir(probe[good])]
    chosen = np.concatenate([rng.permutation(good)[:24], rng.permutation(p2)[:12]]) if len(good) else good
    for i in chosen:
        t = f32(hit["t"][i])
        tm = np.array([t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf)), 0.0, -0.0, -1.0, DENORM_MIN,
                       FLT_MAX, np.inf, np.nan], f32)
        add("E", np.repeat(base_o[i][None], len(tm), 0), np.repeat(base_d[i][None], len(tm), 0), tm)

    order = sorted(range(len(sets)), key=lambda j: CLASSES[sets[j][0]])
    o = np.concatenate([sets[j][1] for j in order])
    d = np.concatenate([sets[j][2] for j in order])
    tmax = np.concatenate([np.full(len(sets[j][1]), np.inf, f32) if sets[j][3] is None else sets[j][3] for j in order])
    labels = np.concatenate([np.full(len(sets[j][1]), CLASSES[sets[j][0]], np.int8) for j in order])
    rays = np.zeros(len(o), rtgpu.RAY_DTYPE)
    rays["ox"], rays["oy"], rays["oz"] = o[:, 0], o[:, 1], o[:, 2]
    rays["dx"], rays["dy"], rays["dz"] = d[:, 0], d[:, 1], d[:, 2]
    rays["tmax"] = tmax
    rays["time"] = _times(rng, len(o))
    # a finite tmax on some rays of the other classes too (about a scene diagonal: hits and misses)
    diag = f32(np.linalg.norm((hi - lo).astype(np.float64)))
    cut = (labels != CLASSES["E"]) & (np.arange(len(o)) % 5 == 2)
    rays["tmax"][cut] = (diag * (f32(0.05) + f32(0.5) * rng.random(int(cut.sum())).astype(f32))).astype(f32)
    assert np.all((rays["time"] >= 0) & (rays["time"] < 1))
    return rays, labels
