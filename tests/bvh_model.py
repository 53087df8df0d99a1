"""An independent statement of the reference's mesh BVH build, for the BVH suites
(test_bvh_build_host.py, test_gpu_bvh_cases.py): face preparation (parser.cpp:579-747), the mesh
box (parser.cpp:1393-1468) and Mesh::ConstructBVH / RecursiveBVHBuild / RecomputeBoundingBox
(mesh.cpp:23-156) in NumPy float32 scalars and plain Python loops.  A helper module like
query_util.py, not a conftest; it shares no code with host_scene.cpp or rtg_bvh.hip.

    m = build(verts, faces)             # verts (nv, 3) float32, faces (nf, 3) int, 0-based
    m.nodes                             # NODE_DTYPE records in the reference's allocation order
    m.perm                              # final face order: perm[p] = parse-order face at position p
    m.patterns                          # node index -> tuple of bools (True: big, centroid >= split),
                                        # the input of that node's partition, in arrival order
    m.arrivals                          # node index -> the parse-order faces in that arrival order
    walk_records(m, node_base, face_off)  # (nodes (N, 8) float32, ext (N, 2) int32) of rtg_device.hpp

Ties are the reference's: std::min(a, b) is `b < a ? b : a` and std::max(a, b) is `a < b ? b : a`,
so of two equal values (+0.0 and -0.0) the FIRST argument is kept.  RecomputeBoundingBox calls
min(box, face): the first-seen zero stays.  The parser's mesh box calls min(face, box): the
last-seen zero wins.
"""
import numpy as np

f32 = np.float32
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("first", "<i4"), ("count", "<i4")])
LEAF_EXT = 0x7FFFFFFF
FLT_MIN = np.finfo(f32).tiny
FLT_MAX = np.finfo(f32).max


def std_min(a, b):
    """std::min on float32 arrays, component by component: b where b < a, else a."""
    return np.where(b < a, b, a)


def std_max(a, b):
    """std::max on float32 arrays, component by component: b where a < b, else a."""
    return np.where(a < b, b, a)


class Model:
    pass


def face_prep(verts, faces):
    """(centre, box min, box max) per face: (a + b + c) / 3.0f (parser.cpp:586-593) and
    min(min(a, b), c) / max(max(a, b), c) (parser.cpp:734-747), all float32."""
    verts = np.asarray(verts, f32)
    a, b, c = (verts[np.asarray(faces)[:, k]] for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        cen = ((a + b) + c) / f32(3.0)
    assert cen.dtype == f32
    return cen, std_min(std_min(a, b), c), std_max(std_max(a, b), c)


def mesh_box(fmn, fmx):
    """parser.cpp:1392-1394 and :1455-1461: max starts at FLT_MIN, min at FLT_MAX, and every face
    is folded in as min(face, box) / max(face, box)."""
    mn = np.full(3, FLT_MAX, f32)
    mx = np.full(3, FLT_MIN, f32)
    for i in range(len(fmn)):
        mn = std_min(fmn[i], mn)
        mx = std_max(fmx[i], mx)
    return mn, mx


def build(verts, faces):
    cen, fmn, fmx = face_prep(verts, faces)
    n = len(cen)
    assert n >= 1
    nodes = np.zeros(2 * n - 1, NODE_DTYPE)
    nodes["left"] = -1
    nodes["bmin"][0], nodes["bmax"][0] = mesh_box(fmn, fmx)
    nodes["first"][0], nodes["count"][0] = 0, n
    perm = list(range(n))
    patterns, arrivals = {}, {}
    next_free = 1
    todo = [0]                                  # a stack: left subtree completely, then right
    while todo:
        k = todo.pop()
        first, count = int(nodes["first"][k]), int(nodes["count"][k])
        if count < 2:
            continue
        bmin, bmax = nodes["bmin"][k], nodes["bmax"][k]
        with np.errstate(over="ignore", invalid="ignore"):
            ln = bmax - bmin                    # float32
            lenX, lenY, lenZ = ln[0], ln[1], ln[2]
            if lenX > lenY:
                axis = 0 if lenX > lenZ else 2
            else:
                axis = 1 if lenY > lenZ else 2
            split = bmin[axis] + ln[axis] * f32(0.5)
        assert split.dtype == f32
        arrivals[k] = tuple(perm[first:first + count])
        patterns[k] = tuple(not (cen[f, axis] < split) for f in arrivals[k])
        i, j = first, first + count - 1
        while i <= j:
            if cen[perm[i], axis] < split:
                i += 1
            else:
                perm[i], perm[j] = perm[j], perm[i]
                j -= 1
        left_count = i - first
        if left_count == 0 or left_count == count:
            continue                            # stays a leaf, in the order the loop left behind
        li, ri = next_free, next_free + 1
        next_free += 2
        nodes["first"][li], nodes["count"][li] = first, left_count
        nodes["first"][ri], nodes["count"][ri] = i, count - left_count
        nodes["left"][k] = li
        nodes["count"][k] = 0
        for c in (li, ri):
            mn = np.full(3, np.inf, f32)
            mx = np.full(3, -np.inf, f32)
            for p in range(int(nodes["first"][c]), int(nodes["first"][c]) + int(nodes["count"][c])):
                mn = std_min(mn, fmn[perm[p]])
                mx = std_max(mx, fmx[perm[p]])
            nodes["bmin"][c], nodes["bmax"][c] = mn, mx
        todo.append(ri)
        todo.append(li)
    m = Model()
    m.nodes = nodes[:next_free].copy()
    m.perm = np.array(perm, np.int32)
    m.patterns, m.arrivals = patterns, arrivals
    m.centres, m.face_min, m.face_max = cen, fmn, fmx
    return m


def walk_records(m, node_base=0, face_off=0):
    """The walk records of rtg_device.hpp for one mesh: pre-order (left subtree before right), the
    skip link, and the leaf word (first << 8) | count for first < 2^23 and count < 255, else
    LEAF_EXT with (first, count) in ext.  Returns (nodes (N, 8) float32, ext (N, 2) int32); inner
    nodes have leaf = -1 and ext = (-1, 0)."""
    N = m.nodes
    order, stack = [], [0]
    while stack:
        k = stack.pop()
        order.append(k)
        if N["left"][k] >= 0:
            stack.append(int(N["left"][k]) + 1)
            stack.append(int(N["left"][k]))
    size = np.ones(len(N), np.int64)
    for k in reversed(order):
        if N["left"][k] >= 0:
            size[k] = 1 + size[N["left"][k]] + size[N["left"][k] + 1]
    rec = np.zeros((len(N), 8), f32)
    words = rec.view(np.int32)
    ext = np.zeros((len(N), 2), np.int32)
    for at, k in enumerate(order):
        rec[at, 0:3] = N["bmin"][k]
        rec[at, 3:6] = N["bmax"][k]
        words[at, 6] = node_base + at + size[k]
        if N["left"][k] >= 0:
            words[at, 7] = -1
            ext[at] = (-1, 0)
        else:
            first, cnt = face_off + int(N["first"][k]), int(N["count"][k])
            words[at, 7] = (first << 8) | cnt if first < (1 << 23) and cnt < 255 else LEAF_EXT
            ext[at] = (first, cnt)
    return rec, ext


def tri_records(verts, faces, perm):
    """(F, 12) float32 face records in the final order: {v0, 0}, {v0 - v1, 0}, {v0 - v2, 0}
    (the matrixA columns of mesh.cpp:208-210)."""
    verts = np.asarray(verts, f32)
    F = np.asarray(faces)[np.asarray(perm)]
    v0, v1, v2 = verts[F[:, 0]], verts[F[:, 1]], verts[F[:, 2]]
    out = np.zeros((len(F), 12), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, 0:3], out[:, 4:7], out[:, 8:11] = v0, v0 - v1, v0 - v2
    return out


# ---- the partition alone ---------------------------------------------------------------------

def sequential_partition(big):
    """mesh.cpp:91-100 on a list of bools (True: the face goes right): the order the loop leaves
    behind, as source positions, and the left count."""
    pos = list(range(len(big)))
    i, j = 0, len(big) - 1
    while i <= j:
        if not big[pos[i]]:
            i += 1
        else:
            pos[i], pos[j] = pos[j], pos[i]
            j -= 1
    return pos, i


def closed_form_partition(big):
    """The closed form stated in rtg_bvh.hip's header, restated: destination of every source
    position, computed independently per position from prefix counts and two select tables."""
    n = len(big)
    S = n - sum(big)
    a = S + (1 if S < n and big[S] else 0)
    # R sequence: positions n-1, n-2, ..., a (R index m <-> position n-1-m)
    selL = [q for q in range(a) if big[q]]                       # k-th big of [0, a) -> q
    selR = [m for m in range(n - a) if not big[n - 1 - m]]       # j-th small of R -> R index
    dest = [None] * n
    for q in range(n):
        if q < a:
            if not big[q]:
                np_ = q
            else:
                k = sum(big[:q + 1])                             # bigs in [0, q]
                rank = selR[k - 2] + 1 if k >= 2 else 0
                np_ = n - 1 - rank
        elif big[q]:
            np_ = q - 1
        else:
            smalls = sum(1 for p in range(q, n) if not big[p])   # smalls in [q, n)
            np_ = selL[smalls - 1]
        dest[q] = np_
    out = [None] * n
    for q, d in enumerate(dest):
        assert out[d] is None, (big, dest)
        out[d] = q
    return out, S
