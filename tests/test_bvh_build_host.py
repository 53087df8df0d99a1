"""The host BVH build (Loader::constructBVH, host_scene.cpp) on the adversarial meshes of
bvh_cases.py, pinned three ways, bit for bit and without a tolerance anywhere:

  * to bvh_model.py, an independent NumPy statement of mesh.cpp:23-156 and parser.cpp:579-747;
  * to the reference's own answer, tests/golden/bvh_<case>.npz (make_goldens.py `bvh`: refdriver
    bvh, run twice) -- node boxes, child indices, firstFace, faceCount and the final face order;
  * and the model to that recorded answer directly.

Cases dropped from the goldens because the reference crashed or differed between two runs: none
(bvh_manifest.json lists them; the test fails if a case is neither recorded nor listed there).

The closed form that rtg_bvh.hip's header states for the reference's swap loop is checked here as
well, restated in Python (bvh_model.closed_form_partition), against the sequential loop on every
big / small pattern of length <= 12.
"""
import itertools
import json
import os

import numpy as np
import pytest

import bvh_cases as bc
import bvh_model as bm
import edge_rays as er
import oracle_bind as ob
import query_util as qu
import rtgpu

with open(os.path.join(ob.GOLDEN, "bvh_manifest.json")) as _f:
    MANIFEST = json.load(_f)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load_golden(name):
    z = np.load(os.path.join(ob.GOLDEN, f"bvh_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture()
def scene(tmp_path, request):
    """The case's scene written to a temp directory, loaded with and without the host build."""
    name = request.param
    case = bc.get(name)
    bc.write_scene(case, str(tmp_path), name)
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        yield name, case, rtgpu.HostScene(name + ".xml"), rtgpu.HostScene(name + ".xml", device_bvh=True)
    finally:
        os.chdir(old)


def test_every_case_is_recorded_or_named():
    assert set(MANIFEST["cases"]) | set(MANIFEST["dropped"]) == set(bc.NAMES)
    assert not set(MANIFEST["cases"]) & set(MANIFEST["dropped"])
    for name in MANIFEST["cases"]:
        assert os.path.getsize(os.path.join(ob.GOLDEN, f"bvh_{name}.npz")) <= 256 * 1024


def test_min_max_ties_are_the_references():
    """std::min / std::max keep their first argument on a tie: the model's own two helpers."""
    pz, nz = np.array([0.0], np.float32), np.array([-0.0], np.float32)
    assert not np.signbit(bm.std_min(pz, nz))[0] and np.signbit(bm.std_min(nz, pz))[0]
    assert not np.signbit(bm.std_max(pz, nz))[0] and np.signbit(bm.std_max(nz, pz))[0]
    one, two = np.array([1.0], np.float32), np.array([2.0], np.float32)
    assert bm.std_min(two, one)[0] == 1 and bm.std_min(one, two)[0] == 1
    assert bm.std_max(two, one)[0] == 2 and bm.std_max(one, two)[0] == 2


def test_closed_form_equals_swap_loop():
    """Every pattern of length 1..12 (8190 of them): the closed form of rtg_bvh.hip's header
    leaves the faces where mesh.cpp:91-100 does, and reports the same left count."""
    n = 0
    for length in range(1, 13):
        for big in itertools.product((False, True), repeat=length):
            assert bm.closed_form_partition(big) == bm.sequential_partition(big), big
            n += 1
    assert n == 2 ** 13 - 2


def test_lattice_feeds_every_pattern():
    """A3's coverage, as a condition: by the model, each of the 494 big / small patterns of length
    2..8 with both halves non-empty is the input of some node's partition."""
    v, f = bc.get("lattice").meshes[0]
    assert len(f) == 3514
    wanted = bc.lattice_patterns()
    assert len(wanted) == 494 and len(set(wanted)) == 494
    fed = set(bm.build(v, f).patterns.values())
    assert not set(wanted) - fed


@pytest.mark.parametrize("scene", bc.NAMES, indirect=True)
def test_host_build_equals_model_and_reference(scene):
    name, case, hs, hd = scene
    # the generated float32 bits reach the description unchanged (parse order: the deferred load)
    _, _, meshes_d, faces_d = qu.scene_arrays(hd)
    bc.check_round_trip(case, faces_d, meshes_d)
    assert hd.counts()["nodes"] == 0

    _, _, meshes, faces = qu.scene_arrays(hs)
    nodes = er.node_array(hs)
    assert len(meshes) == len(case.meshes)
    recorded = name in MANIFEST["cases"]
    assert recorded or name in MANIFEST["dropped"]
    gold = load_golden(name) if recorded else None
    if recorded:
        assert str(gold["sha256"]) == case.vertex_sha256() == MANIFEST["cases"][name]["sha256"], \
            "the generator drifted: record the goldens again (make_goldens.py bvh)"
    base = 0                                             # vertex ids are 1-based into the shared list
    for k, (v, f) in enumerate(case.meshes):
        M = meshes[k]
        N = nodes[M["node_offset"]:M["node_offset"] + M["node_count"]]
        F = faces[M["face_offset"]:M["face_offset"] + M["face_count"]]
        host_faces = np.stack([F["v0"], F["v1"], F["v2"]], 1)
        m = bm.build(v, f)

        # host build == model
        assert len(N) == len(m.nodes), (name, k, len(N), len(m.nodes))
        for field in ("left", "first", "count"):
            assert np.array_equal(N[field], m.nodes[field]), (name, k, field)
        assert np.array_equal(_bits(N["bmin"]), _bits(m.nodes["bmin"])), (name, k)
        assert np.array_equal(_bits(N["bmax"]), _bits(m.nodes["bmax"])), (name, k)
        assert np.array_equal(_bits(host_faces), _bits(v[f[m.perm]])), (name, k, "face order")

        if recorded:
            gn, gf = gold[f"nodes{k}"], gold[f"faces{k}"]
            ref_box = gn[:, :6].view(np.uint32)
            ref_faces = np.concatenate([vv for vv, _ in case.meshes])[gf[:, 3:6] - 1]
            for who, box, left, first, count, order, centres in (
                    ("host", np.concatenate([_bits(N["bmin"]), _bits(N["bmax"])], 1), N["left"], N["first"],
                     N["count"], host_faces, None),
                    ("model", np.concatenate([_bits(m.nodes["bmin"]), _bits(m.nodes["bmax"])], 1), m.nodes["left"],
                     m.nodes["first"], m.nodes["count"], v[f[m.perm]], m.centres[m.perm])):
                assert len(box) == len(gn), (name, k, who)
                assert np.array_equal(box, ref_box), (name, k, who, "boxes")
                assert np.array_equal(left, gn[:, 6]), (name, k, who, "left")
                # (an inner node's firstFace stays what it was; its faceCount is zeroed: mesh.cpp:125)
                assert np.array_equal(first, gn[:, 7]) and np.array_equal(count, gn[:, 8]), (name, k, who)
                assert np.array_equal(_bits(order), _bits(ref_faces)), (name, k, who, "face order")
                if centres is not None:
                    assert np.array_equal(_bits(centres), gf[:, :3].view(np.uint32)), (name, k, "centres")
            # and the ids themselves where faces differ: the reference's final order as parse-order faces
            if name not in bc.COINCIDENT:
                assert np.array_equal(gf[:, 3:6] - 1 - base, f[m.perm]), (name, k, "vertex ids")
        base += len(v)
