"""The shadow rays' any-hit trees (rtg_ahb.cpp), built on the host exactly as rtg_scene_create
builds them, checked structurally on every fixture scene in the three modes (0: the reference's
BVH collapsed, 1: the default, binned SAH over its leaves, 2: opt-in, large leaves split into single
faces): every face of a mesh reached by exactly one leaf entry naming its reference leaf, child
boxes nested in their parent slot's box, every entry's triangle inside its leaf slot's box
(rtg_desc_anyhit_check).  The traversal answer against the reference walk is the GPU test
tests/test_gpu_shadow.py."""
import os

import pytest

import bvh_cases as bc
import oracle_bind as ob
import rtgpu
import walk_cases as wc

SCENES = os.path.join(ob.GOLDEN, "scenes")
NAMES = sorted(ob.manifest())


@pytest.fixture(scope="module", autouse=True)
def _cwd():
    old = os.getcwd()
    os.chdir(SCENES)
    yield
    os.chdir(old)


@pytest.mark.parametrize("name", NAMES + bc.NAMES + list(wc.WALK_ONLY))
def test_anyhit_tree_structure(name, tmp_path):
    """Every fixture scene, every adversarial mesh of bvh_cases.py (coincident copies, where the
    centroids' extent is 0 and the builder halves by count; 300 faces in one reference leaf,
    chunked 255 + 45; huge_*, whose box areas reach 1e77) and the walk-only cases of walk_cases.py.

    The size comparison (the default tree no larger than the collapsed reference, in wide nodes)
    is what anyhit_trees' fall-back (scene_tables.cpp) is for: the binned SAH alone gave lattice /
    lattice_uv 353 wide nodes against 341, pinwheel_49152 5 462 against 5 461 and
    pinwheel_49152_blocked 7 707 against 5 464; a scene on which the SAH loses takes the
    reference's topology."""
    if name in NAMES:
        hs = rtgpu.HostScene(name + ".xml")
    else:
        hs = wc.load(tmp_path, name)
    faces = hs.counts()["faces"]
    res = [hs.anyhit_check(mode) for mode in (0, 1, 2)]
    for mode, r in enumerate(res):
        assert r["built"] == 1 and r["violations"] == 0, (mode, r)
        assert r["entries"] == faces, (mode, r)
    # only mode 2 splits leaves; the SAH trees are no larger than the collapsed reference
    assert res[0]["face_prims"] == res[1]["face_prims"] == 0
    assert res[1]["nodes"] <= res[0]["nodes"], (res[1]["nodes"], res[0]["nodes"])


def test_anyhit_splits_pole_fans():
    """ton_Roosendaal's mesh has the reference's large leaves (pole fans): split into faces,
    their slivers (kappa > 64) kept on their leaf box."""
    hs = rtgpu.HostScene("ton_roosendaal.xml")
    r = hs.anyhit_check(2)
    assert r["face_prims"] > 1000 and 0 < r["exact_faces"] < r["face_prims"] and r["violations"] == 0


def test_anyhit_headline_size(tmp_path):
    import scenes
    xml = scenes.synthetic_heightfield(str(tmp_path), K=100352)
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        hs = rtgpu.HostScene(xml)
        r = hs.anyhit_check(2)
    finally:
        os.chdir(old)
    assert r["built"] == 1 and r["violations"] == 0 and r["entries"] == 100352
