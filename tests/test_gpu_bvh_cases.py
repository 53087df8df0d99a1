"""The device BVH build (rtg_bvh.hip) on the adversarial meshes of bvh_cases.py: its closed-form
partition (k_select / k_permute), its keyed child-box reduction (k_child_box /
k_child_box_final), the leaf word at 254 / 255 / 256 faces, one- and two-face meshes, a
92-level chain, signed zeros, overflowing and subnormal boxes, several meshes in one scene.

For every case, HostScene(xml) against HostScene(xml, device_bvh=True), everything as bits and
nothing with a tolerance:

  * the device build's walk records equal the host build's;
  * the device build's walk records equal bvh_model.walk_records -- the independent NumPy
    statement of mesh.cpp:23-156 --, so the check does not pass through the host build;
  * one ray per face (from just above its centroid, straight back at it) through trace(normals=True)
    and surface() gives identical t, object, face, n, ng, u, v, material and kd on both scenes:
    what reaches node_ext (the big leaves), face_n, face_uv and face_v12 in the device-built order;
  * a 64 x 48 render with traversal counters gives identical pixels and counters.

Every face must be its own ray's hit in the host-built scene, with two stated exceptions: in the
copies_<n> cases the copies coincide, and the first of them in the final order answers every ray;
in huge_empty, huge_split and subnormal the face test's own determinants overflow or underflow
(differences near 1e36, or subnormal), so no face can be hit by any ray -- there the answers are
only required to be the same bits on both scenes.
"""
import os

import numpy as np
import pytest

import bvh_cases as bc
import bvh_model as bm
import edge_rays as er
import query_util as qu
import rtgpu

pytestmark = pytest.mark.gpu


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _load(tmp_path, name):
    case = bc.get(name)
    bc.write_scene(case, str(tmp_path), name)
    host = rtgpu.HostScene(name + ".xml")
    dev = rtgpu.HostScene(name + ".xml", device_bvh=True)
    assert dev.counts()["nodes"] == 0 and dev.counts()["faces"] == host.counts()["faces"]
    return case, host, dev


@pytest.fixture(autouse=True)
def _cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield
    os.chdir(old)


def model_records(case):
    """The walk records of the whole scene by the model: every mesh at its node base and face
    offset, then the zeroed pad node."""
    nodes, tris, base, off = [], [], 0, 0
    for v, f in case.meshes:
        m = bm.build(v, f)
        rec, _ = bm.walk_records(m, base, off)
        nodes.append(rec)
        tris.append(bm.tri_records(v, f, m.perm))
        base += len(rec)
        off += len(f)
    nodes.append(np.zeros((1, 8), np.float32))
    return np.concatenate(nodes), np.concatenate(tris)


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_build_equals_host_and_model(tmp_path, name):
    case, hs, hd = _load(tmp_path, name)
    _, _, meshes, faces = qu.scene_arrays(hd)
    bc.check_round_trip(case, faces, meshes)
    ds_h, ds_d = rtgpu.DeviceScene(hs, 0), rtgpu.DeviceScene(hd, 0)

    # ---- the records: device == host, device == model ---------------------------------------
    nh, th = ds_h.export_bvh()
    nd, td = ds_d.export_bvh()
    nm, tm = model_records(case)
    print(name, nd.shape[0], "nodes", td.shape[0], "faces")
    assert nd.shape == nh.shape == nm.shape and td.shape == th.shape == tm.shape, (nd.shape, nh.shape, nm.shape)
    assert np.array_equal(_u32(nd), _u32(nh)), "device-built nodes differ from the host build"
    assert np.array_equal(_u32(td), _u32(th)), "device-built face records differ from the host build"
    assert np.array_equal(_u32(nd), _u32(nm)), "device-built nodes differ from the model"
    assert np.array_equal(_u32(td), _u32(tm)), "device-built face records differ from the model"

    # ---- one ray per face -------------------------------------------------------------------
    W, owner = er.world_faces(hs)
    o, d = bc.face_rays(W, owner)
    rays = rtgpu.make_rays(o, d)
    hits_h, nrm_h = ds_h.trace(rays, normals=True)
    hits_d, nrm_d = ds_d.trace(rays, normals=True)
    sur_h, sur_d = ds_h.surface(rays), ds_d.surface(rays)
    assert hits_h.tobytes() == hits_d.tobytes()
    assert np.array_equal(_u32(nrm_h), _u32(nrm_d))
    for field in sur_h.dtype.names:
        assert np.array_equal(_u32(sur_h[field]), _u32(sur_d[field])), (name, field)
    assert np.array_equal(sur_h["face"], hits_h["face"]) and np.array_equal(sur_h["object"], hits_h["object"])
    hit = hits_h["object"] >= 0
    pairs = set(zip(hits_h["object"][hit].tolist(), hits_h["face"][hit].tolist()))
    if name in bc.COINCIDENT:
        # the copies coincide: every ray is answered by the first copy in the final order
        assert hit.all() and pairs == {(0, 0)}
    elif name not in bc.UNHITTABLE:
        assert hit.all() and np.array_equal(hits_h["object"], owner)
        assert len(pairs) == len(rays), "some face is no ray's hit"
    if case.uv:
        assert np.any(sur_h["u"][hit] != 0) and np.any(sur_h["n"][hit] != sur_h["ng"][hit])   # the map is in effect

    # ---- a small render with counters -------------------------------------------------------
    ds_h.reset_stats()
    ds_d.reset_stats()
    a, _ = ds_h.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS, seed=7)
    b, _ = ds_d.render(0, flags=rtgpu.RTG_RENDER_COUNT_STATS, seed=7)
    assert a.shape[:2] == (48, 64)
    assert np.array_equal(_u32(a), _u32(b))
    assert ds_h.stats() == ds_d.stats()


def test_several_meshes_built_twice(tmp_path):
    """Non-zero face offsets and node bases, twice in one process: the same records both times."""
    case, hs, hd = _load(tmp_path, "several")
    first = rtgpu.DeviceScene(hd, 0)
    second = rtgpu.DeviceScene(hd, 0)
    n1, t1 = first.export_bvh()
    first.close()
    third = rtgpu.DeviceScene(hd, 0)
    nm, tm = model_records(case)
    for ds in (second, third):
        n, t = ds.export_bvh()
        assert np.array_equal(_u32(n), _u32(n1)) and np.array_equal(_u32(t), _u32(t1))
        assert np.array_equal(_u32(n), _u32(nm)) and np.array_equal(_u32(t), _u32(tm))
