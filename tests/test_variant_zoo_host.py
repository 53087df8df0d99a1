"""The zoo's table (tests/variant_scenes.py CELLS) proven on the host, with no GPU.

For every cell's scene: scene_tables_main (as test_scene_tables.py builds it) gives the scene's feature
bits `feat` and `shade_sk` and the pipelines it may take; kernel_variants_main (as
test_kernel_variants.py builds it) gives the instantiation csrc/rtg_variants.hpp chooses for those
bits, the scene's depth and renderer and the cell's flags and environment; it must be the cell's.
The cells taken together must equal the instantiation sets of test_kernel_variants.py (imported, not
copied), no cell is redundant, and the deep scenes meet their conditions under the oracle: linear ray
trees, and a last level that shows in the image.

The same coverage is printed for the fixture scenes under tests/golden/scenes, so that the gap the
zoo closes stays visible (run with -s).
"""
import glob
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import oracle_bind as ob
import rtgpu
import test_kernel_variants as kv
import test_scene_tables as tst
import variant_scenes as zoo

SCENES = os.path.join(ob.GOLDEN, "scenes")
PARITY = 1e-4


def _unique_scenes():
    return {zoo.key(c.switches): c.switches for c in zoo.CELLS}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """{scene key: the digest of its tables} for every zoo scene (any-hit mode `exact`)."""
    out = tmp_path_factory.mktemp("zoo_tables")
    exe = str(out / "scene_tables_main")
    subprocess.run(tst.BASE + tst.BUILDS["o2"] + tst.SOURCES + ["-o", exe, "-lz"], check=True)
    names = []
    for key, sw in _unique_scenes().items():
        zoo.room(str(out), **sw)
        names.append(key + ".xml")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTG_")}
    r = subprocess.run([exe, "--digest"] + names, cwd=str(out), env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return {k: v["exact"] for k, v in json.loads(r.stdout).items()}


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """(the full table of kernel_variants_main, a function that looks up (sk, feat, depth, pt, rr,
    stats, general) tuples of any depth -> [(MAXD, PT, SK, FEAT)])."""
    exe = str(tmp_path_factory.mktemp("zoo_variants") / "kernel_variants")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(kv.ROCM, "include"), "-I" + kv.CSRC,
                    os.path.join(kv.ROOT, "tests", "kernel_variants_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    full = json.loads(r.stdout)

    def lookup(queries):
        if not queries:
            return []
        args = [str(int(x)) for q in queries for x in q]
        q = subprocess.run([exe] + args, capture_output=True, text=True)
        assert q.returncode == 0 and not q.stderr, q.stderr[-4000:]
        rows = json.loads(q.stdout)["mega"]
        assert [tuple(r[:7]) for r in rows] == [tuple(int(x) for x in q) for q in queries]
        return [(r[7], bool(r[8]), r[9], r[10]) for r in rows]
    return full, lookup


def _mega_query(sk, feat, sw, stats, general):
    s = zoo.resolve(**sw)
    return (sk, feat, s["depth"], s["renderer"] != "rt", s["renderer"] == "pt_rr", bool(stats), bool(general))


def test_every_cell_takes_its_instantiation(tables, variants, capsys):
    full, lookup = variants
    trav = dict(full["trav"])
    step = {(s, f): (k, g) for s, f, k, g in full["step"]}
    tree = dict(full["tree"])
    lines = []
    for c in zoo.CELLS:
        key = zoo.key(c.switches)
        T = tables[key]
        sk, feat = T["shade_sk"], T["feat"]
        assert (sk, feat) == zoo.expected_bits(c.switches), (c.id, sk, feat)      # a switch sets its bit and no other
        s = zoo.resolve(**c.switches)
        pt = s["renderer"] != "rt"
        general = "RTG_MEGA_GENERAL" in c.env
        assert set(c.env) <= {"RTG_MEGA_GENERAL"}
        if c.kernel == "k_render":
            assert c.flags & zoo.FUSED and not c.flags & zoo.TREE
            stats = bool(c.flags & zoo.COUNT)
            got = lookup([_mega_query(sk, feat, c.switches, stats, general)])[0]
            assert got + (stats,) == c.inst, (c.id, got)
            assert got in kv.MEGA[stats]
        elif c.kernel == "k_radiance":
            got = lookup([_mega_query(sk, feat, c.switches, False, general)])[0]
            assert got == c.inst, (c.id, got)
        elif c.kernel == "k_path_step":
            # PIPE_PATH: a path-tracing camera, RTG_RENDER_TREE without RTG_RENDER_FUSED, path_ok
            assert pt and T["path_ok"] and c.flags & zoo.TREE and not c.flags & zoo.FUSED
            counted = bool(c.flags & zoo.COUNT)
            want = (kv.SK_ALL, kv.FEAT_ALL) if counted else step[(sk, feat)]
            assert (counted,) + want == c.inst, (c.id, want)
            # the depth-12 cell and the Russian-roulette cells take the 32-frame path stacks
            maxd = lookup([_mega_query(sk, feat, c.switches, counted, False)])[0][0]
            assert maxd == kv.path_max_depth(s["depth"], s["renderer"] == "pt_rr")
        elif c.kernel == "k_tree_shade":
            # PIPE_TREE: ray tracing, tree_ok, RTG_RENDER_TREE
            assert not pt and T["tree_ok"] and c.flags & zoo.TREE
            assert (tree[sk],) == c.inst, (c.id, tree[sk])
        else:
            pipe, f = c.inst
            assert trav[feat] == f, (c.id, feat, trav[feat])
            if pipe == "wave":
                assert not pt and T["wave_ok"] and c.flags == 0
            elif pipe == "tree":
                assert not pt and T["tree_ok"] and c.flags == zoo.TREE
            elif pipe == "path":
                assert pt and T["path_ok"] and c.flags == zoo.TREE
            else:
                assert c.flags == 0
        lines.append("%-44s %-32s %s" % (zoo.inst_name(c), c.id, key))
    with capsys.disabled():
        print("\ninstantiation -> zoo cell -> scene")
        print("\n".join(lines))


def _required():
    """What the cells must cover: the sets of test_kernel_variants.py, once per kernel / pipeline."""
    return {
        "render": {False: kv.MEGA[False], True: kv.MEGA[True]},
        "radiance": kv.MEGA[False],
        "step": kv.STEP_SETS,
        "step_counted": {(kv.SK_ALL, kv.FEAT_ALL)},
        "tree_shade": kv.TREE_SHADE_SETS,
        "trav": {p: kv.TRAV_SETS for p in zoo.PIPELINES},
    }


def test_cells_equal_the_instantiation_sets():
    got = zoo.covered()
    # RTG_MEGA_GENERAL, the A/B switch, is the reason at least once per kernel, at both stack depths
    switch = got.pop("general_switch")
    assert all(v and v <= kv.MEGA_GENERAL for v in switch.values()), switch
    assert {v[0] for vs in switch.values() for v in vs} == {8, 32}
    assert got == _required()
    # the 16 special cells, per kernel
    for kernel in ("k_render", "k_radiance"):
        assert {c.inst[:4] for c in zoo.CELLS if c.kernel == kernel and zoo.is_special(c)} == kv.MEGA_SPECIAL
    # no cell is redundant: without any one of them the coverage is short
    for k, c in enumerate(zoo.CELLS):
        rest = zoo.CELLS[:k] + zoo.CELLS[k + 1:]
        assert zoo.covered(rest) != zoo.covered(), c.id
    # every depth at which the rule switches, and the last frame
    depths = {zoo.resolve(**c.switches)["depth"] for c in zoo.CELLS if c.kernel == "k_render"}
    assert {0, 3, 8, 9, 31, 32} <= depths


def _oracle(path):
    hs = rtgpu.HostScene(path)
    hdr, _, st = ob.render(hs, seed=1234)
    return hdr, st


def _outside(a, ref):
    """Per pixel: some channel outside the parity bound 1e-4 * max(1, |ref|)."""
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return (np.abs(a - ref) > PARITY * np.maximum(1.0, np.abs(ref))).any(-1)


@pytest.mark.parametrize("name", sorted(zoo.DEEP))
def test_deep_fixture_conditions(name, tmp_path):
    """The committed deep scenes are the generator's, their ray trees are linear, and -- the mirror
    corridors -- the last level is in use: the image at depth d - 1 differs from the image at depth d
    by more than the parity bound in at least 1 % of the pixels, so a device one frame short fails
    the oracle comparison."""
    sw = zoo.DEEP[name]
    assert open(zoo.write_deep(str(tmp_path), name)).read() == open(os.path.join(SCENES, name + ".xml")).read()
    hdr, st = _oracle(os.path.join(SCENES, name + ".xml"))
    d = sw["depth"]
    print(name, st)
    assert st["camera_rays"] == sw["width"] * sw["height"]
    assert 0 < st["secondary_rays"] <= 4 * d * st["camera_rays"]
    less, _ = _oracle(zoo.room(str(tmp_path), "less", **dict(sw, depth=d - 1)))
    frac = float(_outside(less, hdr).mean())
    print(name, "pixels that show level", d, ":", frac)
    if name.startswith("deep_mirrors"):
        assert frac >= 0.01, frac


def test_deep_cells_have_linear_trees(tmp_path):
    """Every zoo scene above depth 8: secondary rays <= 4 * depth * camera rays (no dielectric among
    mirrors), and the closed ray-tracing rooms use their last level as the fixtures do."""
    seen = set()
    for c in zoo.CELLS:
        s = zoo.resolve(**c.switches)
        key = zoo.key(c.switches)
        if s["depth"] <= 8 or key in seen:
            continue
        seen.add(key)
        hdr, st = _oracle(zoo.room(str(tmp_path), **c.switches))
        assert st["secondary_rays"] <= 4 * s["depth"] * st["camera_rays"], (key, st)
        if s["closed"]:
            less, _ = _oracle(zoo.room(str(tmp_path), "less", **dict(c.switches, depth=s["depth"] - 1)))
            assert _outside(less, hdr).mean() >= 0.01, key
    assert len(seen) >= 8


def test_shallow_room_is_depth_invariant(tmp_path):
    """The stack-depth invariance case of test_gpu_variants.py is not vacuous: with the mirrors out of
    each other's view no ray passes level 2, and the oracle's images at depths 8 (MAXD 8) and 9
    (MAXD 32) are equal bit for bit."""
    imgs = [_oracle(zoo.room(str(tmp_path), **dict(zoo.SHALLOW, depth=d))) for d in (8, 9)]
    assert imgs[0][1] == imgs[1][1]
    assert imgs[0][1]["secondary_rays"] > 0
    assert np.array_equal(imgs[0][0].view(np.uint32), imgs[1][0].view(np.uint32))


def _fixture_inputs(name, T):
    root = ET.parse(os.path.join(SCENES, name + ".xml")).getroot()
    d = root.find("MaxRecursionDepth")
    depth = int(d.text) if d is not None else 0
    cam = root.find("Cameras/Camera")
    pt = cam is not None and (cam.findtext("Renderer") or "").strip() == "PathTracing"
    rr = pt and "RussianRoulette" in (cam.findtext("RendererParams") or "")
    return T["shade_sk"], T["feat"], depth, pt, rr


def test_fixture_coverage_report(variants, capsys):
    """What the fixture scenes under tests/golden/scenes reach, whatever flags a test renders them with
    -- printed, and the instantiations only the zoo reaches named."""
    full, lookup = variants
    trav = dict(full["trav"])
    step = {(s, f): (k, g) for s, f, k, g in full["step"]}
    with open(os.path.join(ob.GOLDEN, "scene_tables.json")) as f:
        recorded = json.load(f)
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SCENES, "*.xml")))
    assert set(names) <= set(recorded)
    got = {"render": {False: set(), True: set()}, "step": set(), "trav": set()}
    rows = []
    for name in names:
        sk, feat, depth, pt, rr = _fixture_inputs(name, recorded[name]["exact"])
        v = lookup([(sk, feat, depth, pt, rr, st, False) for st in (False, True)])
        got["render"][False].add(v[0])
        got["render"][True].add(v[1])
        got["trav"].add(trav[feat])
        if pt:
            got["step"].add(step[(sk, feat)])
        rows.append("%-24s sk %d feat %2d depth %2d %s -> uncounted %s counted %s" % (
            name, sk, feat, depth, "pt_rr" if rr else "pt" if pt else "rt", v[0], v[1]))
    with capsys.disabled():
        print("\nfixture scenes (no RTG_MEGA_GENERAL)")
        print("\n".join(rows))
        for st in (False, True):
            print("k_render / k_radiance, STATS %s: reached only by the zoo:" % st, sorted(kv.MEGA[st] - got["render"][st]))
        print("k_path_step<false>: reached only by the zoo:", sorted(kv.STEP_SETS - got["step"]))
        print("traversal sets: reached only by the zoo:", sorted(kv.TRAV_SETS - got["trav"]))
    for st in (False, True):
        assert got["render"][st] <= kv.MEGA[st]
    # the deep fixtures: the (32, false) instantiations run under a reference pin
    assert (32, False, kv.SK_BRDF, kv.FEAT_SPHERE) in got["render"][False]
    assert (32, False, kv.SK_ALL, kv.FEAT_ALL) in got["render"][True]
