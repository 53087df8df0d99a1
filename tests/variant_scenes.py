"""The zoo: small scenes that between them take every kernel instantiation csrc/rtg_variants.hpp can
choose (test_variant_zoo_host.py proves the table on the host, test_gpu_variants.py runs every row
on the device).  A helper module like radiance_rays.py, not a conftest.

One base room -- a ground mesh under the identity transform, a mirror back wall, a diffuse, a mirror,
a conductor and one dielectric sphere, a point light -- and independent switches that each set one
feature bit (room()'s arguments):

    brdf        BRDF materials                           SK_BRDF
    xlight      a spot light                             SK_XLIGHT
    tex         a Perlin replace_kd texture              SK_TEX
    xform       a translated mesh                        FEAT_XFORM
    instance    a MeshInstance                           FEAT_INSTANCE
    bigleaf     bvh_cases.copies(17) as a mesh           FEAT_BIGLEAF
    spheres     False: no sphere at all                  feat 0 or 8
    depth       MaxRecursionDepth                        MAXD 0 / 8 / 32
    renderer    "rt", "pt" or "pt_rr"                    PT, and with Russian roulette the 32-frame stack
    bodies      "all"; "metal": no dielectric (the deep scenes: linear ray trees); "glass": the
                dielectric sphere among diffuse bodies, no mirror; "shallow": one mirror sphere among
                diffuse bodies (no ray passes level 2)
    closed      the room closed by mirror and conductor walls, a mirror floor and ceiling, the camera
                inside: every ray tree runs to MaxRecursionDepth, one ray per level

CELLS lists one row per instantiation and pipeline: the switches of a scene that reaches it and the
render flags and environment of the launch that takes it.  The three deep reference fixtures
(tests/golden/scenes/deep_*.xml, written by write_deep for make_goldens.py) are rooms too.
"""
import collections
import itertools
import os

import bvh_cases
import rtgpu
import scenes as gen

FEAT_SPHERE, FEAT_INSTANCE, FEAT_XFORM, FEAT_BIGLEAF, FEAT_ALL = 1, 2, 4, 8, 15
SK_TEX, SK_BRDF, SK_XLIGHT, SK_ALL = 1, 2, 4, 7
FUSED, TREE, COUNT = rtgpu.RTG_RENDER_FUSED, rtgpu.RTG_RENDER_TREE, rtgpu.RTG_RENDER_COUNT_STATS
GENERAL = {"RTG_MEGA_GENERAL": "1"}
WIDTH, HEIGHT = 100, 60          # 6 000 pixels: 94 wavefronts, the last one partial

DEFAULTS = dict(spheres=True, brdf=False, xlight=False, tex=False, xform=False, instance=False, bigleaf=False,
                depth=3, renderer="rt", bodies=None, closed=None, spp=None, width=WIDTH, height=HEIGHT)


def resolve(**sw):
    """The switches with their defaults filled in: no dielectric above depth 8 (its tree doubles per
    level), ray-tracing rooms above depth 8 closed, 2 samples per pixel for path tracing."""
    bad = set(sw) - set(DEFAULTS)
    assert not bad, bad
    s = dict(DEFAULTS, **sw)
    if s["bodies"] is None:
        s["bodies"] = "all" if s["depth"] <= 8 else "metal"
    if s["closed"] is None:
        s["closed"] = s["renderer"] == "rt" and s["depth"] > 8 and s["bodies"] == "metal"
    if s["spp"] is None:
        s["spp"] = 1 if s["renderer"] == "rt" else 2
    assert s["bodies"] in ("all", "metal", "glass", "shallow") and s["renderer"] in ("rt", "pt", "pt_rr")
    assert not (s["closed"] and s["bodies"] != "metal")
    return s


def key(sw):
    """A file-name-safe name of a set of switches (resolved)."""
    s = resolve(**sw)
    parts = [s["renderer"], "d%d" % s["depth"], s["bodies"]]
    parts += [k for k in ("brdf", "xlight", "tex", "xform", "instance", "bigleaf", "closed") if s[k]]
    if not s["spheres"]:
        parts.append("nosphere")
    if (s["width"], s["height"]) != (WIDTH, HEIGHT):
        parts.append("%dx%d" % (s["width"], s["height"]))
    if s["spp"] > 1:
        parts.append("spp%d" % s["spp"])
    return "_".join(parts)


def expected_bits(sw):
    """(shade_sk, feat) the switches are meant to set; the host test checks them against the tables."""
    s = resolve(**sw)
    sk = (SK_BRDF if s["brdf"] else 0) | (SK_XLIGHT if s["xlight"] else 0) | (SK_TEX if s["tex"] else 0)
    feat = ((FEAT_SPHERE if s["spheres"] else 0) | (FEAT_XFORM if s["xform"] else 0) |
            (FEAT_INSTANCE if s["instance"] else 0) | (FEAT_BIGLEAF if s["bigleaf"] else 0))
    return sk, feat


# the room's corners: x in [-4, 4], y in [0, 5], z in [-3.5, 8]; the camera stands at z = 6.5
_BOX = [(-4, 0, -3.5), (4, 0, -3.5), (4, 0, 8), (-4, 0, 8), (-4, 5, -3.5), (4, 5, -3.5), (4, 5, 8), (-4, 5, 8)]
_SPHERES = [(-2.2, 0.8, 0.5), (-0.6, 0.9, -1.8), (2.4, 0.8, -1.6), (0.9, 0.6, 2.4)]
_PLAQUE = [(2.6, 0, 1.5), (3.6, 0, 1.5), (3.6, 1.2, 1.5), (2.6, 1.2, 1.5)]
BIG_COPIES = 17                  # faces of the large leaf: more than kBigLeaf = 8


def _mesh(mid, material, faces, extra=""):
    rows = "\n                ".join(faces)
    return (f'        <Mesh id="{mid}">\n            <Material>{material}</Material>{extra}\n'
            f'            <Faces>\n                {rows}\n            </Faces>\n        </Mesh>')


def _sphere(sid, material, centre, radius):
    return (f'        <Sphere id="{sid}"><Material>{material}</Material><Center>{centre}</Center>'
            f'<Radius>{radius}</Radius></Sphere>')


def room(out_dir, name=None, **sw):
    """Write the room with these switches to <out_dir>/<name or key(sw)>.xml; returns the path.  The
    scene refers to no other file."""
    s = resolve(**sw)
    name = name or key(sw)
    bodies, closed = s["bodies"], s["closed"]
    big_v, big_f = bvh_cases.copies(BIG_COPIES)
    verts = _BOX + _SPHERES + [tuple(float(x) for x in v) for v in big_v] + _PLAQUE
    vdata = "\n        ".join("%g %g %g" % v for v in verts)
    b = " BRDF=\"%d\""
    brdf1, brdf2 = (b % 1, b % 2) if s["brdf"] else ("", "")
    ground_mat = 6 if closed else 1
    tex = "\n            <Textures>1</Textures>" if s["tex"] else ""
    objs = [_mesh(1, ground_mat, ["1 3 2", "1 4 3"], tex)]
    mid = 2
    if bodies in ("all", "metal"):                         # the back wall: a mirror
        objs.append(_mesh(mid, 3, ["1 2 6", "1 6 5"]))
        mid += 1
    if closed:
        objs.append(_mesh(mid, 3, ["4 7 3", "4 8 7"]))      # front wall (behind the camera): a mirror
        objs.append(_mesh(mid + 1, 4, ["1 5 8", "1 8 4"]))  # left and right walls: conductors
        objs.append(_mesh(mid + 2, 4, ["2 7 6", "2 3 7"]))
        objs.append(_mesh(mid + 3, 3, ["5 6 7", "5 7 8"]))  # ceiling: a mirror
        mid += 4
    if s["bigleaf"]:
        objs.append(_mesh(mid, 2, ["%d %d %d" % tuple(13 + r) for r in big_f]))
        mid += 1
    if s["xform"] or s["instance"]:
        move = "\n            <Transformations>t1</Transformations>" if s["xform"] else ""
        objs.append(_mesh(mid, 2, ["16 17 18", "16 18 19"], move))
        if s["instance"]:
            objs.append(f'        <MeshInstance id="{mid + 1}" baseMeshId="{mid}">\n            <Material>1</Material>\n'
                        '            <Transformations>t2</Transformations>\n        </MeshInstance>')
        mid += 2
    if s["spheres"]:
        objs.append(_sphere(1, 2, 9, 0.8))
        if bodies in ("all", "metal", "shallow"):
            objs.append(_sphere(2, 3, 10, 0.9))
        else:
            objs.append(_sphere(2, 1, 10, 0.9))
        if bodies in ("all", "metal"):
            objs.append(_sphere(3, 4, 11, 0.8))
        if bodies in ("all", "glass"):
            objs.append(_sphere(4, 5, 12, 0.6))
    renderer = ""
    if s["renderer"] != "rt":
        params = "NextEventEstimation ImportanceSampling" + (" RussianRoulette" if s["renderer"] == "pt_rr" else "")
        renderer = (f"\n            <Renderer>PathTracing</Renderer>\n            <RendererParams>{params}</RendererParams>")
    samples = f"\n            <NumSamples>{s['spp']}</NumSamples>" if s["spp"] > 1 else ""
    spot = """
        <SpotLight id="1">
            <Position>0 4.5 3</Position>
            <Direction>0 -1 -0.45</Direction>
            <Intensity>2500 2500 2000</Intensity>
            <CoverageAngle>50</CoverageAngle>
            <FalloffAngle>20</FalloffAngle>
        </SpotLight>""" if s["xlight"] else ""
    brdfs = """    <BRDFs>
        <OriginalBlinnPhong id="1">
            <Exponent>30</Exponent>
        </OriginalBlinnPhong>
        <ModifiedPhong id="2" normalized="true">
            <Exponent>25</Exponent>
        </ModifiedPhong>
    </BRDFs>
""" if s["brdf"] else ""
    textures = """    <Textures>
        <TextureMap id="1" type="perlin">
            <DecalMode>replace_kd</DecalMode>
            <NoiseConversion>absval</NoiseConversion>
            <NoiseScale>1.5</NoiseScale>
        </TextureMap>
    </Textures>
""" if s["tex"] else ""
    xml = f"""<Scene>
    <MaxRecursionDepth>{s['depth']}</MaxRecursionDepth>
    <BackgroundColor>20 25 40</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1" type="lookAt">
            <Position>0 2.2 6.5</Position>
            <GazePoint>0 0.8 0</GazePoint>
            <Up>0 1 0</Up>
            <FovY>42</FovY>
            <NearDistance>1</NearDistance>
            <ImageResolution>{s['width']} {s['height']}</ImageResolution>
            <ImageName>{name}.png</ImageName>{samples}{renderer}
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>15 15 15</AmbientLight>
        <PointLight id="1">
            <Position>1.5 4.2 3</Position>
            <Intensity>2500 2400 2300</Intensity>
        </PointLight>{spot}
    </Lights>
{brdfs}    <Materials>
        <Material id="1"{brdf1}>
            <AmbientReflectance>0.3 0.3 0.3</AmbientReflectance>
            <DiffuseReflectance>0.5 0.5 0.5</DiffuseReflectance>
            <SpecularReflectance>0.2 0.2 0.2</SpecularReflectance>
            <PhongExponent>10</PhongExponent>
        </Material>
        <Material id="2"{brdf2}>
            <AmbientReflectance>0.3 0.1 0.1</AmbientReflectance>
            <DiffuseReflectance>0.7 0.2 0.2</DiffuseReflectance>
            <SpecularReflectance>0.4 0.4 0.4</SpecularReflectance>
            <PhongExponent>25</PhongExponent>
        </Material>
        <Material id="3" type="mirror">
            <AmbientReflectance>0.1 0.1 0.1</AmbientReflectance>
            <DiffuseReflectance>0.15 0.15 0.15</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <MirrorReflectance>0.9 0.9 0.9</MirrorReflectance>
        </Material>
        <Material id="4" type="conductor">
            <AmbientReflectance>0.1 0.1 0.1</AmbientReflectance>
            <DiffuseReflectance>0.1 0.05 0.02</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <MirrorReflectance>1 0.86 0.57</MirrorReflectance>
            <RefractionIndex>0.370</RefractionIndex>
            <AbsorptionIndex>2.820</AbsorptionIndex>
        </Material>
        <Material id="5" type="dielectric">
            <AmbientReflectance>0 0 0</AmbientReflectance>
            <DiffuseReflectance>0 0 0</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <AbsorptionCoefficient>0.01 0.05 0.1</AbsorptionCoefficient>
            <RefractionIndex>1.5</RefractionIndex>
        </Material>
        <Material id="6" type="mirror">
            <AmbientReflectance>0.2 0.2 0.2</AmbientReflectance>
            <DiffuseReflectance>0.3 0.3 0.35</DiffuseReflectance>
            <SpecularReflectance>0.1 0.1 0.1</SpecularReflectance>
            <PhongExponent>10</PhongExponent>
            <MirrorReflectance>0.9 0.9 0.9</MirrorReflectance>
        </Material>
    </Materials>
{textures}    <VertexData>
        {vdata}
    </VertexData>
    <Transformations>
        <Translation id="1">-6 0 0.5</Translation>
        <Translation id="2">0.2 1.4 0.4</Translation>
    </Transformations>
    <Objects>
{chr(10).join(objs)}
    </Objects>
</Scene>
"""
    return gen._write(str(out_dir), name, xml)


# ---------------------------------------------------------------------------
# The deep reference fixtures (tests/golden/scenes/deep_*.xml; make_goldens.py)
# ---------------------------------------------------------------------------
DEEP = {
    # the closed mirror and conductor corridor: one ray per level, every level in use
    "deep_mirrors_9": dict(depth=9, width=96, height=64),
    "deep_mirrors_32": dict(depth=32, width=96, height=64),
    # the single dielectric sphere (Beer absorption) among diffuse bodies, no mirror
    "deep_glass_12": dict(depth=12, bodies="glass", width=96, height=64),
}


# the stack-depth invariance case: one mirror sphere among diffuse bodies, no ray passes level 2, so
# the images at depths 8 (MAXD 8) and 9 (MAXD 32) are the same work on two frame stacks
SHALLOW = dict(bodies="shallow", closed=False, brdf=True)
# the same without a closing wall at any depth: the open metal room, whose rays leave within 8 levels
OPEN_METAL = dict(bodies="metal", closed=False)
# the update across the 8 / 9 switch: the closed room (every level shows) at depths 6 and 12
UPDATE = dict(bodies="metal", closed=True, xlight=True)


def write_deep(out_dir, name):
    return room(out_dir, name, **DEEP[name])


# ---------------------------------------------------------------------------
# CELLS
# ---------------------------------------------------------------------------
# kernel: "k_render" inst (MAXD, PT, SK, FEAT, STATS); "k_radiance" inst (MAXD, PT, SK, FEAT);
# "k_path_step" inst (STATS, SK, FEAT); "k_tree_shade" inst (SK,); "trav" inst (pipeline, FEAT).
# switches: room()'s arguments; flags / env: of the render that takes the instantiation (radiance and
# ray queries have no flags).
Cell = collections.namedtuple("Cell", "id kernel inst switches flags env")
PIPELINES = ("wave", "tree", "query", "anyhit", "multihit", "surface", "path")


def _sk_switches(sk):
    return dict(brdf=bool(sk & SK_BRDF), xlight=bool(sk & SK_XLIGHT), tex=bool(sk & SK_TEX))


def _feat_switches(feat):
    return dict(spheres=bool(feat & FEAT_SPHERE), instance=bool(feat & FEAT_INSTANCE), xform=bool(feat & FEAT_XFORM),
                bigleaf=bool(feat & FEAT_BIGLEAF))


def _mega_rows():
    """[(MAXD, PT, SK, FEAT), switches, env]: the uncounted k_render / k_radiance instantiations."""
    rows = []
    # special: the depths on both sides of every rule -- 3 and 8 take MAXD 8; 9, 31 and 32 take 32;
    # path tracing takes 32 with Russian roulette at any depth, and without it above 8
    rt_depth = {8: itertools.cycle((3, 8)), 32: itertools.cycle((9, 32, 31, 32))}
    pt_mode = {8: itertools.cycle((("pt", 3), ("pt", 8))), 32: itertools.cycle((("pt_rr", 3), ("pt", 12), ("pt", 9), ("pt_rr", 1)))}
    for maxd, pt, sk, feat in itertools.product((8, 32), (False, True), (SK_BRDF, SK_BRDF | SK_XLIGHT),
                                                (FEAT_SPHERE, FEAT_SPHERE | FEAT_BIGLEAF)):
        sw = dict(_sk_switches(sk), bigleaf=bool(feat & FEAT_BIGLEAF))
        if sk == SK_BRDF and feat == FEAT_SPHERE:
            sw["brdf"] = False                             # sk = 0 takes the SK_BRDF instantiation too
        if pt:
            sw["renderer"], sw["depth"] = next(pt_mode[maxd])
        else:
            sw["depth"] = next(rt_depth[maxd])
        rows.append(((maxd, pt, sk, feat), sw, {}))
    # general: depth 0; a texture; a transform; an instance -- and RTG_MEGA_GENERAL on scenes that
    # would take a special instantiation
    rows += [((0, False, SK_ALL, FEAT_ALL), dict(depth=0), {}),
             ((8, False, SK_ALL, FEAT_ALL), dict(depth=8, tex=True, brdf=True), {}),
             ((32, False, SK_ALL, FEAT_ALL), dict(depth=32, xform=True, xlight=True), {}),
             ((8, True, SK_ALL, FEAT_ALL), dict(renderer="pt", depth=3, instance=True), {}),
             ((32, True, SK_ALL, FEAT_ALL), dict(renderer="pt_rr", depth=2, tex=True, xlight=True), {})]
    return rows


def _cells():
    out = []
    for inst, sw, env in _mega_rows():
        tag = "d%d_%s_sk%d_f%d" % (inst[0], "pt" if inst[1] else "rt", inst[2], inst[3])
        out.append(Cell("render_" + tag, "k_render", inst + (False,), sw, FUSED, env))
        out.append(Cell("radiance_" + tag, "k_radiance", inst, sw, 0, env))
    # the counted builds: the general instantiations only, on scenes whose uncounted render is special
    counted = [((0, False), dict(depth=0, brdf=True)), ((8, False), dict(depth=3, xlight=True)),
               ((32, False), dict(depth=31, bigleaf=True)), ((8, True), dict(renderer="pt", depth=2, brdf=True)),
               ((32, True), dict(renderer="pt", depth=9))]
    for (maxd, pt), sw in counted:
        out.append(Cell("render_counted_d%d_%s" % (maxd, "pt" if pt else "rt"), "k_render",
                        (maxd, pt, SK_ALL, FEAT_ALL, True), sw, FUSED | COUNT, {}))
    # the wavefront path tracer's step kernel; one cell at depth 12 without Russian roulette (the
    # 32-frame path stacks), Russian roulette on others
    modes = itertools.cycle((("pt", 3), ("pt_rr", 2), ("pt", 12)))
    for sk, feat in itertools.product((SK_BRDF, SK_BRDF | SK_XLIGHT, SK_ALL), (FEAT_SPHERE, FEAT_SPHERE | FEAT_BIGLEAF, FEAT_ALL)):
        sw = dict(_sk_switches(sk), bigleaf=bool(feat & FEAT_BIGLEAF), xform=feat == FEAT_ALL)
        sw["renderer"], sw["depth"] = next(modes)
        out.append(Cell("step_sk%d_f%d" % (sk, feat), "k_path_step", (False, sk, feat), sw, TREE, {}))
    out.append(Cell("step_counted", "k_path_step", (True, SK_ALL, FEAT_ALL), dict(renderer="pt", depth=3, xlight=True),
                    TREE | COUNT, {}))
    out.append(Cell("tree_shade_sk1", "k_tree_shade", (SK_TEX,), dict(depth=3, tex=True), TREE, {}))
    out.append(Cell("tree_shade_sk7", "k_tree_shade", (SK_ALL,), dict(depth=3, brdf=True), TREE, {}))
    # every traversal set in every pipeline that instantiates it
    for feat, pipe in itertools.product((0, FEAT_SPHERE, FEAT_ALL & ~FEAT_BIGLEAF, FEAT_BIGLEAF, FEAT_SPHERE | FEAT_BIGLEAF,
                                         FEAT_ALL), PIPELINES):
        sw = _feat_switches(feat)
        if feat == FEAT_ALL & ~FEAT_BIGLEAF:
            sw["spheres"] = pipe != "query"                # xform + instance without spheres walks set 7 too
        if feat == FEAT_ALL:
            sw["instance"] = pipe in ("tree", "anyhit", "path")   # FEAT_XFORM | FEAT_BIGLEAF alone walks set 15 too
        sw["depth"] = 0 if pipe == "wave" else 3
        flags = 0
        if pipe == "path":
            sw["renderer"] = "pt"
        if pipe in ("tree", "path"):
            flags = TREE
        out.append(Cell("trav_%s_f%d" % (pipe, feat), "trav", (pipe, feat), sw, flags, {}))
    # RTG_MEGA_GENERAL, the A/B switch, as the reason a general instantiation is taken
    out.append(Cell("render_general_switch_d8", "k_render", (8, False, SK_ALL, FEAT_ALL, False), dict(depth=3, brdf=True),
                    FUSED, GENERAL))
    out.append(Cell("radiance_general_switch_d32", "k_radiance", (32, False, SK_ALL, FEAT_ALL), dict(depth=9, bigleaf=True),
                    0, GENERAL))
    assert len({c.id for c in out}) == len(out)
    return out


CELLS = _cells()


def is_special(cell):
    return cell.kernel in ("k_render", "k_radiance") and cell.inst[2] != SK_ALL


def is_path_tracing(cell):
    return resolve(**cell.switches)["renderer"] != "rt"


def covered(cells=None):
    """The instantiation sets the cells cover, shaped like test_kernel_variants.py's: by what the scene
    is, and -- "general_switch" -- because RTG_MEGA_GENERAL says so."""
    cells = CELLS if cells is None else cells
    return {
        "render": {st: {c.inst[:4] for c in cells if c.kernel == "k_render" and c.inst[4] == st and not c.env}
                   for st in (False, True)},
        "radiance": {c.inst for c in cells if c.kernel == "k_radiance" and not c.env},
        "general_switch": {k: {c.inst[:4] for c in cells if c.kernel == k and c.env} for k in ("k_render", "k_radiance")},
        "step": {c.inst[1:] for c in cells if c.kernel == "k_path_step" and not c.inst[0]},
        "step_counted": {c.inst[1:] for c in cells if c.kernel == "k_path_step" and c.inst[0]},
        "tree_shade": {c.inst[0] for c in cells if c.kernel == "k_tree_shade"},
        "trav": {p: {c.inst[1] for c in cells if c.kernel == "trav" and c.inst[0] == p} for p in PIPELINES},
    }


def assertions(cell):
    """The checks of test_gpu_variants.py that run on a cell, by name."""
    s = resolve(**cell.switches)
    a = []
    if cell.kernel == "k_render":
        a.append("oracle" + (" + counters" if cell.inst[4] else ""))
        if is_special(cell):
            a.append("special == general")
        if cell.inst[4] or cell.env:
            a.append("counted == uncounted")
        if s["renderer"] == "rt" and s["depth"] > 0:
            a.append("tree == fused")
    elif cell.kernel == "k_radiance":
        a.append("oracle")
        if is_special(cell):
            a.append("special == general")
    elif cell.kernel == "k_path_step":
        a += ["oracle", "wavefront == fused"]
    elif cell.kernel == "k_tree_shade":
        a += ["oracle", "tree == fused"]
    else:
        a.append({"wave": "oracle, wave == fused", "tree": "oracle, tree == fused", "path": "oracle, wavefront == fused",
                  "query": "device == host", "anyhit": "device == host", "multihit": "device == host",
                  "surface": "device == host, == trace"}[cell.inst[0]])
    return a


def inst_name(cell):
    i = cell.inst
    b = lambda v: "true" if v else "false"
    if cell.kernel == "k_render":
        return "k_render<%d, %s, %s, %d, %d>" % (i[0], b(i[4]), b(i[1]), i[2], i[3])
    if cell.kernel == "k_radiance":
        return "k_radiance<%d, %s, %d, %d>" % (i[0], b(i[1]), i[2], i[3])
    if cell.kernel == "k_path_step":
        return "k_path_step<%s, %d, %d>" % (b(i[0]), i[1], i[2])
    if cell.kernel == "k_tree_shade":
        return "k_tree_shade<·, %d>" % i[0]
    return "%s walk, FEAT %d" % i


def design_table():
    """DESIGN.md §2's table: instantiation, zoo cell (its scene), assertions."""
    rows = ["| instantiation | zoo cell | scene | assertions |", "|---|---|---|---|"]
    for c in CELLS:
        rows.append("| `%s` | `%s` | `%s` | %s |" % (inst_name(c), c.id, key(c.switches), "; ".join(assertions(c))))
    return "\n".join(rows)


if __name__ == "__main__":
    print(design_table())
