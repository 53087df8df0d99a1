"""Variants of the golden scenes for the scene-update tests: the same geometry under other
transforms, cameras, lights and materials.

variant() writes a copy of tests/golden/scenes/<name>.xml with elements edited.  The variants refer
to the PLY files and images of the golden scenes by relative path, so load them -- as in_scenes()
does -- with the current directory at tests/golden/scenes.

An edit is a tuple (op, path, argument[, k]); `path` is an ElementTree path below <Scene>, and k
picks the k-th match (default 0):
    ("set", path, text)                     the element's text
    ("remove", path, None)                  the element
    ("dup", path, [(subpath, text), ...])   a copy right after the element, its children edited
    ("add", parent path, xml[, position])   a new child parsed from `xml` (appended, or at `position`)

PAIRS names, per base scene, the edits that make B out of A = the golden scene itself; every B keeps
A's geometry (meshes, faces, BVH, images), which tests/scene_update_main.cpp asserts.
"""
import contextlib
import copy
import os
import xml.etree.ElementTree as ET

import oracle_bind as ob

SCENES = os.path.join(ob.GOLDEN, "scenes")


def golden(name: str) -> str:
    return os.path.join(SCENES, name + ".xml")


def variant(name: str, out_dir, edits, tag: str = "b") -> str:
    """The golden scene `name` with `edits` applied, written to out_dir; returns its path."""
    root = ET.parse(golden(name)).getroot()
    for e in edits:
        op, path, arg = e[0], e[1], e[2]
        k = e[3] if len(e) > 3 else 0
        if op == "add":
            parent = root if path in ("", ".") else root.findall(path)[0]
            child = ET.fromstring(arg)
            if len(e) > 3:
                parent.insert(e[3], child)
            else:
                parent.append(child)
            continue
        found = root.findall(path)
        assert len(found) > k, (name, path, len(found))
        el = found[k]
        if op == "set":
            el.text = arg
        elif op in ("remove", "dup"):
            parent = next(p for p in root.iter() if el in list(p))
            if op == "remove":
                parent.remove(el)
            else:
                twin = copy.deepcopy(el)
                if "id" in twin.attrib:
                    twin.set("id", str(90 + list(parent).index(el)))
                for sub, text in arg:
                    twin.findall(sub)[0].text = text
                parent.insert(list(parent).index(el) + 1, twin)
        else:
            raise ValueError(op)
    out = os.path.join(str(out_dir), f"{name}_{tag}.xml")
    with open(out, "w") as f:
        f.write(ET.tostring(root, encoding="unicode"))
    return out


@contextlib.contextmanager
def in_scenes():
    old = os.getcwd()
    os.chdir(SCENES)
    try:
        yield
    finally:
        os.chdir(old)


# base scene -> the edits of its B
PAIRS = {
    # mesh, instance, nested instance and sphere transforms; a material; the depth
    "transforms_textures": [
        ("set", "Transformations/Translation[@id='2']", "-2.0 1.1 0.4"),
        ("set", "Transformations/Translation[@id='3']", "2.0 1.0 -1.2"),
        ("set", "Transformations/Rotation[@id='1']", "55 0 1 0"),
        ("set", "Transformations/Rotation[@id='2']", "-40 1 0 0"),
        ("set", "Transformations/Scaling[@id='2']", "0.9 1.1 0.7"),
        ("set", "Materials/Material[@id='2']/DiffuseReflectance", "0.8 0.4 0.2"),
        ("set", "Materials/Material[@id='3']/MirrorReflectance", "0.5 0.6 0.7"),
        ("set", "MaxRecursionDepth", "3"),
    ],
    # the motion-blur vectors of a mesh, an instance and a sphere
    "dof_motion": [
        ("set", ".//MotionBlur", "0.3 0.2 0", 0),
        ("set", ".//MotionBlur", "0 0.25 0.4", 1),
        ("set", ".//MotionBlur", "0.5 0 0.2", 2),
        ("set", "Transformations/Translation[@id='1']", "-1.5 0.2 0.8"),
    ],
    # the light mesh gets a transform and another radiance
    "mesh_light": [
        ("add", ".", "<Transformations><Translation id=\"1\">0.3 -0.4 0.2</Translation></Transformations>", 5),
        ("add", "Objects/LightMesh", "<Transformations>t1</Transformations>"),
        ("set", "Objects/LightMesh/Radiance", "20 15 9"),
    ],
    # a second area light (no environment light)
    "area_light": [
        ("dup", "Lights/AreaLight", [("Position", "3 9.5 1"), ("Radiance", "300 500 900"), ("Size", "2")]),
    ],
    # a second environment light (env_mix grows)
    "env_light": [
        ("dup", "Lights/SphericalDirectionalLight", []),
        ("set", "Lights/PointLight/Position", "-2 5 4"),
    ],
    "bump_normal": [
        ("set", ".//BumpFactor", "0.05", 0),
        ("set", ".//BumpFactor", "0.9", 1),
        ("set", ".//BumpFactor", "1.5", 2),
    ],
    # material types kept, indices changed
    "cornell_dielectric": [
        ("set", "Materials/Material[@id='5']/RefractionIndex", "0.2"),
        ("set", "Materials/Material[@id='5']/AbsorptionIndex", "3.9"),
        ("set", "Materials/Material[@id='6']/RefractionIndex", "1.33"),
        ("set", "Materials/Material[@id='6']/AbsorptionCoefficient", "0.05 0.01 0.03"),
    ],
    # camera and light only
    "synth_10k": [
        ("set", "Cameras/Camera/Position", "0.4 -1.1 1.2"),
        ("set", "Cameras/Camera/Gaze", "-0.2 0.8 -0.55"),
        ("set", "Lights/PointLight/Position", "-1.2 -0.6 1.4"),
        ("set", "Lights/PointLight/Intensity", "300 420 500"),
    ],
}

# a map newly needed: transforms_textures has UVs but no normal / bump map in effect
NEEDS_MAP = ("transforms_textures", [
    ("add", "Textures", "<TextureMap id=\"8\" type=\"perlin\"><DecalMode>bump_normal</DecalMode>"
                        "<NoiseScale>3</NoiseScale><BumpFactor>0.4</BumpFactor></TextureMap>"),
    ("set", "Objects/Mesh[@id='1']/Textures", "1 8"),
])
