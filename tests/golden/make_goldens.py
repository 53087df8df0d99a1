"""Generate the golden fixtures under tests/golden/ from the reference itself.

Runs only in the container that has /root/reference: it renders every fixture scene
with oracle/_ref/refdriver (the reference's own sources compiled by oracle/Makefile,
driving Raytracer::RenderPixel single-threaded) and stores the float32 images as
tests/golden/<name>.npz plus tests/golden/manifest.json (sizes, kinds, SHA-256).

Fixture scenes live in tests/golden/scenes/: copies of the reference's own scene files
(archive/hw1_inputs, data) re-sized, plus scenes authored in its XML schema.

    python tests/golden/make_goldens.py            # regenerate everything (the edge-ray goldens
                                                   # last: they need the built librtgpu.so)
    python tests/golden/make_goldens.py edge_rays  # only the edge-ray goldens (edge_rays_<scene>.npz)
                                                   # and scenes/edge_lattice.xml
    python tests/golden/make_goldens.py radiance_rays   # only the radiance-ray goldens
                                                        # (radiance_rays_<scene>.npz)
    python tests/golden/make_goldens.py bvh        # only the BVH goldens (bvh_<case>.npz, bvh_manifest.json)
    python tests/golden/make_goldens.py walk_rays  # only the walk goldens (walk_rays_<case>.npz,
                                                   # walk_rays_manifest.json)
"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SCENES = os.path.join(HERE, "scenes")
REF = "/root/reference/archive/hw1_inputs"
DRIVER = os.path.join(ROOT, "oracle", "_ref", "refdriver")
sys.path.insert(0, os.path.join(ROOT, "advanced-cpu-raytracing_amd"))
import scenes as gen  # noqa: E402

# name -> (source, width, height, kind, edits)
FIXTURES = {
    "simple": (f"{REF}/simple.xml", 200, 200, "exact", None),
    "two_spheres": (f"{REF}/two_spheres.xml", 200, 200, "exact", None),
    "spheres": (f"{REF}/spheres.xml", 180, 180, "exact", None),
    "spheres_mirror": (f"{REF}/spheres_mirror.xml", 180, 180, "exact", None),
    "cornell_conductors": (f"{REF}/cornellbox_recursive_conductors.xml", 200, 200, "exact", None),
    # the archived alt2 camera looks above the ceiling; reset it to (0 0 20)
    "cornell_dielectric": (f"{REF}/cornellbox_recursive_alt2.xml", 200, 200, "exact",
                           [("<Position>-10 15 0</Position>", "<Position>0 0 20</Position>"),
                            ("<Gaze>0.7 -1 0</Gaze>", "<Gaze>0 0 -1</Gaze>")]),
    "scienceTree": (f"{REF}/scienceTree.xml", 288, 144, "exact", None),
    "scienceTree_diamond": (f"{REF}/scienceTree_diamond.xml", 288, 144, "exact", None),
    "berserker": (f"{REF}/akif_uslu/berserker_smooth.xml", 96, 128, "exact", None),
    # the rest of the shipped scenes the reference renders.  The akif_uslu scenes
    # with an empty <TexCoordData /> crash the reference's parser (parser.cpp:279-291), so
    # that element is removed; car_smooth_fixed's second camera is pinned by a copy whose
    # first <Camera> is removed (no tonemapper / renderer params to inherit, parser.cpp:1504).
    "car_smooth": (f"{REF}/akif_uslu/car_smooth_fixed.xml", 256, 192, "exact", None),
    "car_smooth_front": (f"{REF}/akif_uslu/car_smooth_fixed.xml", 256, 192, "exact", "drop_first_camera"),
    "low_poly": (f"{REF}/akif_uslu/low_poly_smooth.xml", 192, 192, "exact", None),
    "ton_roosendaal": (f"{REF}/akif_uslu/ton_Roosendaal_smooth.xml", 216, 216, "exact", [("<TexCoordData />", "")]),
    "tower": (f"{REF}/akif_uslu/tower_smooth.xml", 108, 192, "exact", [("<TexCoordData />", "")]),
    "windmill": (f"{REF}/akif_uslu/windmill_smooth.xml", 200, 200, "exact", [("<TexCoordData />", "")]),
    "brdf_lights": ("authored", 200, 150, "exact", None),
    "transforms_textures": ("authored", 200, 150, "exact", None),
    "synth_10k": ("generated", 256, 144, "exact", None),
    "ply_quads": ("generated", 160, 120, "exact", None),
    "bump_normal": ("generated", 200, 150, "exact", None),
    # PNG textures (stbi_load, nearest / bilinear, replace_kd / blend_kd) and a 16-bit PNG
    # background: the image-decoder fixtures of make_images.py in a scene
    "image_tex": ("generated", 160, 120, "exact", None),
    # path tracing (raytracer.cpp:135-191): per-pixel mean of AVG_SAMPLES reference samples
    "pt_cornell": ("generated", 64, 64, "stochastic_avg", None),
    "pt_nee": ("generated", 64, 64, "stochastic_avg", None),
    "pt_rr": ("generated", 64, 64, "stochastic_avg", None),
    "area_light": ("authored", 160, 160, "stochastic", None),
    "env_light": ("authored", 160, 120, "stochastic", None),
    "dof_motion": ("authored", 160, 120, "stochastic", None),
    # reduced BASELINE.json configurations (scenes.config_c2..c5, 1 spp)
    "c2_cornell": ("generated", 200, 200, "exact", None),
    "c3_blob": ("generated", 192, 108, "stochastic", None),
    # c4_forest (MeshInstance forest) has no reference golden: the reference reads the
    # uninitialised Shape::material_id of every InstancedMesh in CastShadowRay
    # (raytracer.cpp:590; InstancedMesh::SetMaterial sets a shadowing private member,
    # instancedMesh.hpp:23) and segfaults once the heap garbage is out of range; C4 is
    # checked GPU vs the CPU restatement (tests/test_gpu_parity.py).
    "c5_dragon": ("generated", 192, 108, "exact", None),
    # ray trees above depth 8 (the 32-frame stacks): rooms of tests/variant_scenes.py -- the closed
    # mirror and conductor corridor at depths 9 and 32 (one ray per level, every level in use) and
    # the single dielectric sphere with Beer absorption at depth 12
    "deep_mirrors_9": ("generated", 96, 64, "exact", None),
    "deep_mirrors_32": ("generated", 96, 64, "exact", None),
    "deep_glass_12": ("generated", 96, 64, "exact", None),
}


def make_ply_quads():
    """A PLY with quad faces (split 0-1-2 / 2-3-0, parser.cpp:1428-1439) and an offset cube."""
    n = 12
    xs = np.linspace(-2, 2, n + 1)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    Y = 0.25 * np.sin(2 * X) * np.cos(3 * Z)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n + 1) ** 2).reshape(n + 1, n + 1)
    quads = np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]], -1).reshape(-1, 4)
    gen.write_ply(os.path.join(SCENES, "quads.ply"), verts, quads)
    xml = """<Scene>
    <MaxRecursionDepth>1</MaxRecursionDepth>
    <BackgroundColor>30 30 50</BackgroundColor>
    <Cameras>
        <Camera id="1" type="lookAt">
            <Position>0 3 5</Position>
            <GazePoint>0 0 0</GazePoint>
            <Up>0 1 0</Up>
            <FovY>50</FovY>
            <NearDistance>1</NearDistance>
            <ImageResolution>160 120</ImageResolution>
            <ImageName>ply_quads.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>15 15 15</AmbientLight>
        <PointLight id="1"><Position>2 4 3</Position><Intensity>700 700 700</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>0.6 0.7 0.5</DiffuseReflectance>
            <SpecularReflectance>0.4 0.4 0.4</SpecularReflectance>
            <PhongExponent>25</PhongExponent>
        </Material>
        <Material id="2" type="mirror">
            <AmbientReflectance>0.1 0.1 0.1</AmbientReflectance>
            <DiffuseReflectance>0.1 0.1 0.2</DiffuseReflectance>
            <MirrorReflectance>0.6 0.6 0.6</MirrorReflectance>
        </Material>
    </Materials>
    <VertexData>0 0 0</VertexData>
    <Transformations>
        <Translation id="1">0 0.6 0</Translation>
        <Scaling id="1">0.3 0.3 0.3</Scaling>
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces plyFile="quads.ply"/>
        </Mesh>
        <Mesh id="2">
            <Material>2</Material>
            <Transformations>s1 t1</Transformations>
            <Faces plyFile="quads.ply" vertexOffset="0"/>
        </Mesh>
    </Objects>
</Scene>
"""
    with open(os.path.join(SCENES, "ply_quads.xml"), "w") as f:
        f.write(xml)


def make_image_tex():
    """Two textured quads (an RGB and a palette PNG) in front of a 16-bit PNG
    replace_background texture; copies the decoder fixtures to scenes/inputs/."""
    for f in ("png_rgb8.png", "png_pal8.png", "png_rgb16.png"):
        shutil.copyfile(os.path.join(HERE, "images", f), os.path.join(SCENES, "inputs", f))
    xml = """<Scene>
    <MaxRecursionDepth>1</MaxRecursionDepth>
    <BackgroundColor>0 0 0</BackgroundColor>
    <Cameras>
        <Camera id="1">
            <Position>0 0 6</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>2</NearDistance>
            <ImageResolution>160 120</ImageResolution>
            <ImageName>image_tex.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>0 2 5</Position><Intensity>900 900 900</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>0.2 0.2 0.2</AmbientReflectance>
            <DiffuseReflectance>0.8 0.8 0.8</DiffuseReflectance>
            <SpecularReflectance>0.3 0.3 0.3</SpecularReflectance>
            <PhongExponent>20</PhongExponent>
        </Material>
    </Materials>
    <Textures>
        <Images>
            <Image id="1">png_rgb8.png</Image>
            <Image id="2">png_pal8.png</Image>
            <Image id="3">png_rgb16.png</Image>
        </Images>
        <TextureMap id="1" type="image">
            <ImageId>1</ImageId>
            <DecalMode>replace_kd</DecalMode>
            <Interpolation>bilinear</Interpolation>
        </TextureMap>
        <TextureMap id="2" type="image">
            <ImageId>2</ImageId>
            <DecalMode>blend_kd</DecalMode>
            <Interpolation>nearest</Interpolation>
        </TextureMap>
        <TextureMap id="3" type="image">
            <ImageId>3</ImageId>
            <DecalMode>replace_background</DecalMode>
            <Interpolation>bilinear</Interpolation>
        </TextureMap>
    </Textures>
    <VertexData>
        -2.1 -1.2 0
        -0.1 -1.2 0
        -0.1 1.2 0
        -2.1 1.2 0
        0.1 -1.0 -0.5
        2.1 -1.0 0
        2.1 1.0 0
        0.1 1.0 -0.5
    </VertexData>
    <TexCoordData>
        0 1
        1 1
        1 0
        0 0
        0 1
        1 1
        1 0
        0 0
    </TexCoordData>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Textures>1</Textures>
            <Faces>1 2 3 1 3 4</Faces>
        </Mesh>
        <Mesh id="2">
            <Material>1</Material>
            <Textures>2</Textures>
            <Faces>5 6 7 5 7 8</Faces>
        </Mesh>
    </Objects>
</Scene>
"""
    with open(os.path.join(SCENES, "image_tex.xml"), "w") as f:
        f.write(xml)


def write_ppm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(img, np.uint8).tobytes())


def make_bump_normal():
    """Normal maps (mesh), image and Perlin bump maps (mesh, instance of a bumped mesh,
    sphere): mesh.cpp:263-358, sphere.cpp:116-193.  Images are seeded patterns written as
    PPM under scenes/inputs/ (parser.cpp:110 prefixes "inputs/")."""
    n = 64
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) / n
    # normal map: tangent-space normals of a sum of bumps, encoded (n + 1) * 127.5
    hx = 0.6 * np.cos(2 * np.pi * 3 * x) * np.sin(2 * np.pi * 2 * y)
    hy = 0.6 * np.sin(2 * np.pi * 3 * x) * np.cos(2 * np.pi * 2 * y)
    nrm = np.stack([-hx, -hy, np.ones_like(hx)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    write_ppm(os.path.join(SCENES, "inputs", "normalmap.ppm"), np.clip(np.round((nrm + 1) * 127.5), 0, 255))
    # bump map: rings + a seeded speckle, grey in all three channels with a colour tint
    rng = np.random.default_rng(1234)
    r = np.hypot(x - 0.5, y - 0.5)
    hgt = 128 + 90 * np.sin(2 * np.pi * 6 * r) + rng.integers(-20, 21, size=(n, n))
    bump = np.stack([hgt, hgt * 0.9, hgt * 1.1], -1)
    write_ppm(os.path.join(SCENES, "inputs", "bumpmap.ppm"), np.clip(np.round(bump), 0, 255))
    xml = """<Scene>
    <MaxRecursionDepth>1</MaxRecursionDepth>
    <BackgroundColor>20 20 30</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>0 4 10</Position>
            <Gaze>0 -0.35 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-0.8 0.8 -0.6 0.6</NearPlane>
            <NearDistance>1.2</NearDistance>
            <ImageResolution>200 150</ImageResolution>
            <ImageName>bump_normal.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>20 20 20</AmbientLight>
        <PointLight id="1">
            <Position>3 7 6</Position>
            <Intensity>2000 2000 2000</Intensity>
        </PointLight>
        <PointLight id="2">
            <Position>-5 3 2</Position>
            <Intensity>600 500 400</Intensity>
        </PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>0.3 0.3 0.3</AmbientReflectance>
            <DiffuseReflectance>0.7 0.7 0.7</DiffuseReflectance>
            <SpecularReflectance>0.5 0.5 0.5</SpecularReflectance>
            <PhongExponent>30</PhongExponent>
        </Material>
        <Material id="2">
            <AmbientReflectance>0.2 0.2 0.3</AmbientReflectance>
            <DiffuseReflectance>0.3 0.5 0.9</DiffuseReflectance>
            <SpecularReflectance>0.6 0.6 0.6</SpecularReflectance>
            <PhongExponent>40</PhongExponent>
        </Material>
        <Material id="3" type="mirror">
            <AmbientReflectance>0.05 0.05 0.05</AmbientReflectance>
            <DiffuseReflectance>0.2 0.1 0.1</DiffuseReflectance>
            <SpecularReflectance>0.2 0.2 0.2</SpecularReflectance>
            <MirrorReflectance>0.6 0.6 0.6</MirrorReflectance>
        </Material>
    </Materials>
    <Textures>
        <Images>
            <Image id="1">normalmap.ppm</Image>
            <Image id="2">bumpmap.ppm</Image>
        </Images>
        <TextureMap id="1" type="image">
            <ImageId>1</ImageId>
            <DecalMode>replace_normal</DecalMode>
            <Interpolation>nearest</Interpolation>
        </TextureMap>
        <TextureMap id="2" type="image">
            <ImageId>2</ImageId>
            <DecalMode>bump_normal</DecalMode>
            <BumpFactor>0.02</BumpFactor>
        </TextureMap>
        <TextureMap id="3" type="perlin">
            <DecalMode>bump_normal</DecalMode>
            <NoiseConversion>absval</NoiseConversion>
            <NoiseScale>3</NoiseScale>
            <BumpFactor>0.4</BumpFactor>
        </TextureMap>
        <TextureMap id="4" type="image">
            <ImageId>2</ImageId>
            <DecalMode>bump_normal</DecalMode>
            <Normalizer>200</Normalizer>
            <BumpFactor>3</BumpFactor>
        </TextureMap>
        <TextureMap id="5" type="perlin">
            <DecalMode>bump_normal</DecalMode>
            <NoiseConversion>linear</NoiseConversion>
            <NoiseScale>4</NoiseScale>
        </TextureMap>
        <TextureMap id="6" type="image">
            <ImageId>1</ImageId>
            <DecalMode>replace_normal</DecalMode>
            <Interpolation>bilinear</Interpolation>
        </TextureMap>
    </Textures>
    <VertexData>
        -6 0 -6
        6 0 -6
        6 0 6
        -6 0 6
        -0.5 -0.5 -0.5
        0.5 -0.5 -0.5
        0.5 0.5 -0.5
        -0.5 0.5 -0.5
        -0.5 -0.5 0.5
        0.5 -0.5 0.5
        0.5 0.5 0.5
        -0.5 0.5 0.5
        2.5 0.2 2.0
        4.0 0.2 2.5
        3.2 2.0 2.2
        0 1 0
    </VertexData>
    <TexCoordData>
        0 0
        3 0
        3 3
        0 3
        0 0
        1 0
        1 1
        0 1
        0.1 0.1
        0.9 0.1
        0.9 0.9
        0.1 0.9
        0 0
        1 0
        0.5 1
        0 0
    </TexCoordData>
    <Transformations>
        <Translation id="1">0 0.01 0</Translation>
        <Translation id="2">-2.5 0.9 0</Translation>
        <Translation id="3">2.2 0.9 -1.5</Translation>
        <Translation id="4">0 0.2 1.8</Translation>
        <Scaling id="1">1.2 1 1.2</Scaling>
        <Scaling id="2">0.8 1.3 0.8</Scaling>
        <Scaling id="3">1.5 1.5 1.5</Scaling>
        <Rotation id="1">30 0 1 0</Rotation>
        <Rotation id="2">-25 1 0 0</Rotation>
        <Rotation id="3">40 0 0 1</Rotation>
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Textures>1</Textures>
            <Transformations>s1 t1</Transformations>
            <Faces>
                1 3 2
                1 4 3
            </Faces>
        </Mesh>
        <Mesh id="2">
            <Material>2</Material>
            <Textures>2</Textures>
            <Transformations>s3 r1 t2</Transformations>
            <Faces>
                5 7 6
                5 8 7
                9 10 11
                9 11 12
                5 6 10
                5 10 9
                8 12 11
                8 11 7
                5 9 12
                5 12 8
                6 7 11
                6 11 10
            </Faces>
        </Mesh>
        <MeshInstance id="10" baseMeshId="2">
            <Material>1</Material>
            <Transformations>r2 t3</Transformations>
        </MeshInstance>
        <MeshInstance id="11" baseMeshId="2" resetTransform="true">
            <Material>3</Material>
            <Transformations>s2 r3 t4</Transformations>
        </MeshInstance>
        <Mesh id="3">
            <Material>2</Material>
            <Textures>6</Textures>
            <Transformations>r3 t4</Transformations>
            <Faces>
                9 10 11
                9 11 12
            </Faces>
        </Mesh>
        <Triangle id="1">
            <Material>1</Material>
            <Textures>3</Textures>
            <Indices>13 14 15</Indices>
        </Triangle>
        <Sphere id="1">
            <Material>1</Material>
            <Textures>4</Textures>
            <Center>16</Center>
            <Radius>0.8</Radius>
            <Transformations>s2 t3</Transformations>
        </Sphere>
        <Sphere id="2">
            <Material>2</Material>
            <Textures>5</Textures>
            <Center>16</Center>
            <Radius>0.6</Radius>
            <Transformations>t2 t1</Transformations>
        </Sphere>
    </Objects>
</Scene>
"""
    with open(os.path.join(SCENES, "bump_normal.xml"), "w") as f:
        f.write(xml)


PT_BOX = """<Scene>
    <MaxRecursionDepth>DEPTH</MaxRecursionDepth>
    <BackgroundColor>0 0 0</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>0 0 7.5</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -1 1</NearPlane>
            <NearDistance>2.5</NearDistance>
            <ImageResolution>64 64</ImageResolution>
            <ImageName>NAME.png</ImageName>
            <Renderer>PathTracing</Renderer>
            <RendererParams>PARAMS</RendererParams>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>5 5 5</AmbientLight>
        LIGHTS
    </Lights>
    <BRDFs>
        <OriginalBlinnPhong id="1">
            <Exponent>30</Exponent>
        </OriginalBlinnPhong>
        <TorranceSparrow id="2" kdfresnel="true">
            <Exponent>40</Exponent>
        </TorranceSparrow>
    </BRDFs>
    <Materials>
        <Material id="1">
            <AmbientReflectance>0.2 0.2 0.2</AmbientReflectance>
            <DiffuseReflectance>KD1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
        <Material id="2">
            <AmbientReflectance>0.2 0.05 0.05</AmbientReflectance>
            <DiffuseReflectance>0.7 0.15 0.15</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
        </Material>
        <Material id="3">
            <AmbientReflectance>0.05 0.2 0.05</AmbientReflectance>
            <DiffuseReflectance>0.15 0.7 0.15</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
        </Material>
        <Material id="4" BRDF="1">
            <AmbientReflectance>0.1 0.1 0.2</AmbientReflectance>
            <DiffuseReflectance>0.3 0.4 0.8</DiffuseReflectance>
            <SpecularReflectance>0.4 0.4 0.4</SpecularReflectance>
        </Material>
        <Material id="5" type="mirror">
            <AmbientReflectance>0 0 0</AmbientReflectance>
            <DiffuseReflectance>0.1 0.1 0.1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <MirrorReflectance>0.8 0.8 0.8</MirrorReflectance>
        </Material>
        <Material id="6" BRDF="2">
            <AmbientReflectance>0.2 0.2 0.1</AmbientReflectance>
            <DiffuseReflectance>0.8 0.6 0.3</DiffuseReflectance>
            <SpecularReflectance>0.5 0.5 0.5</SpecularReflectance>
            <RefractionIndex>1.5</RefractionIndex>
        </Material>
        <Material id="7">
            <AmbientReflectance>0 0 0</AmbientReflectance>
            <DiffuseReflectance>0 0 0</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
        </Material>
    </Materials>
    <VertexData>
        -2 -2 2
        2 -2 2
        2 -2 -2
        -2 -2 -2
        -2 2 2
        2 2 2
        2 2 -2
        -2 2 -2
        -0.7 1.99 0.7
        0.7 1.99 0.7
        0.7 1.99 -0.7
        -0.7 1.99 -0.7
        SPH1
        SPH2
    </VertexData>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
                1 2 3
                1 3 4
                BACK
                CEILING
            </Faces>
        </Mesh>
        WALLS
        LIGHTMESH
        <Sphere id="1">
            <Material>SPHMAT</Material>
            <Center>13</Center>
            <Radius>0.8</Radius>
        </Sphere>
        <Sphere id="2">
            <Material>6</Material>
            <Center>14</Center>
            <Radius>0.7</Radius>
        </Sphere>
    </Objects>
</Scene>
"""
PT_WALLS = """<Mesh id="2">
            <Material>2</Material>
            <Faces>
                1 4 8
                1 8 5
            </Faces>
        </Mesh>
        <Mesh id="3">
            <Material>3</Material>
            <Faces>
                2 6 7
                2 7 3
            </Faces>
        </Mesh>"""
PT_SCENES = {
    # path tracing without next-event estimation: the LightMesh is only reached by GI rays
    # (SampleDirectLighting -- and so the reference's out-of-range face draw -- never runs)
    "pt_cornell": dict(DEPTH="3", PARAMS="ImportanceSampling", LIGHTS="", SPHMAT="4", CEILING="5 7 6\n5 8 7",
                       BACK="4 3 7\n4 7 8", WALLS=PT_WALLS,
                       LIGHTMESH="""<LightMesh id="4">
            <Material>7</Material>
            <Radiance>12 12 12</Radiance>
            <Faces>
                9 11 10
                9 12 11
            </Faces>
        </LightMesh>"""),
    # next-event estimation + uniform hemisphere sampling, point and area lights, a mirror
    # sphere (its GI and mirror children), an open box
    "pt_nee": dict(DEPTH="2", PARAMS="NextEventEstimation", SPHMAT="5", CEILING="", LIGHTMESH="",
                   BACK="4 3 7\n4 7 8", WALLS=PT_WALLS,
                   LIGHTS="""<PointLight id="1">
            <Position>0 1.5 1</Position>
            <Intensity>60 60 60</Intensity>
        </PointLight>
        <AreaLight id="1">
            <Position>0 1.9 -0.5</Position>
            <Normal>0 -1 0</Normal>
            <Radiance>30 30 30</Radiance>
            <Size>1</Size>
        </AreaLight>"""),
    # Russian roulette (+ NEE, importance sampling) over a floor only: every bounce multiplies
    # by ~pi*kd > 1 in the reference's estimator and RR never ends a diffuse chain (the
    # throughput it tests is renormalised each bounce), so only a scene GI rays mostly
    # escape has a finite mean to compare
    "pt_rr": dict(DEPTH="1", PARAMS="NextEventEstimation RussianRoulette ImportanceSampling", SPHMAT="5",
                  CEILING="", LIGHTMESH="", BACK="", WALLS="", KD1="0.2 0.2 0.2", SPH1="-0.8 -0.6 -0.6",
                  SPH2="0.9 -0.5 0.4",
                  LIGHTS="""<PointLight id="1">
            <Position>1 2.5 2</Position>
            <Intensity>1500 1500 1500</Intensity>
        </PointLight>"""),
}


# Scenes with no reference golden: next-event estimation over a LightMesh runs
# MeshLight::getSample, whose uniform_int_distribution(0, faceCount) reads one face past
# the end of the face vector in 1 draw of faceCount+1 (undefined behaviour, meshLight.h:22)
# -- these are checked GPU == oracle only ("parity unpinned" against the reference).
PT_SCENES["mesh_light"] = dict(DEPTH="1", PARAMS="", SPHMAT="4", CEILING="5 7 6\n5 8 7", BACK="4 3 7\n4 7 8",
                               WALLS=PT_WALLS, LIGHTS="", LIGHTMESH=PT_SCENES["pt_cornell"]["LIGHTMESH"])
PT_SCENES["pt_meshlight"] = dict(PT_SCENES["mesh_light"], DEPTH="2",
                                 PARAMS="NextEventEstimation ImportanceSampling")
ORACLE_ONLY = ("mesh_light", "pt_meshlight")


def make_pt(name):
    xml = PT_BOX.replace("NAME", name)
    if not PT_SCENES[name]["PARAMS"]:      # a classic (Whitted) camera
        xml = xml.replace("            <Renderer>PathTracing</Renderer>\n            <RendererParams>PARAMS</RendererParams>\n", "")
    opts = dict(KD1="0.7 0.7 0.7", SPH1="-0.8 -1.2 -0.6", SPH2="0.9 -1.3 0.4")
    opts.update(PT_SCENES[name])
    for k, v in opts.items():
        xml = xml.replace(k, v)
    with open(os.path.join(SCENES, name + ".xml"), "w") as f:
        f.write(xml)


def dump_avg(name, n):
    """Per-pixel mean of n RenderPixel calls and the variance of that mean (refdriver dumpavg)."""
    out = os.path.join(HERE, name + ".bin")
    subprocess.run([DRIVER, "dumpavg", name + ".xml", out, str(n)], cwd=SCENES, check=True, stdout=subprocess.DEVNULL)
    raw = open(out, "rb").read()
    os.remove(out)
    assert raw[:4] == b"RTGV"
    w, h, nn = np.frombuffer(raw[4:16], np.int32)
    body = np.frombuffer(raw[16:], np.float32).reshape(2, h, w, 3)
    return body[0].copy(), body[1].copy(), int(nn)


def prepare(name, src, w, h, edits):
    dst = os.path.join(SCENES, name + ".xml")
    if src == "generated":
        if name == "synth_10k":
            gen.synthetic_heightfield(SCENES, K=10082, width=w, height=h, name="synth_10k")
        elif name == "ply_quads":
            make_ply_quads()
        elif name == "bump_normal":
            make_bump_normal()
        elif name == "image_tex":
            make_image_tex()
        elif name in PT_SCENES:
            make_pt(name)
        elif name == "c2_cornell":
            gen.config_c2(SCENES, os.path.join(SCENES, "cornell_conductors.xml"), w, h)
        elif name == "c3_blob":
            gen.config_c3(SCENES, K=12000, width=w, height=h, spp=1)
        elif name == "c5_dragon":
            gen.config_c5(SCENES, K=30000, width=w, height=h, spp=1)
        elif name.startswith("deep_"):
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import variant_scenes
            assert (variant_scenes.DEEP[name]["width"], variant_scenes.DEEP[name]["height"]) == (w, h)
            variant_scenes.write_deep(SCENES, name)
        return dst
    if src == "authored":
        gen.with_resolution(dst, dst, w, h)
        return dst
    s = open(src).read()
    if edits == "drop_first_camera":
        a = s.index("<Camera ")
        b = s.index("</Camera>", a) + len("</Camera>")
        s = s[:a] + s[b:]
        edits = None
    for a, b in edits or []:
        assert a in s, (name, a)
        s = s.replace(a, b)
    # PLY assets next to the XML (parser.cpp:1404 opens them relative to the CWD)
    for ply in sorted(set(re.findall(r'plyFile="([^"]*)"', s))):
        dst_ply = os.path.join(SCENES, ply)
        if not os.path.exists(dst_ply):
            os.makedirs(os.path.dirname(dst_ply) or SCENES, exist_ok=True)
            shutil.copyfile(os.path.join(os.path.dirname(src), ply), dst_ply)
    s = re.sub(r"<ImageResolution>[^<]*</ImageResolution>", f"<ImageResolution>{w} {h}</ImageResolution>", s)
    with open(dst, "w") as f:
        f.write(s)
    return dst


def dump(name):
    out = os.path.join(HERE, name + ".bin")
    subprocess.run([DRIVER, "dump", name + ".xml", out], cwd=SCENES, check=True, stdout=subprocess.DEVNULL)
    raw = open(out, "rb").read()
    os.remove(out)
    assert raw[:4] == b"RTGF"
    w, h = np.frombuffer(raw[4:12], np.int32)
    return np.frombuffer(raw[12:], np.float32).reshape(h, w, 3).copy()


# Tonemapper goldens: the reference's own Tonemapper::Tonemap (refdriver tonemap) applied
# to golden float images, (key, burn %, saturation, gamma) per case.
TONEMAP_SOURCES = ("env_light", "brdf_lights", "c3_blob", "cornell_conductors")
TONEMAP_PARAMS = ((0.18, 1.0, 1.0, 2.2), (0.36, 0.0, 0.8, 2.0), (0.09, 5.0, 1.2, 1.8))


AVG_SAMPLES = 1024


def make_tonemap_goldens():
    out = {}
    for name in TONEMAP_SOURCES:
        hdr = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)["hdr"].astype(np.float32)
        h, w, _ = hdr.shape
        src = os.path.join(HERE, "_tm_in.bin")
        with open(src, "wb") as f:
            f.write(b"RTGF" + np.array([w, h], np.int32).tobytes() + hdr.tobytes())
        for k, (key, burn, sat, gamma) in enumerate(TONEMAP_PARAMS):
            dst = os.path.join(HERE, "_tm_out.bin")
            subprocess.run([DRIVER, "tonemap", src, str(key), str(burn), str(sat), str(gamma), dst], check=True,
                           stdout=subprocess.DEVNULL)
            raw = open(dst, "rb").read()
            assert raw[:4] == b"RTGL"
            out[f"{name}__{k}"] = np.frombuffer(raw[12:], np.uint8).reshape(h, w, 3).copy()
            os.remove(dst)
        os.remove(src)
    np.savez_compressed(os.path.join(HERE, "tonemap.npz"), **out)
    with open(os.path.join(HERE, "tonemap.json"), "w") as f:
        json.dump({"sources": list(TONEMAP_SOURCES), "params": [list(p) for p in TONEMAP_PARAMS]}, f, indent=1)
    print("tonemap goldens", len(out))


# The stochastic 1-spp fixtures also get a statistical golden: the reference's per-pixel mean
# of AVG_SAMPLES RenderPixel calls and the variance of that mean (<name>_avg.npz), against
# which the oracle and the GPU are z-tested at many samples per pixel.
STOCH_AVG = ("area_light", "env_light", "dof_motion", "c3_blob")


def make_stoch_avg(names):
    man = {}
    for name in names:
        img, var, n = dump_avg(name, AVG_SAMPLES)
        np.savez_compressed(os.path.join(HERE, name + "_avg.npz"), hdr=img, var=var)
        man[name] = n
        print(name, "avg", img.shape, n)
    return man


# Edge-ray goldens (edge_rays_<scene>.npz): the rays of tests/edge_rays.py through the reference's
# own Shape::Intersect (refdriver rays), closest hit and occlusion.
EDGE_SCENES = ("simple", "spheres", "transforms_textures", "cornell_dielectric", "mesh_light", "dof_motion",
               "edge_lattice", "edge_roof")


def make_edge_lattice():
    """Dyadic geometry for the exact checks: two stacked 8x8 lattices of unit squares at integer
    coordinates, each square cut in two -- mesh 1 in the plane z = 1 over [-4, 4]^2, mesh 2 in
    z = -2 over [-9, -1]^2 (entirely negative: its boxes carry the FLT_MIN maxima) --, an instance
    of mesh 1 under a pure translation and a sphere at an integer centre."""
    verts, meshes = [], []
    for x0, y0, z in ((-4, -4, 1), (-9, -9, -2)):
        base = len(verts)
        verts += [(x0 + i, y0 + j, z) for j in range(9) for i in range(9)]
        tri = []
        for j in range(8):
            for i in range(8):
                a, b, c, d = (base + 1 + i + 9 * j, base + 2 + i + 9 * j, base + 2 + i + 9 * (j + 1),
                              base + 1 + i + 9 * (j + 1))
                tri += [f"{a} {b} {c}", f"{a} {c} {d}"]
        meshes.append(tri)
    verts.append((-6, 3, 3))
    vdata = "\n        ".join("%d %d %d" % v for v in verts)
    f1, f2 = ("\n                ".join(m) for m in meshes)
    xml = f"""<Scene>
    <MaxRecursionDepth>1</MaxRecursionDepth>
    <BackgroundColor>0 0 0</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>-2 -1 16</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>1</NearDistance>
            <ImageResolution>64 48</ImageResolution>
            <ImageName>edge_lattice.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>0 0 12</Position><Intensity>1000 1000 1000</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>1 1 1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
    </Materials>
    <VertexData>
        {vdata}
    </VertexData>
    <Transformations>
        <Translation id="1">3 -2 4</Translation>
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
                {f1}
            </Faces>
        </Mesh>
        <Mesh id="2">
            <Material>1</Material>
            <Faces>
                {f2}
            </Faces>
        </Mesh>
        <MeshInstance id="3" baseMeshId="1">
            <Material>1</Material>
            <Transformations>t1</Transformations>
        </MeshInstance>
        <Sphere id="1">
            <Material>1</Material>
            <Center>{len(verts)}</Center>
            <Radius>1</Radius>
        </Sphere>
    </Objects>
</Scene>
"""
    with open(os.path.join(SCENES, "edge_lattice.xml"), "w") as f:
        f.write(xml)


def make_edge_roof():
    """What edge_lattice cannot have: boxes with thickness on every axis around slanted faces.  A flat
    box is never "sure" in the fused slab test (tmax - tmin is 0), so the lattice's rays always take
    the exact branch under an instance; here an 8x8 height field over [-4, 4]^2 with integer heights
    0..3 -- leaf and inner boxes with planes at integer coordinates, 0 among them -- and an instance
    of it under the translation (3, 2, 4), whose inverse's last column is negative on all three
    axes, so that a -0 direction component survives the product into the instance's frame."""
    verts = [(i - 4, j - 4, (3 * i + 5 * j) % 4) for j in range(9) for i in range(9)]
    tri = []
    for j in range(8):
        for i in range(8):
            a, b, c, d = 1 + i + 9 * j, 2 + i + 9 * j, 2 + i + 9 * (j + 1), 1 + i + 9 * (j + 1)
            tri += [f"{a} {b} {c}", f"{a} {c} {d}"]
    vdata = "\n        ".join("%d %d %d" % v for v in verts)
    faces = "\n                ".join(tri)
    xml = f"""<Scene>
    <MaxRecursionDepth>1</MaxRecursionDepth>
    <BackgroundColor>0 0 0</BackgroundColor>
    <ShadowRayEpsilon>1e-3</ShadowRayEpsilon>
    <Cameras>
        <Camera id="1">
            <Position>1 1 20</Position>
            <Gaze>0 0 -1</Gaze>
            <Up>0 1 0</Up>
            <NearPlane>-1 1 -0.75 0.75</NearPlane>
            <NearDistance>1.5</NearDistance>
            <ImageResolution>64 48</ImageResolution>
            <ImageName>edge_roof.png</ImageName>
        </Camera>
    </Cameras>
    <Lights>
        <AmbientLight>25 25 25</AmbientLight>
        <PointLight id="1"><Position>0 0 15</Position><Intensity>1000 1000 1000</Intensity></PointLight>
    </Lights>
    <Materials>
        <Material id="1">
            <AmbientReflectance>1 1 1</AmbientReflectance>
            <DiffuseReflectance>1 1 1</DiffuseReflectance>
            <SpecularReflectance>0 0 0</SpecularReflectance>
            <PhongExponent>1</PhongExponent>
        </Material>
    </Materials>
    <VertexData>
        {vdata}
    </VertexData>
    <Transformations>
        <Translation id="1">3 2 4</Translation>
    </Transformations>
    <Objects>
        <Mesh id="1">
            <Material>1</Material>
            <Faces>
                {faces}
            </Faces>
        </Mesh>
        <MeshInstance id="2" baseMeshId="1">
            <Material>1</Material>
            <Transformations>t1</Transformations>
        </MeshInstance>
    </Objects>
</Scene>
"""
    with open(os.path.join(SCENES, "edge_roof.xml"), "w") as f:
        f.write(xml)


def run_ref_rays(name, rays):
    """refdriver rays on scenes/<name>.xml: (hasHit, minT bits, loop position, occluded) int32
    (n, 4), or None when the reference does not return."""
    src, dst = os.path.join(HERE, "_rays_in.bin"), os.path.join(HERE, "_rays_out.bin")
    rays.tofile(src)
    try:
        rc = subprocess.run([DRIVER, "rays", name + ".xml", src, dst], cwd=SCENES, stdout=subprocess.DEVNULL,
                            timeout=600).returncode
        if rc != 0:
            return None
        raw = open(dst, "rb").read()
    except subprocess.TimeoutExpired:
        return None
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.remove(p)
    assert raw[:4] == b"RTGQ" and np.frombuffer(raw[4:8], np.int32)[0] == rays.size
    return np.frombuffer(raw[8:], np.int32).reshape(-1, 4).copy()


def make_edge_rays(names):
    """Generate the edge rays of each scene (tests/edge_rays.py on our own description of it), run
    the reference on them twice, and store rays, class labels and the reference's answers.  A class
    whose answers differ between the two runs is dropped and named; class G (non-finite rays) is
    stored only if the reference returns on it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_rays
    import query_util
    import rtgpu
    make_edge_lattice()
    make_edge_roof()
    for name in names:
        old = os.getcwd()
        os.chdir(SCENES)
        try:
            hs = rtgpu.HostScene(name + ".xml")
            # refdriver's shadow loop takes instances as not emissive (it cannot read their material):
            # its answers are the reference's only while no instance is
            objs = query_util.scene_arrays(hs)[1]
            inst = objs["kind"] == query_util.RTG_OBJ_INSTANCE
            assert not np.any(objs["flags"][inst] & query_util.RTG_OBJF_SHADOW_SKIP), (name, "emissive instance")
            rays, labels = edge_rays.generate(hs)
        finally:
            os.chdir(old)
        g = labels == edge_rays.CLASSES["G"]
        ans = np.zeros((rays.size, 4), np.int32)
        keep = np.ones(rays.size, bool)
        dropped = []
        for part in (~g, g):
            a, b = run_ref_rays(name, rays[part]), run_ref_rays(name, rays[part])
            if a is None or b is None:
                assert part is g, (name, "the reference failed on finite rays")
                keep &= ~part
                dropped.append("G (no return)")
                continue
            ans[part] = a
            for c in np.unique(labels[part]):
                sel = labels[part] == c
                if not np.array_equal(a[sel], b[sel]):
                    keep &= labels != c
                    dropped.append(edge_rays.NAMES[int(c)] + " (two runs differ)")
        np.savez_compressed(os.path.join(HERE, f"edge_rays_{name}.npz"), rays=rays[keep], labels=labels[keep],
                            has_hit=ans[keep, 0].astype(np.int8), t_bits=ans[keep, 1].view(np.uint32),
                            position=ans[keep, 2], occluded=ans[keep, 3].astype(np.int8))
        print("edge rays", name, int(keep.sum()), "dropped:", dropped or "none")


# Radiance-ray goldens (radiance_rays_<scene>.npz): the off-camera rays of tests/radiance_rays.py
# through the reference's own IntersectObjects / PerformShading (refdriver radiance), under both
# eyes.  The scenes whose render golden is `exact` and that between them cover the shading, and
# edge_roof for its instance.
RADIANCE_SCENES = ("simple", "spheres_mirror", "cornell_dielectric", "cornell_conductors", "brdf_lights", "image_tex",
                   "transforms_textures", "bump_normal", "scienceTree_diamond", "edge_roof", "deep_mirrors_9",
                   "deep_mirrors_32", "deep_glass_12")
RADIANCE_MAX_DROP = 0.01          # of a scene's rays; and no whole class
RADIANCE_MAX_BYTES = 64 * 1024


def run_ref_radiance(name, rays, ids, camera_eye):
    """refdriver radiance on scenes/<name>.xml: (n, 4) uint32 -- the bits of r, g, b and minT."""
    src, dst = os.path.join(HERE, "_rad_in.bin"), os.path.join(HERE, "_rad_out.bin")
    with open(src, "wb") as f:
        f.write(b"RTGR" + np.array([rays.size, int(camera_eye)], np.int32).tobytes() + rays.tobytes()
                + np.ascontiguousarray(ids, np.int32).tobytes())
    try:
        subprocess.run([DRIVER, "radiance", name + ".xml", src, dst], cwd=SCENES, check=True, stdout=subprocess.DEVNULL,
                       timeout=600)
        raw = open(dst, "rb").read()
    finally:
        for p in (src, dst):
            if os.path.exists(p):
                os.remove(p)
    assert raw[:4] == b"RTGC" and np.frombuffer(raw[4:8], np.int32)[0] == rays.size
    return np.frombuffer(raw[8:], np.uint32).reshape(-1, 4).copy()


def make_radiance_rays(names):
    """Generate each scene's rays (tests/radiance_rays.py on our own description of it), run the
    reference on them twice per eye (it reads an uninitialised material id for instances in
    CastShadowRay: see occluded() in ref_driver.cpp), drop the rays on which two runs differ -- a NaN
    equal to a NaN whatever its payload -- and store rays, ids, labels and the reference's colours:
    rgb_origin / rgb_camera (uint32 bits, eye = the ray's origin / the camera's position), t_bits
    (the same under both eyes), dropped (per class, in radiance_rays.CLASSES order)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import radiance_rays as rr
    import rtgpu
    make_edge_roof()
    for name in names:
        old = os.getcwd()
        os.chdir(SCENES)
        try:
            rays, ids, labels = rr.generate(rtgpu.HostScene(name + ".xml"))
        finally:
            os.chdir(old)

        def same(a, b):
            fa, fb = a.view(np.float32), b.view(np.float32)
            return ((a == b) | (np.isnan(fa) & np.isnan(fb))).all(1)

        runs = [[run_ref_radiance(name, rays, ids, eye) for _ in range(2)] for eye in (False, True)]
        keep = same(*runs[0]) & same(*runs[1]) & same(runs[0][0][:, 3:], runs[1][0][:, 3:])
        dropped = np.array([int((~keep & (labels == c)).sum()) for c in sorted(rr.NAMES)], np.int32)
        for c in sorted(rr.NAMES):
            assert not np.any(labels == c) or np.any(keep & (labels == c)), (name, "class lost", rr.NAMES[c])
        assert (~keep).sum() <= RADIANCE_MAX_DROP * rays.size, (name, "dropped", dropped)
        path = os.path.join(HERE, f"radiance_rays_{name}.npz")
        np.savez_compressed(path, rays=rays[keep], ids=ids[keep], labels=labels[keep],
                            rgb_origin=runs[0][0][keep, :3], rgb_camera=runs[1][0][keep, :3],
                            t_bits=runs[0][0][keep, 3], dropped=dropped)
        size = os.path.getsize(path)
        assert size <= RADIANCE_MAX_BYTES, (name, size)
        print("radiance rays", name, int(keep.sum()), "dropped per class", dropped.tolist(), "bytes", size)


# BVH goldens (bvh_<case>.npz): the BVH the reference's own parser builds (refdriver bvh) for the
# adversarial meshes of tests/bvh_cases.py.  Per mesh k: nodes<k> (n, 9) int32 -- box bits, left
# child, firstFace, faceCount in allocation order -- and faces<k> (n, 6) int32 -- centre bits and
# the three vertex ids, in final order; sha256: of the generated vertex and index bits
# (Case.vertex_sha256), so that a drifting generator fails loudly.  bvh_manifest.json lists the
# cases, their vertex hashes and the cases dropped (the reference crashed, or two runs differed).
BVH_MAX_BYTES = 256 * 1024


def run_ref_bvh(xml, cwd):
    """refdriver bvh: [(nodes (n, 9), faces (n, 6)) int32 per mesh], or None if it does not return."""
    dst = os.path.join(cwd, "_bvh_out.bin")
    try:
        rc = subprocess.run([DRIVER, "bvh", xml, dst], cwd=cwd, stdout=subprocess.DEVNULL, timeout=600).returncode
        if rc != 0:
            return None
        raw = np.frombuffer(open(dst, "rb").read(), np.int32)
    except subprocess.TimeoutExpired:
        return None
    finally:
        if os.path.exists(dst):
            os.remove(dst)
    assert raw[0] == np.frombuffer(b"RTGB", np.int32)[0]
    out, at = [], 2
    for _ in range(raw[1]):
        nn, nf = int(raw[at]), int(raw[at + 1])
        at += 2
        nodes = raw[at:at + 9 * nn].reshape(nn, 9).copy()
        at += 9 * nn
        faces = raw[at:at + 6 * nf].reshape(nf, 6).copy()
        at += 6 * nf
        out.append((nodes, faces))
    assert at == raw.size
    return out


def make_bvh(names=None):
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bvh_cases
    path = os.path.join(HERE, "bvh_manifest.json")
    man = json.load(open(path)) if names and os.path.exists(path) else {"cases": {}, "dropped": {}}
    for name in names or bvh_cases.NAMES:
        case = bvh_cases.get(name)
        man["cases"].pop(name, None)
        man["dropped"].pop(name, None)
        with tempfile.TemporaryDirectory() as d:
            bvh_cases.write_scene(case, d, name)
            a, b = run_ref_bvh(name + ".xml", d), run_ref_bvh(name + ".xml", d)
        if a is None or b is None:
            man["dropped"][name] = "the reference does not return"
        elif len(a) != len(b) or not all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q)):
            man["dropped"][name] = "two runs of the reference differ"
        if name in man["dropped"]:
            print("bvh", name, "dropped:", man["dropped"][name])
            continue
        assert len(a) == len(case.meshes)
        arrays = {"sha256": np.array(case.vertex_sha256())}
        for k, (nodes, faces) in enumerate(a):
            arrays[f"nodes{k}"], arrays[f"faces{k}"] = nodes, faces
        out = os.path.join(HERE, f"bvh_{name}.npz")
        np.savez_compressed(out, **arrays)
        size = os.path.getsize(out)
        assert size <= BVH_MAX_BYTES, (name, size)
        man["cases"][name] = {"sha256": case.vertex_sha256(), "meshes": len(a), "bytes": size}
        print("bvh", name, [(len(n), len(f)) for n, f in a], "bytes", size)
    with open(path, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


# Walk goldens (walk_rays_<case>.npz): the edge, aimed and light rays of tests/walk_cases.py on the
# adversarial meshes of tests/bvh_cases.py through the reference's own Shape::Intersect (refdriver
# rays), closest hit and occlusion.  rays, labels (walk_cases.SETS), index (the ray's position in
# walk_cases.ray_sets' output: a drifting generator fails loudly), has_hit, t_bits, position,
# occluded, sha256 (Case.vertex_sha256).  walk_rays_manifest.json lists the cases, what was
# dropped (a set whose two runs differ, or the whole case if the reference does not return) and how
# many rays the seeded subsample kept where all of them would exceed BVH_MAX_BYTES.
def run_ref_rays_in(cwd, xml, rays):
    """run_ref_rays on <cwd>/<xml>."""
    src, dst = os.path.join(cwd, "_rays_in.bin"), os.path.join(cwd, "_rays_out.bin")
    rays.tofile(src)
    try:
        rc = subprocess.run([DRIVER, "rays", xml, src, dst], cwd=cwd, stdout=subprocess.DEVNULL, timeout=600).returncode
        if rc != 0:
            return None
        raw = open(dst, "rb").read()
    except subprocess.TimeoutExpired:
        return None
    assert raw[:4] == b"RTGQ" and np.frombuffer(raw[4:8], np.int32)[0] == rays.size
    return np.frombuffer(raw[8:], np.int32).reshape(-1, 4).copy()


def make_walk_rays(names=None):
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_rays
    import walk_cases
    path = os.path.join(HERE, "walk_rays_manifest.json")
    man = json.load(open(path)) if names and os.path.exists(path) else {"cases": {}, "dropped": {}}
    for name in names or walk_cases.RECORDED:
        case = walk_cases.get(name)
        man["cases"].pop(name, None)
        man["dropped"].pop(name, None)
        with tempfile.TemporaryDirectory() as d:
            hs = walk_cases.load(d, name)
            rays, labels = walk_cases.ray_sets(hs, name)
            g = labels == edge_rays.CLASSES["G"]
            ans = np.zeros((rays.size, 4), np.int32)
            keep = np.ones(rays.size, bool)
            dropped = []
            for part in (~g, g):
                a, b = run_ref_rays_in(d, name + ".xml", rays[part]), run_ref_rays_in(d, name + ".xml", rays[part])
                if a is None or b is None:
                    keep &= ~part
                    dropped.append("G (no return)" if part is g else "every finite ray (no return)")
                    continue
                ans[part] = a
                for c in np.unique(labels[part]):
                    sel = labels[part] == c
                    if not np.array_equal(a[sel], b[sel]):
                        keep &= labels != c
                        dropped.append(walk_cases.SET_NAMES[int(c)] + " (two runs differ)")
        if not np.any(keep & ~g):
            man["dropped"][name] = "the reference does not return"
            print("walk rays", name, "dropped:", man["dropped"][name])
            continue
        # the edge rays whole; of the aimed and light rays a seeded choice that fits the size limit
        edge = np.flatnonzero(keep & (labels < walk_cases.SETS["aimed"]))
        rest = np.random.default_rng(20272).permutation(np.flatnonzero(keep & (labels >= walk_cases.SETS["aimed"])))
        out = os.path.join(HERE, f"walk_rays_{name}.npz")
        m = rest.size
        while True:
            idx = np.sort(np.concatenate([edge, rest[:m]]))
            np.savez_compressed(out, rays=rays[idx], labels=labels[idx], index=idx.astype(np.int32),
                                has_hit=ans[idx, 0].astype(np.int8), t_bits=ans[idx, 1].view(np.uint32),
                                position=ans[idx, 2], occluded=ans[idx, 3].astype(np.int8),
                                sha256=np.array(case.vertex_sha256()))
            size = os.path.getsize(out)
            if size <= BVH_MAX_BYTES:
                break
            assert m > 0, (name, size)
            m = int(m * 0.8 * BVH_MAX_BYTES / size)
        man["cases"][name] = {"sha256": case.vertex_sha256(), "rays": int(idx.size), "generated": int(rays.size),
                              "kept_of_aimed_and_light": [int(m), int(rest.size)], "dropped_sets": dropped, "bytes": size}
        print("walk rays", name, man["cases"][name])
    with open(path, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


def main():
    if not os.path.exists(DRIVER):
        sys.exit(f"{DRIVER} missing: build it with `make -C {os.path.join(ROOT, 'oracle')}` (needs /root/reference)")
    man = {}
    only = set(sys.argv[1:])
    if only and all(o == "walk_rays" or o.startswith("walk_rays_") for o in only):
        make_walk_rays(None if "walk_rays" in only else [o[len("walk_rays_"):] for o in sorted(only)])
        return
    if only and all(o == "bvh" or o.startswith("bvh_") for o in only):
        make_bvh(None if "bvh" in only else [o[len("bvh_"):] for o in sorted(only)])
        return
    if only and only <= {"radiance_rays"} | {"radiance_rays_" + n for n in RADIANCE_SCENES}:
        make_radiance_rays(RADIANCE_SCENES if "radiance_rays" in only else [o[len("radiance_rays_"):] for o in sorted(only)])
        return
    if only and only <= {"edge_rays"} | {"edge_rays_" + n for n in EDGE_SCENES}:
        make_edge_rays(EDGE_SCENES if "edge_rays" in only else [o[len("edge_rays_"):] for o in sorted(only)])
        return
    if only == {"tonemap"}:
        make_tonemap_goldens()
        return
    if only and only <= {n + "_avg" for n in STOCH_AVG}:
        path = os.path.join(HERE, "manifest.json")
        man = json.load(open(path))
        for name, n in make_stoch_avg([o[:-4] for o in sorted(only)]).items():
            man[name]["avg_samples"] = n
        with open(path, "w") as f:
            json.dump(man, f, indent=1, sort_keys=True)
        return
    for name in ORACLE_ONLY:
        if not only or name in only:
            make_pt(name)
    for name, (src, w, h, kind, edits) in FIXTURES.items():
        if only and name not in only:
            continue
        prepare(name, src, w, h, edits)
        extra = {}
        if kind == "stochastic_avg":
            img, var, n = dump_avg(name, AVG_SAMPLES)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), hdr=img, var=var)
            extra = {"samples": n}
        else:
            img = dump(name)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), hdr=img)
        man[name] = {"xml": f"scenes/{name}.xml", "width": int(img.shape[1]), "height": int(img.shape[0]),
                     "kind": kind, "source": src if src.startswith("/") else src,
                     "sha256": hashlib.sha256(img.tobytes()).hexdigest(), **extra}
        print(name, img.shape, kind)
    path = os.path.join(HERE, "manifest.json")
    if only and os.path.exists(path):
        old = json.load(open(path))
        old.update(man)
        man = old
    with open(path, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    if not only:
        make_edge_rays(EDGE_SCENES)
        make_radiance_rays(RADIANCE_SCENES)
        make_bvh()
        make_walk_rays()


if __name__ == "__main__":
    main()
