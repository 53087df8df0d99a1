"""Helpers of the surface-query tests (test_surface_abi.py, test_gpu_surface.py).  A helper module
like radiance_rays.py, not a conftest.

Two independent yardsticks for DeviceScene.surface():

  re-lighting   relit() rewrites a scene so that what the CPU oracle renders along a ray is a known
                function of the hit's shading normal, diffuse coefficient and position: no ambient
                light, no specular term, no mirror / dielectric / conductor / emissive materials,
                and three point lights of pure red, green and blue.  For a hit at p = o + d t with
                normal n and coefficient kd the oracle's channel c is then (raytracer.cpp:706-720,
                192-206 with ks = 0)

                    kd_c * max(0, n . w_c) * I / |L_c - p|^2,   w_c = unit(L_c - p),

                or 0 where the shadow ray (origin p + n * ShadowRayEpsilon, direction w_c,
                tmax = |L_c - p|) is occluded -- HostScene.trace(any_hit=True) answers that.  Three
                light positions pin all three components of n; kd pins uv and the texture path.
                predict() evaluates the formula; compare_relit() counts.

  uv            expected_uv() recomputes the texture coordinates in float64 from the description:
                the ray through the object's inv_transform, Moeller-Trumbore barycentrics on the
                face's vertices and its uv through tiledUV for meshes, the spherical mapping for
                spheres.
"""
import re

import numpy as np

import query_util as qu
import radiance_rays as rr
import rtgpu

f32 = np.float32
# the bounds of the issue that introduced the queries: the project's parity figure applied relatively
# to lit values (4x the worst deviation measured along the reference chain), and the share of a
# scene's values per channel that may miss it or disagree about lit / not lit
REL = 1e-4
CAP = 1e-3
UV_REL = 1e-4                 # |d| <= UV_REL * max(1, |value|): the project's parity bound
UV_WRAP = 1e-3                # rays this close to a tiledUV wrap or to the sphere's seam are left out
# ... and rays on which a float64 recomputation is no yardstick for float32 arithmetic, because the
# mapping is singular there.  A sphere's azimuth has the condition number 1 / sin(theta): within
# UV_WRAP of a pole the roundings of p.x and p.z (both cancel to nearly 0) decide phi.  A face's
# barycentrics are quotients by det = -d . (e1 x e2): their float32 error is about
# 2^-24 |s| |e| / |det|, which grows as 1 / cos of the angle between the ray and the face's normal and is
# unbounded for a ray in the face's plane (radiance_rays' classes S and B aim such rays on purpose).
UV_POLE = 1e-3                # sin(theta) below this: left out
UV_GRAZE = 1e-2               # |cos(ray, face normal)| below this (0.57 degrees off the plane): left out
POLE_NAN = 1e-6               # |p.y| / r within this of 1: the reference's acos may see an argument above 1
UV_EXCLUDED_CAP = 0.02
TEX_DIFFUSE, TEX_SPECULAR, TEX_NORMAL, TEX_BUMP, TEX_REPLACE_ALL = range(5)      # rtg_object's tex_* order


def materials(hs):
    d = qu.Desc.from_address(hs.desc)
    return qu._array(d.materials, d.num_materials, rr.MAT_DTYPE)


def material_diffuse(hs):
    """(num_materials, 3) float32 DiffuseReflectance (rtg_material: ambient, then diffuse)."""
    return np.ascontiguousarray(materials(hs)["f"][:, 3:6])


def shadow_epsilon(hs):
    return f32(qu.Desc.from_address(hs.desc).shadow_epsilon)


# ---- re-lighting
def light_setup(eye, median_t):
    """The three lights of the issue: red at the rays' common origin, green at E + s (1, 0.5, 0), blue at
    E + s (-0.5, 1, 0) with s a third of the median hit distance; intensity median_t^2 so that lit values
    are of order 1.  Returns [(position float32[3], intensity float32[3])] in channel order."""
    eye = np.asarray(eye, f32)
    s = f32(median_t / 3.0)
    I = f32(median_t * median_t)
    offs = (np.zeros(3, f32), np.array([1, 0.5, 0], f32) * s, np.array([-0.5, 1, 0], f32) * s)
    return [((eye + off).astype(f32), np.eye(3, dtype=f32)[c] * I) for c, off in enumerate(offs)]


def relit(xml_text, lights):
    """`xml_text` with its <Lights> block replaced by AmbientLight 0 0 0 and the given point lights,
    every SpecularReflectance set to 0 and every material's type= attribute removed."""
    fmt = lambda v: " ".join(repr(float(x)) for x in v)
    block = ["<Lights>", "        <AmbientLight>0 0 0</AmbientLight>"]
    for k, (pos, inten) in enumerate(lights):
        block += ['        <PointLight id="%d">' % (k + 1), "            <Position>%s</Position>" % fmt(pos),
                  "            <Intensity>%s</Intensity>" % fmt(inten), "        </PointLight>"]
    block.append("    </Lights>")
    text, n = re.subn(r"<Lights>.*?</Lights>", lambda m: "\n".join(block), xml_text, count=1, flags=re.S)
    assert n == 1, "no <Lights> block"
    text = re.sub(r"<SpecularReflectance>[^<]*</SpecularReflectance>", "<SpecularReflectance>0 0 0</SpecularReflectance>", text)
    text = re.sub(r"(<Material\b[^>]*?)\s+type\s*=\s*\"[^\"]*\"", r"\1", text)
    assert not re.search(r"<Material\b[^>]*\btype\s*=", text)
    return text


def predict(hs, rays, t, n, kd, lights):
    """The colour the relit scene's render gives each hit: (m, 3) float64, computed from the hit
    distance t, normal n (m, 3) and coefficient kd (m, 3) as given (float32) and `hs`'s own occlusion.
    The point and the shadow ray are formed in float32 as the renderer forms them; the rest in float64."""
    o, d = qu.origins(rays), qu.directions(rays)
    t, n, kd = np.asarray(t, f32), np.asarray(n, f32), np.asarray(kd, f32)
    p = (o + d * t[:, None]).astype(f32)
    eps = shadow_epsilon(hs)
    so = (p + n * eps).astype(f32)
    out = np.zeros((len(p), 3))
    for c, (pos, inten) in enumerate(lights):
        to = (np.asarray(pos, f32)[None] - p).astype(f32)
        dist = np.sqrt((to * to).sum(1, dtype=f32)).astype(f32)
        w = (to / dist[:, None]).astype(f32)
        occ = hs.trace(rtgpu.make_rays(so, w, tmax=dist), any_hit=True)["object"] >= 0
        to64 = np.asarray(pos, np.float64)[None] - p.astype(np.float64)
        d2 = (to64 * to64).sum(1)
        cos = (n.astype(np.float64) * to64).sum(1) / np.sqrt(d2)
        val = kd[:, c].astype(np.float64) * np.maximum(cos, 0.0) * float(inten[c]) / d2
        out[:, c] = np.where(occ, 0.0, val)
    return out


def compare_relit(got, want):
    """Per channel of (m, 3) oracle colours `got` against predictions `want`: a value is lit where it is
    > 0.  Returns a dict of per-channel lists: lit (both sides), outside (lit values with
    |got - want| > REL |got|), disagree (lit on one side only), max_rel (over lit values), and m."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    res = {"m": len(got), "lit": [], "outside": [], "disagree": [], "max_rel": []}
    for c in range(3):
        lg, lw = got[:, c] > 0, want[:, c] > 0
        both = lg & lw
        rel = np.abs(got[both, c] - want[both, c]) / np.abs(got[both, c])
        res["lit"].append(int(both.sum()))
        res["outside"].append(int((rel > REL).sum()))
        res["disagree"].append(int((lg != lw).sum()))
        res["max_rel"].append(float(rel.max()) if rel.size else 0.0)
    return res


def relit_ok(res):
    """The issue's conditions on compare_relit's counts."""
    return all(res["outside"][c] <= CAP * res["lit"][c] and res["disagree"][c] <= CAP * res["m"] for c in range(3))


def shaded_by_formula(hs):
    """Per object: True where the relit render's colour is the diffuse formula above.  Not so for
    replace_all objects (PerformShading returns the texture sample, raytracer.cpp:87-89) and for
    objects whose specular coefficient is read from a texture (GetSpecular with a replace_ks and a
    diffuse texture, raytracer.cpp:509-539: relit()'s SpecularReflectance 0 does not reach it)."""
    objs = qu.scene_arrays(hs)[1]
    tex = objs["tex"]
    return ~((tex[:, TEX_REPLACE_ALL] >= 0) | ((tex[:, TEX_SPECULAR] >= 0) & (tex[:, TEX_DIFFUSE] >= 0)))


# ---- uv
def _tiled(x):
    """tiledUV (mesh.cpp:382-389) in float64."""
    x = np.asarray(x, np.float64).copy()
    big = x > 1.0001
    fr = x - np.floor(x)
    fr = np.where(fr < 0.0001, 1.0, fr)
    return np.where(big, fr, x)


def _near_wrap(x):
    """Raw coordinates within UV_WRAP of a tiledUV wrap: 1.0001, or an integer above it."""
    x = np.asarray(x, np.float64)
    return (np.abs(x - 1.0001) < UV_WRAP) | ((x > 1.0001 - UV_WRAP) & (np.abs(x - np.round(x)) < UV_WRAP) & (np.round(x) >= 1))


def expected_uv(hs, rays, surf):
    """(uv (n, 2) float64, valid bool, excluded bool) for surface() results `surf` of `rays`: the
    texture coordinates recomputed in float64.  valid: hits on meshes with UVs and on spheres, of
    objects without motion blur; excluded: valid rays near a wrap or the sphere's seam."""
    _, objs, meshes, faces = qu.scene_arrays(hs)
    n = rays.size
    uv = np.zeros((n, 2))
    valid = np.zeros(n, bool)
    excluded = np.zeros(n, bool)
    o = qu.origins(rays).astype(np.float64)
    d = qu.directions(rays).astype(np.float64)
    for k, ob in enumerate(objs):
        sel = np.flatnonzero(surf["object"] == k)
        if not sel.size or np.any(ob["motion_blur"]):
            continue
        M = ob["inv_transform"].reshape(4, 4)
        lo = o[sel] @ M[:3, :3].T + M[:3, 3]
        ld = d[sel] @ M[:3, :3].T
        if ob["kind"] == qu.RTG_OBJ_SPHERE:
            p = lo + ld * surf["t"][sel].astype(np.float64)[:, None] - ob["center"].astype(np.float64)
            phi = np.arctan2(p[:, 2], p[:, 0])
            theta = np.arccos(np.clip(p[:, 1] / float(ob["radius"]), -1.0, 1.0))
            uv[sel, 0] = (-phi + np.pi) / (2.0 * np.pi)
            uv[sel, 1] = theta / np.pi
            valid[sel] = True
            excluded[sel] = (np.abs(np.abs(phi) - np.pi) < UV_WRAP) | (np.sin(theta) < UV_POLE)
            continue
        if not meshes[ob["mesh"]]["has_uv"]:
            continue
        F = faces[surf["face"][sel]]
        v0, v1, v2 = (F[x].astype(np.float64) for x in ("v0", "v1", "v2"))
        e1, e2 = v1 - v0, v2 - v0
        pv = np.cross(ld, e2)
        det = (pv * e1).sum(1)
        s = lo - v0
        beta = (s * pv).sum(1) / det
        gamma = (ld * np.cross(s, e1)).sum(1) / det
        t0, t1, t2 = (F["uv"][:, 2 * j:2 * j + 2].astype(np.float64) for j in range(3))
        raw = t0 + beta[:, None] * (t1 - t0) + gamma[:, None] * (t2 - t0)
        uv[sel] = _tiled(raw)
        valid[sel] = True
        nf = np.cross(e1, e2)
        cos = np.abs((ld * nf).sum(1)) / (np.linalg.norm(ld, axis=1) * np.linalg.norm(nf, axis=1))
        excluded[sel] = _near_wrap(raw).any(1) | (cos < UV_GRAZE)
    return uv, valid, excluded & valid


def sphere_poles(hs, rays, surf):
    """Hits on a sphere within POLE_NAN of a pole (|p.y| / r >= 1 - POLE_NAN in float64).  There the
    reference's theta = acos(p.y / r) can meet an argument above 1 in float32 and give NaN -- for v,
    and for a bumped sphere's normal, whose tangents are built from sin(theta) (sphere.cpp:71-193).
    The device repeats that arithmetic, as the render does."""
    objs = qu.scene_arrays(hs)[1]
    out = np.zeros(rays.size, bool)
    o = qu.origins(rays).astype(np.float64)
    d = qu.directions(rays).astype(np.float64)
    for k, ob in enumerate(objs):
        sel = np.flatnonzero(surf["object"] == k)
        if not sel.size or ob["kind"] != qu.RTG_OBJ_SPHERE or np.any(ob["motion_blur"]):
            continue
        M = ob["inv_transform"].reshape(4, 4)
        lo = o[sel] @ M[:3, :3].T + M[:3, 3]
        p = lo + (d[sel] @ M[:3, :3].T) * surf["t"][sel].astype(np.float64)[:, None] - ob["center"].astype(np.float64)
        out[sel] = np.abs(p[:, 1]) / float(ob["radius"]) >= 1.0 - POLE_NAN
    return out
