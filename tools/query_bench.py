#!/usr/bin/env python3
"""Ray-query throughput on the headline height field (scenes.synthetic_heightfield, K = 100 352,
1920x1080): the 2 073 600 camera rays generated on the device, then, timed with HIP events
around --launches launches each, in --reps interleaved repetitions after a warm-up,

  (a) closest hit with RTG_QUERY_COHERENT        (b) closest hit without the hint
  (c) the same rays randomly permuted (no hint; c+hint: with it)
  (d) occlusion of the shadow rays' equivalent: from the hit points towards the scene's light
  (a-tiled) as (a) with the rays in k_primary's order (a wave = an 8x8 pixel tile, not a 64x1 strip)

and, from the same session, the render's own kernels (rtg_scene_timings of RTG_RENDER_TIMING
renders: RTG_FRAME_KERNEL=0 splits the sample pass into k_primary + k_shade_shadow;
RTG_RENDER_EXACT_SHADOW gives k_shadow with the reference walk).  k_primary is the yardstick of
(a): the same walk on the same rays, with a 32-byte ray read in place of ray generation.

    python tools/query_bench.py [--launches 50] [--reps 3] [--out FILE] [--sections query,radiance,surface,update,multi,closest,crossings,sdf]

The radiance section (rtg_radiance_rays_device, DeviceScene.radiance_device) runs on the same
height field and on the path-tracing fixture tests/golden/scenes/pt_cornell.xml at its own size:
the camera's rays, generated on the device, shaded

  (r)  in pixel order    (r-tiled) in k_primary's 8x8-tile order, pixel ids alongside
  (r-perm) randomly permuted, pixel ids alongside
  (r-tiled general) as (r-tiled) with RTG_MEGA_GENERAL=1: the SK_ALL / FEAT_ALL instantiation

against the yardstick of the same session: stage k_render of RTG_RENDER_FUSED | RTG_RENDER_TIMING
renders -- the same ray trees, with ray generation in place of a 32-byte load.

The surface section (rtg_surface_rays_device, DeviceScene.surface_device) runs on the same height
field and on the textured fixture tests/golden/scenes/transforms_textures.xml (its camera's rays
repeated to about a million, so that a launch is not all launch overhead): the camera's rays in
k_primary's 8x8-tile order and in pixel order, with and without the hint,

  (s)  surface_device: 64 B per ray out        (t)  trace_device with normals: 32 B per ray out

on the same rays in the same session; the ratio (s) / (t) is the figure to read.

The update section (rtg_scene_update, rtg_scene_clone; DeviceScene.update / clone) runs on the same
height field and on a C4-style instanced scene (scenes.config_c4 at one sample), each with a variant
of the same geometry (light moved; C4: a rotation and a translation of the instances changed): the
wall-clock time of create, update, clone and clone + update as the median of --setups calls, and the
render time of the updated scene against a freshly created one, interleaved.

The multi section (rtg_trace_rays_multi_device, DeviceScene.trace_multi_device) runs on the same
height field: the k nearest hits for k = 1, 2, 4, 8 on the camera's rays in pixel order and on the
same rays randomly permuted, with trace_device (closest hit, no hint) on the same rays in the same
session beside them.

The closest section (rtg_closest_points_device, DeviceScene.closest_device) runs on the same height
field, about two million points a launch, in Gpoints/s:

  (g)  a jittered 512 x 512 x 8 grid through the box of the camera's hit points (its height that
       of the field plus a twentieth of its width), in grid order    (g-perm) the same, shuffled
  (h)  the camera rays' hit points lifted along the shading normal by 1e-3 to 1 (log-uniform)

each with max_dist = inf and with a radius of four mean cell sizes.  A 65 536-point sample of every
case is checked against the host walk bit for bit before anything is timed.  The library is the
one rtgpu loads ($RTGPU_LIB for an experiment's build, as in the seed-pass comparison of DESIGN.md).

The crossings section (rtg_count_crossings_device, DeviceScene.crossings_device) runs on the same
height field: the camera's unbounded rays, in pixel order and permuted, through crossings_device and
through trace_multi_device with k = 8 and counts.  All but a few hundred of the two million rays
(grazing ones near the horizon) hold fewer than 8 hits there, so on those both walks visit the same
boxes and the counts are equal (asserted; the others count at least 8); the condition is crossings
rate >= the k = 8 multi-hit rate of the same run.

The sdf section (rtg_signed_distance_points_device, DeviceScene.signed_distance_device) runs on the
closest section's grid (g) with dir = (0, 0, 1), unbounded and within four cells: the fused launch
against closest_device then crossings_device on the same points.  The condition is fused time <= the
sum of the two launches' times in the same run.
"""
import argparse
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "advanced-cpu-raytracing_amd"))

import numpy as np  # noqa: E402


def radiance_section(args, name, xml):
    """Timings of one scene: lines of text."""
    import torch

    import rtgpu

    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    cam = hs.camera(0)
    w, h = cam["width"], cam["height"]
    n = w * h
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ds.camera_rays_device(rays.data_ptr(), stream=st)
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(1234)
    perm = torch.randperm(n, generator=g)
    # k_primary's wave shape (rtg_frame.hpp tile_pixel): 64 consecutive rays = one 8x8 pixel tile
    assert w % 8 == 0 and h % 8 == 0
    yy, xx = np.divmod(np.arange(n), w)
    key = (yy // 8) * (w // 8) * 64 + (xx // 8) * 64 + (yy % 8) * 8 + (xx % 8)
    order = np.empty(n, np.int64)
    order[key] = np.arange(n)
    order = torch.from_numpy(order)
    sets = {"pixel": (rays, None)}
    for tag, idx in (("tiled", order), ("perm", perm)):
        sets[tag] = (rays[idx.to(dev)].contiguous(), idx.to(torch.int32).to(dev))
    cases = [("r  radiance, pixel order", "pixel", False), ("r-tiled radiance, 8x8 tiles", "tiled", False),
             ("r-perm radiance, permuted", "perm", False), ("r-tiled general instantiation", "tiled", True)]

    def run(which, general, k):
        buf, ids = sets[which]
        if general:
            os.environ["RTG_MEGA_GENERAL"] = "1"
        for _ in range(k):
            ds.radiance_device(buf.data_ptr(), n, out.data_ptr(), ids_ptr=ids.data_ptr() if ids is not None else 0,
                               stream=st, camera_eye=True)
        os.environ.pop("RTG_MEGA_GENERAL", None)

    hdr = torch.empty((h, w, 3), dtype=torch.float32, device=dev)

    def k_render():
        ds.render_device(hdr.data_ptr(), 0, stream=st, flags=rtgpu.RTG_RENDER_FUSED | rtgpu.RTG_RENDER_TIMING)
        return ds.timings()["k_render"]

    # the answers first: every order gives the fused render's image
    k_render()
    torch.cuda.synchronize()
    want = hdr.reshape(-1, 3).clone()
    for _, which, general in cases:
        run(which, general, 1)
        torch.cuda.synchronize()
        ids = sets[which][1]
        ref = want if ids is None else want[ids.long()]
        assert torch.equal(out[:, :3].view(torch.int32), ref.view(torch.int32)), which
    for _, which, general in cases:
        run(which, general, args.warmup)
    for _ in range(args.warmup):
        k_render()
    torch.cuda.synchronize()
    ms = {c[0]: [] for c in cases}
    kr = []
    for _ in range(args.reps):
        for label, which, general in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(which, general, args.launches)
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / args.launches)
        kr.append(float(np.median([k_render() for _ in range(args.launches)])))
    lines = [f"radiance: {name} {w}x{h}, {n} rays, {args.launches} launches x {args.reps} interleaved repetitions "
             f"(every order checked against the fused render bit for bit)",
             f"{'case':40s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'/ k_render':>10s}"]
    lines.append(f"{'k_render (fused render, same session)':40s} {np.median(kr):12.4f} {min(kr):8.4f} {max(kr):8.4f} {1.0:10.3f}")
    for label, _, _ in cases:
        v = ms[label]
        lines.append(f"{label:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {np.median(v) / np.median(kr):10.3f}")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append(f"spread over the repetitions: k_render {spread(kr):.1f} %, " +
                 ", ".join(f"{label.split()[0]} {spread(ms[label]):.1f} %" for label, _, _ in cases))
    return lines


def radiance_main(args):
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    lines = []
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    lines += radiance_section(args, f"synthetic_heightfield K={args.K}", xml)
    os.chdir(os.path.join(ROOT, "tests", "golden", "scenes"))
    lines += radiance_section(args, "pt_cornell", "pt_cornell.xml")
    return lines


def surface_section(args, name, xml, min_rays):
    """Timings of one scene: lines of text."""
    import torch

    import rtgpu

    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    cam = hs.camera(0)
    w, h = cam["width"], cam["height"]
    n0 = w * h
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rays0 = torch.empty((n0, 8), dtype=torch.float32, device=dev)
    ds.camera_rays_device(rays0.data_ptr(), stream=st)
    torch.cuda.synchronize()
    rep = max(1, -(-min_rays // n0))
    n = n0 * rep
    pixel = rays0.repeat(rep, 1).contiguous()
    sets = {"pixel": pixel}
    if w % 8 == 0 and h % 8 == 0:
        # k_primary's wave shape (rtg_frame.hpp tile_pixel): 64 consecutive rays = one 8x8 pixel tile
        yy, xx = np.divmod(np.arange(n0), w)
        key = (yy // 8) * (w // 8) * 64 + (xx // 8) * 64 + (yy % 8) * 8 + (xx % 8)
        order = np.empty(n0, np.int64)
        order[key] = np.arange(n0)
        sets["tiled"] = rays0[torch.from_numpy(order).to(dev)].repeat(rep, 1).contiguous()
    surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
    hits = torch.empty((n, 4), dtype=torch.int32, device=dev)
    nrm = torch.empty((n, 4), dtype=torch.float32, device=dev)
    C = rtgpu.RTG_QUERY_COHERENT
    cases = []
    for which in sets:
        for hint in (True, False):
            tag = f"{which}{', hint' if hint else ''}"
            cases.append((f"s  surface, {tag}", which, hint, True))
            cases.append((f"t  trace + normals, {tag}", which, hint, False))

    def run(which, hint, is_surface, k):
        buf = sets[which]
        for _ in range(k):
            if is_surface:
                ds.surface_device(buf.data_ptr(), n, surf.data_ptr(), stream=st, coherent=hint)
            else:
                ds.trace_device(buf.data_ptr(), n, hits.data_ptr(), nrm.data_ptr(), stream=st, flags=C if hint else 0)

    # the answers first: the hit and the geometric normal of (s) are those of (t), bit for bit
    for which in sets:
        for hint in (True, False):
            run(which, hint, True, 1)
            run(which, hint, False, 1)
            torch.cuda.synchronize()
            assert torch.equal(surf[:, 0:3].view(torch.int32), hits[:, 0:3]), which
            assert torch.equal(surf[:, 8:11].view(torch.int32), nrm[:, 0:3].view(torch.int32)), which
    n_hit = int((hits[:, 1] >= 0).sum())
    for _, which, hint, is_surface in cases:
        run(which, hint, is_surface, args.warmup)
    torch.cuda.synchronize()
    ms = {c[0]: [] for c in cases}
    for _ in range(args.reps):
        for label, which, hint, is_surface in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(which, hint, is_surface, args.launches)
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / args.launches)
    lines = [f"surface: {name} {w}x{h} x {rep}, {n} rays ({n_hit} hits), {args.launches} launches x {args.reps} interleaved "
             f"repetitions, device {torch.cuda.get_device_name(0)} (t / object / face / ng of every case checked against trace_device)",
             f"{'case':40s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Grays/s':>9s} {'s / t':>7s}"]
    for label, which, hint, is_surface in cases:
        v = ms[label]
        ratio = ""
        if is_surface:
            other = next(c[0] for c in cases if c[1] == which and c[2] == hint and not c[3])
            ratio = f"{np.median(v) / np.median(ms[other]):7.3f}"
        lines.append(f"{label:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e6:9.3f} {ratio:>7s}")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append("spread over the repetitions: " + ", ".join(f"{spread(ms[c[0]]):.1f} %" for c in cases))
    return lines


def surface_main(args):
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    lines = []
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    lines += surface_section(args, f"synthetic_heightfield K={args.K}", xml, 0)
    os.chdir(os.path.join(ROOT, "tests", "golden", "scenes"))
    lines += surface_section(args, "transforms_textures", "transforms_textures.xml", 1 << 20)
    return lines


def update_section(args, name, xml_a, xml_b):
    """Scene set-up times of one scene and its variant (same geometry): lines of text."""
    import time

    import torch

    import rtgpu

    hs_a, hs_b = rtgpu.HostScene(xml_a), rtgpu.HostScene(xml_b)
    cam = hs_a.camera(0)
    w, h = cam["width"], cam["height"]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn, n):
        """Wall-clock ms of n calls, each between two device synchronisations."""
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    live = rtgpu.DeviceScene(hs_a, 0)
    flip = [hs_b, hs_a]

    def create():
        rtgpu.DeviceScene(hs_b, 0).close()

    def update():
        flip.reverse()
        live.update(flip[0], stream=st)

    def clone():
        live.clone().close()

    def clone_update():
        c = live.clone()
        c.update(hs_b, stream=st)
        torch.cuda.synchronize()
        c.close()

    for fn in (create, update, clone, clone_update):
        timed(fn, 2)
    ms = {"create (rtg_scene_create + destroy)": timed(create, args.setups),
          "update (rtg_scene_update, in place)": timed(update, 4 * args.setups),
          "clone (rtg_scene_clone + destroy)": timed(clone, args.setups),
          "clone + update + destroy": timed(clone_update, args.setups)}
    # renders: the scene updated to B against a scene freshly created from B, interleaved
    if flip[0] is not hs_b:
        update()
    fresh = rtgpu.DeviceScene(hs_b, 0)
    bufs = [torch.empty((h, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]
    scenes_ = (("render, updated scene", live, bufs[0]), ("render, fresh scene", fresh, bufs[1]))
    for _, ds, buf in scenes_:
        for _ in range(args.warmup):
            ds.render_device(buf.data_ptr(), 0, stream=st)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0].view(torch.int32), bufs[1].view(torch.int32)), "updated and fresh renders differ"
    rs = {label: [] for label, _, _ in scenes_}
    for _ in range(args.reps):
        for label, ds, buf in scenes_:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                ds.render_device(buf.data_ptr(), 0, stream=st)
            e1.record()
            e1.synchronize()
            rs[label].append(e0.elapsed_time(e1) / args.launches)
    c = hs_a.counts()
    lines = [f"update: {name} {w}x{h}, {c['objects']} objects, {c['faces']} faces, {c['lights']} lights, device "
             f"{torch.cuda.get_device_name(0)}; wall clock between device synchronisations, median of {args.setups} calls "
             f"(update: {4 * args.setups}); renders: {args.launches} launches x {args.reps} interleaved repetitions, "
             f"the two images equal bit for bit",
             f"{'case':40s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'/ create':>9s}"]
    base = np.median(ms["create (rtg_scene_create + destroy)"])
    for label, v in ms.items():
        lines.append(f"{label:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {np.median(v) / base:9.4f}")
    for label, v in rs.items():
        lines.append(f"{label:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f}")
    return lines


def update_main(args):
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    os.chdir(tmp)

    def variant(xml, subs):
        text = open(xml).read()
        for pat, rep in subs:
            text, k = re.subn(pat, rep, text, count=1)
            assert k == 1, pat
        out = xml[:-4] + "_b.xml"
        with open(out, "w") as f:
            f.write(text)
        return out

    light = r"(<PointLight id=\"1\">\s*<Position>)[^<]*"
    lines = []
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    lines += update_section(args, f"synthetic_heightfield K={args.K}", xml,
                            variant(xml, [(light, r"\g<1>1.2 -0.7 1.3"), (r"(<Intensity>)[^<]*", r"\g<1>380 420 400")]))
    xml = scenes.config_c4(tmp, width=args.width, height=args.height, spp=1)
    lines += update_section(args, "c4_forest (100 instances of a 10k-triangle tree), 1 spp", xml,
                            variant(xml, [(light, r"\g<1>4 28 14"), (r"(<Rotation id=\"2\">)[^<]*", r"\g<1>55 0 1 0"),
                                          (r"(<Translation id=\"9\">)[^<]*", r"\g<1>-9.5 0 3.5")]))
    return lines


def multi_main(args):
    """Multi-hit queries (rtg_trace_rays_multi_device) on the headline height field: lines of text."""
    import torch

    import rtgpu
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    w, h = args.width, args.height
    n = w * h
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    ds.camera_rays_device(rays.data_ptr(), stream=st)
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(1234)
    sets = {"pixel order": rays, "permuted": rays[torch.randperm(n, generator=g).to(dev)].contiguous()}
    ks = (1, 2, 4, 8)
    hits = torch.empty((n, max(ks), 4), dtype=torch.int32, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    closest = torch.empty((n, 4), dtype=torch.int32, device=dev)
    cases = [(f"trace_device (closest, no hint), {which}", which, 0) for which in sets]
    cases += [(f"multi k = {k}, {which}", which, k) for which in sets for k in ks]

    def run(which, k, reps):
        buf = sets[which]
        for _ in range(reps):
            if k:
                ds.trace_multi_device(buf.data_ptr(), n, k, hits.data_ptr(), cnt.data_ptr(), stream=st)
            else:
                ds.trace_device(buf.data_ptr(), n, closest.data_ptr(), stream=st)

    # the answers first: k = 1 is the closest hit bit for bit; slot 0 of a longer list is too, except
    # on near ties (a larger minT culls fewer boxes, and a face one ulp nearer behind a box the
    # closest-hit walk culls is found): there the distances agree within 1e-4 relative
    held, ties = {}, {}
    for which in sets:
        run(which, 0, 1)
        for k in ks:
            run(which, k, 1)
            torch.cuda.synchronize()
            first = hits.view(-1, 4)[: n * k].view(n, k, 4)[:, 0, :]
            differ = (first[:, :3] != closest[:, :3]).any(1)
            ta, tb = first[differ, 0].view(torch.float32), closest[differ, 0].view(torch.float32)
            assert (k > 1 or not differ.any()) and bool(((ta - tb).abs() <= 1e-4 * tb.abs().clamp(min=1.0)).all()), (which, k)
            held[which, k], ties[which, k] = float(cnt.float().mean()), int(differ.sum())
    for _, which, k in cases:
        run(which, k, args.warmup)
    torch.cuda.synchronize()
    ms = {c[0]: [] for c in cases}
    for _ in range(args.reps):
        for label, which, k in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(which, k, args.launches)
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / args.launches)
    lines = [f"multi: synthetic_heightfield K={args.K} {w}x{h}, {n} rays, {args.launches} launches x {args.reps} interleaved "
             f"repetitions, device {torch.cuda.get_device_name(0)} (slot 0 of every case checked against trace_device: "
             f"equal but for {max(ties.values())} near-tie rays at most)",
             f"{'case':44s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Grays/s':>9s} {'hits held':>10s}"]
    for label, which, k in cases:
        v = ms[label]
        lines.append(f"{label:44s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e6:9.3f} "
                     f"{held[which, k] if k else float('nan'):10.3f}")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append("spread over the repetitions: " + ", ".join(f"{spread(ms[c[0]]):.1f} %" for c in cases))
    return lines


def closest_main(args):
    """Closest-point queries (rtg_closest_points_device) on the headline height field: lines of text."""
    import torch

    import rtgpu
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    rng = np.random.default_rng(1234)
    rays = ds.camera_rays()
    hits, nrm = ds.trace(rays, normals=True)
    ok = hits["object"] >= 0
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)[ok]
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)[ok]
    hit_xyz = o + d * hits["t"][ok][:, None]
    lo, hi = hit_xyz.min(0).astype(np.float64), hit_xyz.max(0).astype(np.float64)
    hi[2] += 0.05 * (hi[0] - lo[0])
    gx, gy, gz = 512, 512, 8
    cell = (hi - lo) / (gx, gy, gz)
    zz, yy, xx = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    grid = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    grid = (lo + (grid + rng.random(grid.shape)) * cell).astype(np.float32)
    lifted = (hit_xyz + nrm[ok, :3] * (10.0 ** rng.uniform(-3.0, 0.0, (len(hit_xyz), 1)))).astype(np.float32)
    radius = float(4.0 * np.sqrt((hi[0] - lo[0]) * (hi[1] - lo[1]) / (args.K / 2)))
    sets = {"(g) grid order": grid, "(g-perm) shuffled": grid[rng.permutation(len(grid))], "(h) lifted hit points": lifted}
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    cases, bufs, held = [], {}, {}
    for which, xyz in sets.items():
        for label, md in (("max_dist = inf", np.inf), ("max_dist = %.4g" % radius, radius)):
            pts = rtgpu.make_points(xyz, md)
            key = f"{which}, {label}"
            d_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)
            d_out = torch.empty((len(pts), 8), dtype=torch.int32, device=dev)
            ds.closest_device(d_pts.data_ptr(), len(pts), d_out.data_ptr(), stream=st)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            pick = rng.choice(len(pts), 65536, replace=False)
            want = hs.closest(pts[pick])
            assert got[pick].tobytes() == want.tobytes(), (key, "device != host walk")
            held[key] = float((got[:, 1] >= 0).mean())
            bufs[key] = (d_pts, d_out, len(pts))
            cases.append(key)

    def run(key, reps):
        d_pts, d_out, n = bufs[key]
        for _ in range(reps):
            ds.closest_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=st)

    for key in cases:
        run(key, args.warmup)
    torch.cuda.synchronize()
    ms = {key: [] for key in cases}
    for _ in range(args.reps):
        for key in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(key, args.launches)
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / args.launches)
    lines = [f"closest: synthetic_heightfield K={args.K}, {args.launches} launches x {args.reps} interleaved repetitions, "
             f"device {torch.cuda.get_device_name(0)}, library {os.path.basename(rtgpu.LIB_PATH)} (65 536 points of every "
             f"case equal the host walk bit for bit)",
             f"{'case':48s} {'points':>9s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Gpoints/s':>10s} {'answered':>9s}"]
    for key in cases:
        v, n = ms[key], bufs[key][2]
        lines.append(f"{key:48s} {n:9d} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e6:10.3f} "
                     f"{held[key]:9.3f}")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append("spread over the repetitions: " + ", ".join(f"{spread(ms[key]):.1f} %" for key in cases))
    return lines


def _timed(cases, run, args):
    """ms per launch of every case: warm-up, then --reps interleaved repetitions of --launches launches."""
    import torch
    for key in cases:
        run(key, args.warmup)
    torch.cuda.synchronize()
    ms = {key: [] for key in cases}
    for _ in range(args.reps):
        for key in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(key, args.launches)
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / args.launches)
    return ms


def crossings_main(args):
    """Crossing counts (rtg_count_crossings_device) on the headline height field: lines of text."""
    import torch

    import rtgpu
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    n = args.width * args.height
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    ds.camera_rays_device(rays.data_ptr(), stream=st)
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(1234)
    sets = {"pixel order": rays, "permuted": rays[torch.randperm(n, generator=g).to(dev)].contiguous()}
    hits = torch.empty((n, 8, 4), dtype=torch.int32, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    cases = [(kind, which) for which in sets for kind in ("crossings", "multi k = 8 + counts")]

    def run(key, reps):
        kind, which = key
        buf = sets[which]
        for _ in range(reps):
            if kind == "crossings":
                ds.crossings_device(buf.data_ptr(), n, out.data_ptr(), stream=st)
            else:
                ds.trace_multi_device(buf.data_ptr(), n, 8, hits.data_ptr(), cnt.data_ptr(), stream=st)

    # the answers first: the multi-hit counts (equal wherever that walk holds fewer than 8 hits) and a sample of the host walk
    most = {}
    for which, buf in sets.items():
        run(("crossings", which), 1)
        run(("multi k = 8 + counts", which), 1)
        torch.cuda.synchronize()
        full = cnt >= 8
        assert torch.equal(out[:, 0][~full], cnt[~full]) and bool((out[:, 0][full] >= 8).all()), which
        pick = np.random.default_rng(1234).choice(n, 65536, replace=False)
        want = hs.crossings(buf.cpu().numpy().view(rtgpu.RAY_DTYPE).reshape(-1)[pick])
        assert out.cpu().numpy()[pick].tobytes() == want.tobytes(), (which, "device != host walk")
        most[which] = (int(out[:, 0].max()), float(out[:, 0].float().mean()), int(full.sum()))
    ms = _timed(cases, run, args)
    lines = [f"crossings: synthetic_heightfield K={args.K} {args.width}x{args.height}, {n} unbounded camera rays, {args.launches} "
             f"launches x {args.reps} interleaved repetitions, device {torch.cuda.get_device_name(0)} (counts equal the k = 8 "
             f"multi-hit counts on every ray that holds fewer than 8 hits, all but {most['pixel order'][2]}; 65 536 rays of each "
             f"order equal the host walk bit for bit; hits per ray: mean {most['pixel order'][1]:.3f}, most {most['pixel order'][0]})",
             f"{'case':44s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Grays/s':>9s}"]
    for key in cases:
        v = ms[key]
        lines.append(f"{key[0] + ', ' + key[1]:44s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e6:9.3f}")
    for which in sets:
        c, m = np.median(ms["crossings", which]), np.median(ms["multi k = 8 + counts", which])
        lines.append(f"{which}: crossings rate / multi-hit k = 8 rate = {m / c:.3f} (condition: >= 1)")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append("spread over the repetitions: " + ", ".join(f"{spread(ms[key]):.1f} %" for key in cases))
    return lines


def sdf_main(args):
    """Signed distances (rtg_signed_distance_points_device) on the headline height field against
    closest_device then crossings_device on the same points: lines of text."""
    import torch

    import rtgpu
    import scenes

    tmp = tempfile.mkdtemp(prefix="query_bench_")
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    rng = np.random.default_rng(1234)
    rays = ds.camera_rays()
    hits = ds.trace(rays)
    ok = hits["object"] >= 0
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)[ok]
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1)[ok]
    hit_xyz = o + d * hits["t"][ok][:, None]
    # the closest section's grid: jittered 512 x 512 x 8 through the box of the camera's hit points
    lo, hi = hit_xyz.min(0).astype(np.float64), hit_xyz.max(0).astype(np.float64)
    hi[2] += 0.05 * (hi[0] - lo[0])
    gx, gy, gz = 512, 512, 8
    cell = (hi - lo) / (gx, gy, gz)
    zz, yy, xx = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    grid = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    grid = (lo + (grid + rng.random(grid.shape)) * cell).astype(np.float32)
    radius = float(4.0 * np.sqrt((hi[0] - lo[0]) * (hi[1] - lo[1]) / (args.K / 2)))
    up = (0.0, 0.0, 1.0)                         # the field's heights are along z
    n = len(grid)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    up_rays = rtgpu.make_rays(grid, np.tile(np.array(up, np.float32), (n, 1)))
    d_rays = torch.from_numpy(up_rays.view(np.float32).reshape(-1, 8).copy()).to(dev)
    d_cross = torch.empty((n, 2), dtype=torch.int32, device=dev)
    d_out = torch.empty((n, 8), dtype=torch.int32, device=dev)
    bufs, below = {}, {}
    for label, md in (("max_dist = inf", np.inf), ("max_dist = %.4g" % radius, radius)):
        pts = rtgpu.make_points(grid, md)
        d_pts = torch.from_numpy(pts.view(np.float32).reshape(-1, 4).copy()).to(dev)
        ds.signed_distance_device(d_pts.data_ptr(), n, d_out.data_ptr(), direction=up, stream=st)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        pick = rng.choice(n, 65536, replace=False)
        assert got[pick].tobytes() == hs.signed_distance(pts[pick], up).tobytes(), (label, "device != host walk")
        # the two launches give the same record: closest's with the count and the sign put in
        ds.closest_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=st)
        ds.crossings_device(d_rays.data_ptr(), n, d_cross.data_ptr(), stream=st)
        torch.cuda.synchronize()
        two = d_out.cpu().numpy().view(rtgpu.NEAREST_DTYPE).reshape(-1).copy()
        count = d_cross.cpu().numpy()[:, 0]
        two["pad0"] = count
        flip = (two["object"] >= 0) & ((count & 1) == 1)
        two["dist"][flip] = -two["dist"][flip]
        assert two.tobytes() == got.tobytes(), (label, "fused != closest + crossings")
        below[label] = float((count & 1).mean())
        bufs[label] = d_pts
    cases = [(kind, label) for label in bufs for kind in ("signed_distance (fused)", "closest", "crossings")]

    def run(key, reps):
        kind, label = key
        d_pts = bufs[label]
        for _ in range(reps):
            if kind == "closest":
                ds.closest_device(d_pts.data_ptr(), n, d_out.data_ptr(), stream=st)
            elif kind == "crossings":
                ds.crossings_device(d_rays.data_ptr(), n, d_cross.data_ptr(), stream=st)
            else:
                ds.signed_distance_device(d_pts.data_ptr(), n, d_out.data_ptr(), direction=up, stream=st)

    ms = _timed(cases, run, args)
    lines = [f"sdf: synthetic_heightfield K={args.K}, {n} points of the closest section's grid, dir = (0, 0, 1), {args.launches} "
             f"launches x {args.reps} interleaved repetitions, device {torch.cuda.get_device_name(0)} (65 536 points of each "
             f"case equal the host walk bit for bit; the fused record equals closest + crossings on every point; "
             f"{below['max_dist = inf']:.3f} of the points are below the terrain)",
             f"{'case':48s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Gpoints/s':>10s}"]
    for key in cases:
        v = ms[key]
        lines.append(f"{key[0] + ', ' + key[1]:48s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e6:10.3f}")
    for label in bufs:
        f = np.median(ms["signed_distance (fused)", label])
        two = np.median(ms["closest", label]) + np.median(ms["crossings", label])
        lines.append(f"{label}: fused {f:.4f} ms, closest + crossings {two:.4f} ms, ratio {f / two:.3f} (condition: <= 1)")
    spread = lambda v: (max(v) - min(v)) / np.median(v) * 100
    lines.append("spread over the repetitions: " + ", ".join(f"{spread(ms[key]):.1f} %" for key in cases))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", type=int, default=9, help="update section: calls per set-up time")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=100352)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="query,radiance")
    args = ap.parse_args()
    out = os.path.abspath(args.out) if args.out else None
    sections = args.sections.split(",")
    text = []
    if "query" in sections:
        text += query_main(args)
    if "radiance" in sections:
        text += radiance_main(args)
    if "surface" in sections:
        text += surface_main(args)
    if "update" in sections:
        text += update_main(args)
    if "multi" in sections:
        text += multi_main(args)
    if "closest" in sections:
        text += closest_main(args)
    if "crossings" in sections:
        text += crossings_main(args)
    if "sdf" in sections:
        text += sdf_main(args)
    text = "\n".join(text)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


def query_main(args):
    import torch

    import rtgpu
    import scenes

    os.environ["RTG_FRAME_KERNEL"] = "0"      # the timed renders: k_primary as its own stage
    tmp = tempfile.mkdtemp(prefix="query_bench_")
    xml = scenes.synthetic_heightfield(tmp, K=args.K, width=args.width, height=args.height)
    os.chdir(tmp)
    hs = rtgpu.HostScene(xml)
    ds = rtgpu.DeviceScene(hs, 0)
    light = np.array(re.search(r"<Position>([^<]*)</Position>\s*<Intensity>", open(xml).read()).group(1).split(),
                     np.float32)
    eps = float(re.search(r"<ShadowRayEpsilon>([^<]*)<", open(xml).read()).group(1))
    w, h = args.width, args.height
    n = w * h
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    hits = torch.empty((n, 4), dtype=torch.int32, device=dev)
    nrm = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ds.camera_rays_device(rays.data_ptr(), stream=st)
    ds.trace_device(rays.data_ptr(), n, hits.data_ptr(), nrm.data_ptr(), stream=st, flags=rtgpu.RTG_QUERY_COHERENT)
    torch.cuda.synchronize()
    g = torch.Generator(device="cpu").manual_seed(1234)
    permuted = rays[torch.randperm(n, generator=g).to(dev)].contiguous()
    # k_primary's wave shape (rtg_frame.hpp tile_pixel): 64 consecutive rays = one 8x8 pixel tile
    assert w % 16 == 0 and h % 8 == 0
    yy, xx = np.divmod(np.arange(n), w)
    key = (yy // 8) * (w // 8) * 64 + (xx // 8) * 64 + (yy % 8) * 8 + (xx % 8)
    order = np.empty(n, np.int64)
    order[key] = np.arange(n)
    tiled = rays[torch.from_numpy(order).to(dev)].contiguous()
    # the shadow rays' equivalent (IsInShadow, raytracer.cpp:555-584): from p + n * eps towards the
    # light, up to the light's distance; misses get a zero-length query
    t = hits[:, 0].view(torch.float32)
    hit = hits[:, 1] >= 0
    p = rays[:, 0:3] + rays[:, 4:7] * torch.where(hit, t, torch.zeros_like(t))[:, None]
    to_l = torch.from_numpy(light).to(dev)[None, :] - p
    dist = to_l.norm(dim=1)
    shadow = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    shadow[:, 0:3] = p + nrm[:, 0:3] * eps
    shadow[:, 3] = torch.where(hit, dist, torch.zeros_like(dist))
    shadow[:, 4:7] = to_l / dist[:, None]
    n_hit = int(hit.sum())

    C, A = rtgpu.RTG_QUERY_COHERENT, rtgpu.RTG_QUERY_ANY_HIT
    cases = [("a  closest, coherent hint", rays, C), ("b  closest, no hint", rays, 0),
             ("c  closest, permuted, no hint", permuted, 0), ("c+ closest, permuted, hint", permuted, C),
             ("d  occlusion, shadow rays", shadow, A), ("d+ occlusion, shadow rays, hint", shadow, A | C),
             ("a-tiled closest, 8x8 tiles, hint", tiled, C)]

    def run(buf, flags, k):
        for _ in range(k):
            ds.trace_device(buf.data_ptr(), n, hits.data_ptr(), stream=st, flags=flags)

    hdr = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    ldr = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)

    def render_stages(flags):
        ds.render_device(hdr.data_ptr(), ldr.data_ptr(), stream=st, flags=flags | rtgpu.RTG_RENDER_TIMING)
        return ds.timings()

    for _, buf, flags in cases:
        run(buf, flags, args.warmup)
    for _ in range(args.warmup):
        render_stages(0)
        render_stages(rtgpu.RTG_RENDER_EXACT_SHADOW)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in cases}
    stages = {}
    for _ in range(args.reps):
        for name, buf, flags in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(buf, flags, args.launches)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.launches)
        # (a render's stages are single launches: the median of as many renders as launches)
        for tag, flags in (("", 0), (" [exact shadow]", rtgpu.RTG_RENDER_EXACT_SHADOW)):
            per = {}
            for _ in range(args.launches):
                for k, v in render_stages(flags).items():
                    per.setdefault(k + tag, []).append(v)
            for k, v in per.items():
                stages.setdefault(k, []).append(float(np.median(v)))

    lines = [f"query_bench: synthetic_heightfield K={args.K} {w}x{h}, {n} rays ({n_hit} hits), "
             f"{args.launches} launches x {args.reps} interleaved repetitions, device {torch.cuda.get_device_name(0)}",
             f"{'case':40s} {'ms (median)':>12s} {'min':>8s} {'max':>8s} {'Mrays/s':>10s}"]
    for name, _, _ in cases:
        v = ms[name]
        lines.append(f"{name:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e3:10.0f}")
    lines.append("render stages of the same session (RTG_FRAME_KERNEL=0; median of single launches per repetition)")
    for k, v in stages.items():
        lines.append(f"{k:40s} {np.median(v):12.4f} {min(v):8.4f} {max(v):8.4f} {n / np.median(v) / 1e3:10.0f}")
    a, kp = ms[cases[0][0]], stages.get("k_primary", [float("nan")])
    lines.append(f"(a) / k_primary = {np.median(a) / np.median(kp):.3f}; spread of k_primary over the repetitions "
                 f"{(max(kp) - min(kp)) / np.median(kp) * 100:.1f} %, of (a) {(max(a) - min(a)) / np.median(a) * 100:.1f} %")
    os.environ.pop("RTG_FRAME_KERNEL", None)
    return lines


if __name__ == "__main__":
    main()
