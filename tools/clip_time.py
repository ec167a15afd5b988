#!/usr/bin/env python3
"""What clip planes cost next to the plain render, and next to what a caller pays for a cutaway without the feature
(DESIGN.md 4.14).  Not a test.

A 1920 x 1080 view of the golden 120-cell and of the 600-cell lit (the "lit" variant of tests/ray_color_cases.py: shadows, two
point lights, a global light, 30 % reflective materials).  The planes come from the view's own primary hits, as
tests/clip_cases.py takes them: a = -(forward + 0.3 right), offsets at quantiles of a . x over the hit points.  The legs are
timed against each other, alternately in one process, each on a scene object of its own (same description, same camera):

  plain          nt_render_device into fp32 x 3, the setting off
  keep_all       planes that keep the whole scene box: the packet walk with the window, nothing cut
  median         one plane at the 0.5 quantile: the near half of what is seen taken away
  slab           that plane and a second at the 0.2 quantile behind it: a finite t1 on every ray
  plain_var      `plain` under NTRACER_FORCE_VAR=1: the run-time-n kernels, whose resources the setting changed -- the figure to
                 hold against the parent commit's (--label parent --package-root <a built checkout of it>)
  median_var     `median` under NTRACER_FORCE_VAR=1: the general route
  hits           scene.primary_hits under the median plane, device tensors
  hits_plain     the same with the setting off
  rays_advanced  what a caller has without the feature: render_rays from origins advanced to the median plane, which loses the
                 shared origin and with it the packet walk, cannot limit the far side and clips no shadow or reflection ray.
                 The rays are formed once, outside the timing, so the leg is a lower bound of the caller's cost

A library without the setting (the parent commit's) runs the legs that need none: plain, plain_var, hits_plain, rays_advanced.

The chip is settled the way tools/cue_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of
--leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/clip_time.py [--rounds 7] [--reps 10] [--frame 0] [--label this]      one JSON line a scene, appended to
                                                                                       profiles/clip_time.jsonl"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--frame", type=int, default=0, help="camera of the golden sequence")
ap.add_argument("--leg-timeout", type=int, default=60, help="seconds a leg's warm-up, settling calls or one timed round may take")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--label", default="this", help="what the line says it measured: this commit's library, or the parent's")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clip_time.jsonl"))
ap.add_argument("--package-root", default=HERE, help="the tree whose ntracer_amd is measured: a built checkout of the parent commit for --label parent")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import tracern  # noqa: E402

W, H = args.width, args.height
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")
HAS_CLIP = hasattr(tracern.CompositeScene, "set_clip_planes")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
renderer = ntracer_amd.BlockingRenderer()


class limit:
    """the calls of one leg under an alarm of their own, up to the synchronisation that ends them"""
    def __enter__(self):
        signal.alarm(args.leg_timeout)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        signal.alarm(0)


def directions(sc, axes):
    """the unit directions [H][W][n] of the pinhole view, in torch"""
    a = torch.tensor(np.asarray(axes, np.float32), device=dev)
    fovI = 2.0 * float(np.tan(sc.fov / 2.0)) / W
    xs = (torch.arange(W, device=dev, dtype=torch.float32) - W / 2.0) * fovI
    ys = (torch.arange(H, device=dev, dtype=torch.float32) - H / 2.0) * fovI
    v = a[2][None, None, :] + a[0][None, None, :] * xs[None, :, None] - a[1][None, None, :] * ys[:, None, None]
    return v / v.norm(dim=2, keepdim=True)


def measure(label, make, n, origin, axes, lo, hi):
    probe = make()
    probe._set_camera_arrays(origin, axes)
    axes = np.asarray(axes, np.float32).reshape(n, n)
    a = (-(axes[2] + np.float32(0.3) * axes[0])).astype(np.float32)
    with limit():
        hp = probe.primary_hits(W, H, device=dev)
        d = directions(probe, axes)
        o_t, a_t = torch.tensor(np.asarray(origin, np.float32), device=dev), torch.tensor(a, device=dev)
        hit = hp.item >= 0
        s = ((d * hp.dist[..., None] + o_t) * a_t).sum(dim=2)
        q20, q50 = (float(np.float32(v)) for v in torch.quantile(s[hit][::7], torch.tensor([0.2, 0.5], device=dev)).tolist())
        # the caller's own cutaway: origins advanced to the median plane (rays that run away from it keep the eye)
        r = (d * a_t).sum(dim=2)
        t0 = torch.where(r < 0, ((q50 - float(np.dot(a, np.asarray(origin, np.float32)))) / r).clamp(min=0.0), torch.zeros_like(r))
        adv_o = (o_t + d * t0[..., None]).reshape(-1, n).contiguous()
        adv_d = d.reshape(-1, n).contiguous()
    keep_all = [(tuple(float(j == k) * s_ for j in range(n)), float(s_ * (hi[k] if s_ > 0 else lo[k]) + 2.0 * (hi[k] - lo[k])))
                for k in range(min(n, 4)) for s_ in (1.0, -1.0)]
    sets = {"keep_all": keep_all, "median": [(tuple(float(v) for v in a), q50)], "median_var": [(tuple(float(v) for v in a), q50)],
            "hits": [(tuple(float(v) for v in a), q50)], "slab": [(tuple(float(v) for v in a), q50), (tuple(float(-v) for v in a), -q20)]}
    want = ["plain", "plain_var", "hits_plain", "rays_advanced"] + (["keep_all", "median", "slab", "median_var", "hits"] if HAS_CLIP else [])
    scenes = {}
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name in sets:
            sc.set_clip_planes(sets[name])
        scenes[name] = sc
    frames = {name: torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev) for name in want}

    def leg(name):
        sc = scenes[name]
        if name.endswith("_var"):
            def run():
                os.environ["NTRACER_FORCE_VAR"] = "1"       # (the switches are read at every call)
                try:
                    renderer.render(frames[name], fmt, sc)
                finally:
                    del os.environ["NTRACER_FORCE_VAR"]
            return run
        if name.startswith("hits"):
            return lambda: sc.primary_hits(W, H, device=dev)
        if name == "rays_advanced":
            return lambda: sc.render_rays(frames[name], fmt, adv_o, adv_d)
        return lambda: renderer.render(frames[name], fmt, sc)
    legs = {name: leg(name) for name in want}
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"label": args.label, "scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "q20": q20, "q50": q50,
           "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev), "library_has_the_setting": HAS_CLIP}
    out["share_of_pixels_hit"] = round(float(hit.float().mean()), 6)
    if HAS_CLIP:
        px = lambda name: frames[name].view(H * W, 12)                      # noqa: E731
        out["keep_all_equals_plain"] = bool(torch.equal(frames["keep_all"], frames["plain"]))
        out["pixels_the_median_plane_changes"] = int((px("median") != px("plain")).any(dim=1).sum())
        out["pixels_the_slab_changes"] = int((px("slab") != px("plain")).any(dim=1).sum())
        out["pixels_where_the_routes_differ"] = int((px("median") != px("median_var")).any(dim=1).sum())
        out["pixels_where_advanced_rays_differ_from_the_median_plane"] = int((px("median") != px("rays_advanced")).any(dim=1).sum())
    t0_ = time.perf_counter()
    while (time.perf_counter() - t0_) * 1e3 < SETTLE_MS:
        for name, fn in legs.items():
            if not name.endswith("_var"):                                  # (the general route takes tens of milliseconds a call)
                with limit():
                    fn()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():              # the legs alternate within a round
            reps = max(1, args.reps // 5) if name.endswith("_var") else args.reps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with limit():
                e0.record(st)
                for _ in range(reps):
                    fn()
                e1.record(st)
            ms[name].append(e0.elapsed_time(e1) / reps)
    for name, v in ms.items():
        out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    if HAS_CLIP:
        out["keep_all_minus_plain_ms"] = round(out["keep_all"]["median_ms"] - out["plain"]["median_ms"], 4)
        out["median_over_rays_advanced"] = round(out["median"]["median_ms"] / out["rays_advanced"]["median_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


def composite(g, lit):
    n = int(g["dimension"])
    flat = {k: np.asarray(g[k]) for k in tracern._FLAT_KEYS}
    params = {k: g[k] for k in PARAM_KEYS if k in g}
    if lit:
        # the "lit" variant of tests/ray_color_cases.py
        m = np.array(flat["materials"], np.float32).copy()
        m[:, 7] = 0.3
        flat["materials"] = m
        lo, hi = np.asarray(g["aabb_start"], np.float32), np.asarray(g["aabb_end"], np.float32)
        ctr, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
        out_pos = ctr + ext * 3.0 * np.resize(np.array([1.0, 0.8, -0.9, 0.4], np.float32), n)
        in_pos = ctr + ext * 0.15 * np.resize(np.array([-0.5, 0.3, 0.2, -0.4], np.float32), n)
        gdir = np.resize(np.array([0.2, -0.9, 0.3, 0.1], np.float32), n)
        params.update(shadows=1, point_light_pos=np.array([out_pos, in_pos], np.float32),
                      point_light_color=np.array([[40.0 * np.linalg.norm(ext) ** (n - 1)] * 3, [0.5 * np.linalg.norm(ext) ** (n - 1)] * 3], np.float32),
                      global_light_dir=np.array([gdir / np.linalg.norm(gdir)], np.float32), global_light_color=np.array([[0.4, 0.4, 0.5]], np.float32),
                      ambient=np.array([0.02, 0.02, 0.03], np.float32))

    def make():
        sc = tracern.CompositeScene.from_flat(n, flat)
        if params:
            sc.set_params_flat(params)
        return sc
    return make, n


for name, lit in (("cell120_n4", False), ("cell600_n4", True)):
    g = golden(name)
    make, n = composite(g, lit)
    f = int(g["frames"][args.frame])
    measure(name + (" lit" if lit else ""), make, n, g["origins"][f], g["axes"][f], np.asarray(g["aabb_start"], np.float64), np.asarray(g["aabb_end"], np.float64))
