#!/usr/bin/env python3
"""What depth cues cost next to the plain render, next to what a caller pays for them without the feature, and next to outlines,
the other two-pass render.  Not a test.

A 1920 x 1080 view; fog between the 0.15 and 0.85 quantiles of the view's own hit distances, at strength 0.875 and on the
background too, and a tint along (0.5, -0.25, 0.75, 1.0, -0.5, ...) between the same quantiles of its coordinate.  The legs are
timed against each other, alternately in one process, each on a scene object of its own (same description, same camera):

  plain          (a) nt_render_device into fp32 x 3, the setting off
  cued           (b) the same with fog and tint on: the packet route, one walk and cue_shade
  composed       (c) what a caller has without the feature: (a) into little-endian floats (a reversed format), scene.primary_hits as
                     device tensors, and a torch expression of the rule on them.  The directions d of the view are formed once,
                     outside the timing, so the leg is a lower bound of the caller's cost
  outlined       (d) the plain format with set_outlines(0.1, 0.02) instead: the yardstick for a walk with a second pass
  cued_var       (e) (b) under NTRACER_FORCE_VAR=1: the general route -- base frame, primary-hit pass, cue_apply -- on the same scene

on the golden 120-cell, and (b) alone on feature5_n5, which takes the general route by itself.

The chip is settled the way tools/ao_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of
--leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/cue_time.py [--rounds 7] [--reps 10] [--frame 0]      one JSON line a scene, appended to profiles/cue_time.jsonl"""
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
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import tracern  # noqa: E402

W, H = args.width, args.height
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
FOG_COLOR, STRENGTH = (0.75, 0.8125, 0.875), 0.875
TINT_COLORS = ((1.0, 0.5, 0.25), (0.25, 0.5, 1.0))
SETTLE_MS = 200.0
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
fmt_le = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32], 0, True)     # little-endian floats, (b, g, r)
renderer = ntracer_amd.BlockingRenderer()


class limit:
    """the calls of one leg under an alarm of their own, up to the synchronisation that ends them"""
    def __enter__(self):
        signal.alarm(args.leg_timeout)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        signal.alarm(0)


def directions(sc, n, origin, axes):
    """the unit directions [H][W][n] of the pinhole view, in torch"""
    a = torch.tensor(np.asarray(axes, np.float32), device=dev)
    fovI = 2.0 * float(np.tan(sc.fov / 2.0)) / W
    xs = (torch.arange(W, device=dev, dtype=torch.float32) - W / 2.0) * fovI
    ys = (torch.arange(H, device=dev, dtype=torch.float32) - H / 2.0) * fovI
    v = a[2][None, None, :] + a[0][None, None, :] * xs[None, :, None] - a[1][None, None, :] * ys[:, None, None]
    return v / v.norm(dim=2, keepdim=True)


def measure(label, make, n, origin, axes, want):
    axis = np.array([(0.5, -0.25, 0.75, 1.0, -0.5)[k % 5] for k in range(n)], np.float32)
    probe = make()
    probe._set_camera_arrays(origin, axes)
    with limit():
        hp = probe.primary_hits(W, H, device=dev)
        d = directions(probe, n, origin, axes)
        o_t, axis_t = torch.tensor(np.asarray(origin, np.float32), device=dev), torch.tensor(axis, device=dev)
        hit = hp.item >= 0
        s = ((d * hp.dist[..., None] + o_t) * axis_t).sum(dim=2)
        q = torch.tensor([0.15, 0.85], device=dev)
        near, far = (float(np.float32(v)) for v in torch.quantile(hp.dist[hit][::7], q).tolist())
        lo, hi = (float(np.float32(v)) for v in torch.quantile(s[hit][::7], q).tolist())
    inv_fog, inv_tint = 1.0 / (far - near), 1.0 / (hi - lo)
    fog_t = torch.tensor(FOG_COLOR[::-1], device=dev)
    c_lo, c_hi = torch.tensor(TINT_COLORS[0][::-1], device=dev), torch.tensor(TINT_COLORS[1][::-1], device=dev)
    scenes, last = {}, {}
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name.startswith("cued"):
            sc.set_depth_cue(near, far, FOG_COLOR, STRENGTH, True, tint_axis=[float(v) for v in axis], tint_range=(lo, hi), tint_colors=TINT_COLORS)
        if name == "outlined":
            sc.set_outlines(0.1, 0.02)
        scenes[name] = sc
    frames = {name: torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev) for name in want}

    def leg(name):
        sc = scenes[name]
        if name == "composed":
            def run():
                renderer.render(frames[name], fmt_le, sc)
                h = sc.primary_hits(W, H, device=dev)
                P = frames[name].view(torch.float32).view(H, W, 3)
                t, opaque = h.dist, h.item >= 0
                f = ((t - near) * inv_fog).clamp(0.0, 1.0)
                g = ((((d * t[..., None] + o_t) * axis_t).sum(dim=2) - lo) * inv_tint).clamp(0.0, 1.0)
                Q = torch.where(opaque[..., None], P * (c_lo * (1.0 - g)[..., None] + c_hi * g[..., None]), P)
                w = torch.where(opaque, f, (h.n_transparent == 0).to(torch.float32)) * STRENGTH
                fogged = Q * (1.0 - w)[..., None] + fog_t * w[..., None]
                last[name] = torch.where((opaque | (h.n_transparent == 0))[..., None], fogged, Q)
            return run
        if name == "cued_var":
            def run():
                os.environ["NTRACER_FORCE_VAR"] = "1"       # (the switches are read at every call)
                try:
                    renderer.render(frames[name], fmt, sc)
                finally:
                    del os.environ["NTRACER_FORCE_VAR"]
            return run
        return lambda: renderer.render(frames[name], fmt, sc)
    legs = {name: leg(name) for name in want}
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "fog_near": near, "fog_far": far, "tint_lo": lo, "tint_hi": hi,
           "fog_strength": STRENGTH, "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    fg = scenes["cued"].depth_cue_factors(W, H, device=dev)
    torch.cuda.synchronize()
    out["share_of_pixels_hit"] = round(float((fg[..., 1] >= 0).float().mean()), 6)
    out["share_of_hits_on_the_fog_ramp"] = round(float(((fg[..., 0] > 0) & (fg[..., 0] < 1)).sum()) / max(1, int((fg[..., 1] >= 0).sum())), 6)
    if "plain" in frames:
        out["pixels_the_setting_changes"] = int((frames["plain"].view(H * W, 12) != frames["cued"].view(H * W, 12)).any(dim=1).sum())
    if "cued_var" in frames:
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(frames["cued"], frames["cued_var"]))
    if "composed" in last:
        mine = frames["cued"].view(H * W * 3, 4).flip(1).contiguous().view(torch.float32).view(H, W, 3).flip(2)
        out["composed_max_abs_difference"] = float((mine - last["composed"]).abs().max())
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
        for fn in legs.values():
            with limit():
                fn()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():              # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with limit():
                e0.record(st)
                for _ in range(args.reps):
                    fn()
                e1.record(st)
            ms[name].append(e0.elapsed_time(e1) / args.reps)
    for name, v in ms.items():
        out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    if "plain" in ms:
        out["cued_minus_plain_ms"] = round(out["cued"]["median_ms"] - out["plain"]["median_ms"], 4)
    if "outlined" in ms:
        out["cued_minus_outlined_ms"] = round(out["cued"]["median_ms"] - out["outlined"]["median_ms"], 4)
        out["cued_above_outlined_by_more_than_the_spread"] = bool(out["cued"]["min_ms"] > out["outlined"]["max_ms"])
    if "composed" in ms:
        out["cued_over_composed"] = round(out["cued"]["median_ms"] / out["composed"]["median_ms"], 3)
        out["cued_beats_composed_by_more_than_the_spread"] = bool(out["cued"]["max_ms"] < out["composed"]["min_ms"])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "cue_time.jsonl"), "a") as f:
        f.write(line + "\n")


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


def composite(g):
    n = int(g["dimension"])

    def make():
        sc = tracern.CompositeScene.from_flat(n, g)
        if "shadows" in g:
            sc.set_params_flat({k: g[k] for k in PARAM_KEYS if k in g})
        return sc
    return make, n


g = golden("cell120_n4")
make, n = composite(g)
f = int(g["frames"][args.frame])
measure("cell120_n4", make, n, g["origins"][f], g["axes"][f], ("plain", "cued", "composed", "outlined", "cued_var"))
g5 = golden("feature5_n5")
make, n = composite(g5)
f5 = int(g5["frames"][args.frame])
measure("feature5_n5", make, n, g5["origins"][f5], g5["axes"][f5], ("cued",))
