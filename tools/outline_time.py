#!/usr/bin/env python3
"""What outlines cost next to the plain render, and next to what a caller pays for them without the feature.
Not a test.

A 1920 x 1080 view, crease_angle 0.1, depth_gap 0.02, black lines at full strength; the legs are timed against each other,
alternately in one process, each on a scene object of its own (same description, same camera):

  plain          (a) nt_render_device into fp32 x 3, the setting off
  outlined       (b) the same with the setting on: the packet route, one walk and outline_shade
  outlined_var   (c) (b) under NTRACER_FORCE_VAR=1: the general route -- base frame, primary-hit pass with normal rows,
                     outline_mark, outline_apply -- on the same scene
  hits           (d) scene.primary_hits(normals=True) as device tensors, the setting off: what a caller needs on the device before a
                     stencil of their own can start

on the golden 120-cell, and (b) alone on feature5_n5, which takes the general route by itself.  The bar: (b) against (a) + (d), the
walk a caller makes twice today, both from this run.  The caller's own stencil, and the 8 n bytes a pixel it reads, come on top of
(a) + (d) and are not counted.

The chip is settled the way tools/ao_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of
--leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/outline_time.py [--rounds 7] [--reps 10] [--frame 0]      one JSON line a scene, appended to profiles/outline_time.jsonl"""
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
ANGLE, GAP = 0.1, 0.02
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")

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


def measure(label, make, n, origin, axes, want):
    scenes, last = {}, {}
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name.startswith("outlined"):
            sc.set_outlines(ANGLE, GAP)
        scenes[name] = sc
    frames = {name: torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev) for name in want if name != "hits"}

    def leg(name):
        sc = scenes[name]
        if name == "hits":
            return lambda: last.__setitem__(name, sc.primary_hits(W, H, normals=True, device=dev))
        if name == "outlined_var":
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
    out = {"scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "crease_angle": ANGLE, "depth_gap": GAP,
           "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    mask = scenes["outlined"].outline_mask(W, H, device=dev)
    torch.cuda.synchronize()
    out["pixels_marked"] = int((mask != 0).sum())
    out["share_of_pixels_marked"] = round(float((mask != 0).float().mean()), 6)
    if "plain" in frames:
        changed = (frames["plain"].view(H * W, 12) != frames["outlined"].view(H * W, 12)).any(dim=1)
        out["pixels_the_setting_changes"] = int(changed.sum())
    if "outlined_var" in frames:
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(frames["outlined"], frames["outlined_var"]))
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
    if "plain" in ms and "hits" in ms:
        by_hand = [a + b for a, b in zip(ms["plain"], ms["hits"])]
        out["plain_plus_hits"] = {"median_ms": round(float(np.median(by_hand)), 4), "min_ms": round(float(min(by_hand)), 4),
                                  "max_ms": round(float(max(by_hand)), 4)}
        out["outlined_over_plain_plus_hits"] = round(out["outlined"]["median_ms"] / out["plain_plus_hits"]["median_ms"], 3)
        out["outlined_beats_plain_plus_hits_by_more_than_the_spread"] = bool(out["outlined"]["max_ms"] < out["plain_plus_hits"]["min_ms"])
        out["outlined_minus_plain_ms"] = round(out["outlined"]["median_ms"] - out["plain"]["median_ms"], 4)
        if "outlined_var" in ms:
            out["outlined_var_over_plain_plus_hits"] = round(out["outlined_var"]["median_ms"] / out["plain_plus_hits"]["median_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "outline_time.jsonl"), "a") as f:
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
measure("cell120_n4", make, n, g["origins"][f], g["axes"][f], ("plain", "outlined", "outlined_var", "hits"))
g5 = golden("feature5_n5")
make, n = composite(g5)
f5 = int(g5["frames"][args.frame])
measure("feature5_n5", make, n, g5["origins"][f5], g5["axes"][f5], ("outlined",))
