#!/usr/bin/env python3
"""What an X-ray view costs next to the plain render, and next to what a caller does for a look inside without the feature
(DESIGN.md 4.17).  Not a test.

A 1920 x 1080 view, absorbance 0.2, tint 1; the legs are timed against each other, alternately in one process, each on a scene
object of its own (same description, same camera):

  plain         (a) nt_render_device into fp32 x 3, the setting off
  xray          (b) the same with the setting on: the packet walk xray_packet, one launch
  counts        (c) scene.crossing_counts as a device tensor: the same walk without the factors and the packer
  transparent   (d) (a) on the same scene with every material's opacity set to 0.5: today's transparent route, which sorts and
                    blends in order and drops what lies beyond 24 hits a ray
  xray_var      (e) (b) under NTRACER_FORCE_VAR=1: the general route xray_var on the same scene

on the golden 120-cell, and (b), (c) on feature5_n5 (Solids in front of the walk) and feature16_n16 (the general route by itself).

The chip is settled the way tools/ao_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of
--leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/xray_time.py [--rounds 7] [--reps 10] [--frame 0]      one JSON line a scene, appended to profiles/xray_time.jsonl"""
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
ABSORBANCE, TINT = 0.2, 1.0
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")
FLAT_KEYS = ("root", "node_axis", "node_split", "node_left", "node_right", "items", "batch_recs", "batch_mats", "tri_recs", "tri_mats",
             "solid_recs", "solid_types", "solid_mats", "materials", "aabb_start", "aabb_end")

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


def measure(label, g, want):
    n = int(g["dimension"])
    f = int(g["frames"][args.frame])
    origin, axes = g["origins"][f], g["axes"][f]
    scenes, last = {}, {}
    for name in want:
        flat = {k: np.array(g[k]) for k in FLAT_KEYS}
        if name == "transparent":
            m = np.array(flat["materials"], np.float32).reshape(-1, 10).copy()
            m[:, 6] = 0.5
            flat["materials"] = m
        sc = tracern.CompositeScene.from_flat(n, flat)
        if "shadows" in g:
            sc.set_params_flat({k: g[k] for k in PARAM_KEYS if k in g})
        if "fov" in g:
            sc.set_fov(float(g["fov"]))
        sc._set_camera_arrays(origin, axes)
        if name.startswith("xray"):
            sc.set_xray(ABSORBANCE, TINT)
        scenes[name] = sc
    frames = {name: torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev) for name in want if name != "counts"}

    def leg(name):
        sc = scenes[name]
        if name == "counts":
            return lambda: last.__setitem__(name, sc.crossing_counts(W, H, device=dev))
        if name == "xray_var":
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
    out = {"scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "absorbance": ABSORBANCE, "tint": TINT,
           "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    if "counts" in last:
        c = last["counts"]
        out["largest_count"] = int(c.max())
        out["mean_count"] = round(float(c.float().mean()), 3)
        out["pixels_above_24_crossings"] = int((c > 24).sum())
    if "xray_var" in frames:
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(frames["xray"], frames["xray_var"]))
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
    for a, b in (("xray", "plain"), ("xray", "transparent"), ("xray_var", "xray"), ("counts", "xray")):
        if a in ms and b in ms:
            out["%s_over_%s" % (a, b)] = round(out[a]["median_ms"] / out[b]["median_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "xray_time.jsonl"), "a") as fh:
        fh.write(line + "\n")


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


measure("cell120_n4", golden("cell120_n4"), ("plain", "xray", "counts", "transparent", "xray_var"))
measure("feature5_n5", golden("feature5_n5"), ("plain", "xray", "counts"))
measure("feature16_n16", golden("feature16_n16"), ("plain", "xray", "counts"))
