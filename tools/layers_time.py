#!/usr/bin/env python3
"""What the hit layers cost next to the walks they are built on, and next to what a caller composes without them.
Not a test.

A 1920 x 1080 view; the legs are timed against each other, alternately in one process, on one scene object (none of them changes
a setting), every result a device tensor:

  primary_hits   (a) scene.primary_hits: the nearest-hit walk, which prunes
  counts         (b) scene.crossing_counts: the layers' walk without the list (xray_packet / xray_var)
  layers_1 .. 8  (c) scene.hit_layers at 1, 2, 4 and 8 layers
  layers_8_var   (d) (c) at 8 under NTRACER_FORCE_VAR=1: the general route layers_var on the same scene
  composed_8     (e) what a caller composes today: 8 passes of intersect_rays on the view's own rays, t_near / skip_item /
                     skip_lane of each pass taken from the pass before.  NOT the same answer: where two crossings share a distance
                     the second pass skips only one primitive and then steps past the other, and a transparent surface is no
                     hit of such a pass at all; it is here for its cost alone

on the golden 120-cell, feature5_n5 (Solids in front of the walk) and feature16_n16 (the general route by itself, where (d) is (c)).

The chip is settled the way tools/xray_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of
--leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/layers_time.py [--rounds 7] [--reps 10] [--frame 0] [--out profiles/layers_time.jsonl]      one JSON line a scene, appended"""
import argparse
import json
import math
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
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "layers_time.jsonl"))
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
from ntracer_amd import tracern  # noqa: E402

W, H = args.width, args.height
SETTLE_MS = 200.0
FLT_MAX = float(np.finfo(np.float32).max)
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")
FLAT_KEYS = ("root", "node_axis", "node_split", "node_left", "node_right", "items", "batch_recs", "batch_mats", "tri_recs", "tri_mats",
             "solid_recs", "solid_types", "solid_mats", "materials", "aabb_start", "aabb_end")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()


class limit:
    """the calls of one leg under an alarm of their own, up to the synchronisation that ends them"""
    def __enter__(self):
        signal.alarm(args.leg_timeout)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        signal.alarm(0)


def view_rays(origin, axes, fov, n):
    """the pinhole's rays of the view as device tensors (timing only: rounded as numpy rounds them, not as the kernels do)"""
    half_w, half_h = W / 2.0, H / 2.0
    k = math.tan(fov / 2) / half_w
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    sx, sy = (k * (xs - half_w)).reshape(-1, 1), (k * (ys - half_h)).reshape(-1, 1)
    d = axes[2][None] + axes[0][None] * sx - axes[1][None] * sy
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.repeat(np.asarray(origin, np.float32)[None], len(d), axis=0)
    return torch.from_numpy(np.ascontiguousarray(o)).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev)


def measure(label, g, want):
    n = int(g["dimension"])
    f = int(g["frames"][args.frame])
    origin, axes = g["origins"][f], g["axes"][f]
    flat = {k: np.array(g[k]) for k in FLAT_KEYS}
    sc = tracern.CompositeScene.from_flat(n, flat)
    if "shadows" in g:
        sc.set_params_flat({k: g[k] for k in PARAM_KEYS if k in g})
    fov = float(g["fov"]) if "fov" in g else 0.8
    sc.set_fov(fov)
    sc._set_camera_arrays(origin, axes)
    ro, rd = view_rays(origin, np.asarray(axes, np.float32).reshape(n, n), fov, n)
    last = {}

    def composed():
        t_near = skip_item = skip_lane = None
        for _ in range(8):
            r = sc.intersect_rays(ro, rd, t_near=t_near, skip_item=skip_item, skip_lane=skip_lane)
            hit = r["kind"] >= 0
            t_near = torch.where(hit, r["dist"], torch.full_like(r["dist"], FLT_MAX)).contiguous()
            skip_item = torch.where(hit, (r["index"] << 2) | r["kind"], torch.full_like(r["index"], -1)).contiguous()
            skip_lane = r["lane"].contiguous()
        last["composed_8"] = r

    def forced():
        os.environ["NTRACER_FORCE_VAR"] = "1"       # (the switches are read at every call)
        try:
            last["layers_8_var"] = sc.hit_layers(W, H, 8, device=dev)
        finally:
            del os.environ["NTRACER_FORCE_VAR"]

    def layers(k):
        return lambda: last.__setitem__("layers_%d" % k, sc.hit_layers(W, H, k, device=dev))
    legs = {"primary_hits": lambda: last.__setitem__("primary_hits", sc.primary_hits(W, H, device=dev)),
            "counts": lambda: last.__setitem__("counts", sc.crossing_counts(W, H, device=dev)),
            "layers_1": layers(1), "layers_2": layers(2), "layers_4": layers(4), "layers_8": layers(8),
            "layers_8_var": forced, "composed_8": composed}
    legs = {name: legs[name] for name in want}
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "calls_a_round": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(dev)}
    c = last["counts"]
    out["largest_count"] = int(c.max())
    out["mean_count"] = round(float(c.float().mean()), 3)
    out["pixels_cut_at_8"] = int((c > 8).sum())
    out["layers_8_count_is_crossing_counts"] = bool(torch.equal(last["layers_8"].count, c))
    if "layers_8_var" in last:
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(last["layers_8"].records, last["layers_8_var"].records))
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
    for a, b in (("layers_1", "counts"), ("layers_8", "counts"), ("layers_8", "primary_hits"), ("layers_8", "composed_8"), ("layers_8_var", "layers_8")):
        if a in ms and b in ms:
            out["%s_over_%s" % (a, b)] = round(out[a]["median_ms"] / out[b]["median_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


ALL = ("primary_hits", "counts", "layers_1", "layers_2", "layers_4", "layers_8", "layers_8_var", "composed_8")
measure("cell120_n4", golden("cell120_n4"), ALL)
measure("feature5_n5", golden("feature5_n5"), ALL)
measure("feature16_n16", golden("feature16_n16"), tuple(l for l in ALL if l != "layers_8_var"))
