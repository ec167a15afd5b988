#!/usr/bin/env python3
"""What ambient occlusion costs next to the plain render, and next to the same counts composed from the public API without it
(DESIGN.md 4.10).  Not a test.

A 1920 x 1080 view with K = 16 samples (sphere_directions(n, 16)), radius 1, bias 1e-3; the legs are timed against each other,
alternately in one process, each on a scene object of its own (same description, same camera):

  plain          (a) nt_render_device into fp32 x 3, the setting off
  ao_render      (b) the same with the setting on
  counts         (c) scene.occlusion_counts on the device
  composed       (d) the same counts without the feature: scene.primary_hits(normals=True) on the device, the hit pixels' rays
                     expanded in torch (the primary directions are made once, outside the timing), scene.intersect_rays on the
                     device, the K answers of a pixel summed in torch

on the golden 120-cell (a, b, c, d: the fast route) and on feature5_n5 (b, c: the ray route).  (c) and (d) must give the same
counts: the share of equal pixels is reported.

The chip is settled the way tools/lens_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds of --reps calls and their spread, so that a difference between two legs can be set
against the spread of one.  Every call of a leg -- its warm-up, its share of the settling, each of its timed rounds -- runs under an
alarm of --leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/ao_time.py [--rounds 7] [--reps 10] [--frame 0]          one JSON line a scene, appended to profiles/ao_time.jsonl"""
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
K, RADIUS, BIAS = 16, 1.0, 1e-3
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


def primary_directions(sc, origin, axes):
    """the unit directions of the view's primary rays, [H * W][n] on the device, by primary_dir's operations"""
    a = torch.from_numpy(np.asarray(axes, np.float32)).to(dev)
    half_w, half_h = np.float32(W) / np.float32(2), np.float32(H) / np.float32(2)
    fov_i = np.float32(np.tan(np.float32(sc.fov) / np.float32(2))) / half_w
    sx = (torch.arange(W, device=dev, dtype=torch.float32) - float(half_w)) * float(fov_i)
    sy = (torch.arange(H, device=dev, dtype=torch.float32) - float(half_h)) * float(fov_i)
    d = (a[2][None, None, :] + a[0][None, None, :] * sx[None, :, None]) - a[1][None, None, :] * sy[:, None, None]
    return (d / d.norm(dim=2, keepdim=True)).reshape(H * W, -1).contiguous()


def composed_counts(sc, d, T):
    """leg (d): what a caller of the parent commit's API writes to get the counts"""
    n = sc.dimension
    ph = sc.primary_hits(W, H, normals=True, device=dev)
    item = ph.item.reshape(-1)
    hit = torch.nonzero(item >= 0).reshape(-1)
    blocked = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
    if hit.numel() == 0:
        return blocked.reshape(H, W)
    no, nd = ph.normal_origin.reshape(-1, n)[hit], ph.normal_dir.reshape(-1, n)[hit]
    side = -(d[hit] * nd).sum(dim=1)
    b = torch.where(side < 0, -BIAS, BIAS).to(torch.float32)
    o2 = no + nd * b[:, None]
    flip = ((nd @ T.t()) < 0) != (side < 0)[:, None]
    v = torch.where(flip[:, :, None], -T[None], T[None])
    count = hit.numel() * K
    r = sc.intersect_rays(o2[:, None, :].expand(-1, K, -1).reshape(count, n).contiguous(), v.reshape(count, n).contiguous(),
                          t_near=torch.zeros(count, device=dev), t_far=torch.full((count,), RADIUS, device=dev),
                          skip_item=item[hit].repeat_interleave(K).contiguous(), skip_lane=ph.lane.reshape(-1)[hit].repeat_interleave(K).contiguous())
    blocked[hit] = ((r["kind"] >= 0) & (r["dist"] <= RADIUS)).reshape(-1, K).sum(dim=1).to(torch.int32)
    return blocked.reshape(H, W)


def measure(label, make, n, origin, axes, want):
    scenes, legs, last = {}, {}, {}
    T_host = ntracer_amd.sphere_directions(n, K)
    T = torch.from_numpy(T_host).to(dev)
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name in ("ao_render", "counts"):
            sc.set_ambient_occlusion(T_host, RADIUS, bias=BIAS)
        scenes[name] = sc
    frames = {name: torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev) for name in ("plain", "ao_render") if name in want}
    d = primary_directions(scenes[want[0]], origin, axes) if "composed" in want else None

    def leg(name):
        sc = scenes[name]
        if name in frames:
            return lambda: renderer.render(frames[name], fmt, sc)
        if name == "counts":
            return lambda: last.__setitem__(name, sc.occlusion_counts(W, H, device=dev))
        return lambda: last.__setitem__(name, composed_counts(sc, d, T))
    legs = {name: leg(name) for name in want}
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": label, "n": n, "frame": args.frame, "width": W, "height": H, "samples": K, "radius": RADIUS, "bias": BIAS,
           "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    if "counts" in last:
        c = last["counts"]
        out["pixels_with_a_hit"] = int((c >= 0).sum())
        out["pixels_blocked"] = int((c > 0).sum())
        if "composed" in last:
            out["share_of_pixels_where_composed_equals_counts"] = round(float((c == last["composed"]).float().mean()), 6)
    if "ao_render" in frames and "plain" in frames:
        out["share_of_pixels_the_setting_changes"] = round(float((frames["plain"].view(H * W, 12) != frames["ao_render"].view(H * W, 12)).any(dim=1).float().mean()), 6)
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
    if "ao_render" in ms and "plain" in ms:
        out["ao_render_minus_plain_ms"] = round(out["ao_render"]["median_ms"] - out["plain"]["median_ms"], 4)
    if "composed" in ms and "counts" in ms:
        out["composed_over_counts"] = round(out["composed"]["median_ms"] / out["counts"]["median_ms"], 3)
        out["counts_beats_composed_by_more_than_the_spread"] = bool(out["counts"]["max_ms"] < out["composed"]["min_ms"])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "ao_time.jsonl"), "a") as f:
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
measure("cell120_n4", make, n, g["origins"][f], g["axes"][f], ("plain", "ao_render", "counts", "composed"))
g5 = golden("feature5_n5")
make, n = composite(g5)
f5 = int(g5["frames"][args.frame])
measure("feature5_n5", make, n, g5["origins"][f5], g5["axes"][f5], ("ao_render", "counts"))
