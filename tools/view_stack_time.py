#!/usr/bin/env python3
"""What a view stack costs next to the plain render and next to what a caller pays for it without the feature (DESIGN.md
4.16).  Not a test.

A 1920 x 1080 RGBX8 view; the stack is aperture_disc(n, K, 0.06 dist) with focus = dist, dist the camera's distance from the
origin.  The legs of a measurement are timed against each other, alternately in one process, each on a scene object of its own:

  fused      the setting on: BoxScene's box_stack<N>, one launch, no sample in device memory
  frames     the same on a scene with set_view_stack_route("frames"): the plain render of the K sample cameras into fp32 x 3 scratch, then
             stack_resolve (the route of every composite scene, where it is the leg `stack`)
  by_hand    what a caller has without the feature: a CameraTable of the K sample cameras rendered into little-endian fp32 x 3 (a
             reversed format) and a torch weighted sum -- no packing, which flatters the leg
  plain      the setting off, one frame a camera
  k_plain    composite scenes: K plain RGBX8 renders, what the stack's rays cost without any summing

on BoxScene(6) and BoxScene(10) with K = 2, 8 and 16, one frame; the same legs for a table of --table-frames cameras at K = 8;
and on the golden 120-cell and feature5_n5 at K = 8 (stack, by_hand, k_plain, plain).

The chip is settled the way tools/cue_time.py settles it (untimed calls for 200 ms, then timed calls between events); every leg
reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs under an alarm of --leg-timeout
seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/view_stack_time.py [--rounds 7] [--reps 10]      one JSON line a measurement, appended to profiles/view_stack_time.jsonl"""
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
ap.add_argument("--leg-timeout", type=int, default=60, help="seconds a leg's warm-up, settling calls or one timed round may take")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--table-frames", type=int, default=160)
ap.add_argument("--only", default="", help="comma-separated: box, table, composite (default: all)")
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import tracern  # noqa: E402
from ntracer_amd.render import CameraTable  # noqa: E402

W, H = args.width, args.height
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")
ONLY = set(filter(None, args.only.split(","))) or {"box", "table", "composite"}

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
fmt_le = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32], 0, True)     # little-endian floats, (b, g, r)
renderer = ntracer_amd.BlockingRenderer()


class limit:
    """the calls of one leg under an alarm of their own, up to the synchronisation that ends them"""
    def __enter__(self):
        signal.alarm(args.leg_timeout)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        signal.alarm(0)


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


def measure(label, make, n, origins, axes, K, legs_wanted, centre):
    """origins [F][n], axes [F][n][n]: F = 1 renders the scene's own camera, F > 1 a camera table"""
    F = len(origins)
    dist = float(np.sqrt(((np.asarray(origins[0], np.float64) - centre) ** 2).sum()))
    off, wts = ntracer_amd.aperture_disc(n, K, 0.06 * dist)

    def scene(stack):
        sc = make()
        sc._set_camera_arrays(origins[0], axes[0])
        if stack:
            sc.set_view_stack(off, dist, wts)
        return sc
    on, plain_sc = scene(True), scene(False)
    on_frames = scene(True)
    on_frames.set_view_stack_route("frames")
    table = CameraTable(n, np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(axes, np.float32)) if F > 1 else None
    # by hand: the K sample cameras of every frame, frame-major, in a table of their own
    cams = [on.view_stack_cameras(_camera(n, origins[f], axes[f])) for f in range(F)]
    hand_table = CameraTable(n, np.concatenate([c[0] for c in cams]), np.concatenate([c[1] for c in cams]))
    hand_buf = torch.zeros(K * fmt_le.pitch * H, dtype=torch.uint8, device=dev)
    w_t = torch.tensor(np.ascontiguousarray(wts[:, ::-1]), device=dev)                          # (b, g, r) as the reversed format has them
    out_bytes = fmt.pitch * H
    bufs = {name: torch.zeros(F * out_bytes, dtype=torch.uint8, device=dev) for name in legs_wanted}
    last = {}

    def draw(sc, buf):
        if table is None:
            return lambda: renderer.render(buf, fmt, sc)
        return lambda: table.render(sc, buf, fmt, frame_bytes=out_bytes, first=0, count=F)

    def by_hand():
        for f in range(F):
            hand_table.render(plain_sc, hand_buf, fmt_le, frame_bytes=fmt_le.pitch * H, first=f * K, count=K)
            P = hand_buf.view(torch.float32).view(K, H, W, 3)
            last["by_hand"] = (P * w_t[:, None, None, :]).sum(dim=0)

    def k_plain():
        hand_table.render(plain_sc, kp_buf, fmt, frame_bytes=out_bytes, first=0, count=K)
    kp_buf = torch.zeros(K * out_bytes, dtype=torch.uint8, device=dev) if "k_plain" in legs_wanted else None
    legs = {}
    for name in legs_wanted:
        if name in ("fused", "stack"):
            legs[name] = draw(on, bufs[name])
        elif name == "frames":
            legs[name] = draw(on_frames, bufs[name])
        elif name == "by_hand":
            legs[name] = by_hand
        elif name == "k_plain":
            legs[name] = k_plain
        elif name == "plain":
            legs[name] = draw(plain_sc, bufs[name])
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": label, "n": n, "K": K, "nframes": F, "width": W, "height": H, "calls_a_round": args.reps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(dev)}
    if "fused" in bufs and "frames" in bufs:
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(bufs["fused"], bufs["frames"]))
    shown = "fused" if "fused" in bufs else "stack"
    if "plain" in bufs:
        out["pixels_the_setting_changes"] = int((bufs[shown].view(-1, 4) != bufs["plain"].view(-1, 4)).any(dim=1).sum())
    if "by_hand" in last:
        mine = bufs[shown][(F - 1) * out_bytes:].view(H, W, 4)[..., :3].float() / 255.0
        out["by_hand_max_abs_difference"] = float((mine - last["by_hand"].flip(2).clamp(0.0, 1.0)).abs().max())
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
    if "fused" in ms and "frames" in ms:
        out["fused_over_frames"] = round(out["fused"]["median_ms"] / out["frames"]["median_ms"], 3)
        out["fused_beats_frames_by_more_than_the_spread"] = bool(out["fused"]["max_ms"] < out["frames"]["min_ms"])
    if "by_hand" in ms:
        out["setting_over_by_hand"] = round(out[shown]["median_ms"] / out["by_hand"]["median_ms"], 3)
    if "k_plain" in ms:
        out["setting_over_k_plain"] = round(out[shown]["median_ms"] / out["k_plain"]["median_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "view_stack_time.jsonl"), "a") as f:
        f.write(line + "\n")


def _camera(n, origin, axes):
    c = tracern.Camera(n)
    c._origin, c._axes = np.ascontiguousarray(origin, np.float32), np.ascontiguousarray(axes, np.float32).reshape(n, n)
    return c


def composite(g):
    n = int(g["dimension"])

    def make():
        sc = tracern.CompositeScene.from_flat(n, g)
        if "shadows" in g:
            sc.set_params_flat({k: g[k] for k in PARAM_KEYS if k in g})
        return sc
    return make, n


BOX = {6: golden("box_n6_1920x1080"), 10: golden("box_n10_4096x4096")}
BOX_LEGS = ("fused", "frames", "by_hand", "plain")
if "box" in ONLY:
    for n, g in BOX.items():
        for K in (2, 8, 16):
            measure("box%d" % n, lambda n=n: tracern.BoxScene(n), n, g["origins"][:1], g["axes"][:1], K, BOX_LEGS, np.zeros(n))
if "table" in ONLY:
    for n, g in BOX.items():
        F = args.table_frames
        sel = np.arange(F) % len(g["origins"])
        measure("box%d table" % n, lambda n=n: tracern.BoxScene(n), n, g["origins"][sel], g["axes"][sel], 8, BOX_LEGS, np.zeros(n))
if "composite" in ONLY:
    for name in ("cell120_n4", "feature5_n5"):
        g = golden(name)
        make, n = composite(g)
        f = int(g["frames"][0])
        centre = 0.5 * (np.asarray(g["aabb_start"], np.float64) + np.asarray(g["aabb_end"], np.float64))
        measure(name, make, n, g["origins"][f:f + 1], g["axes"][f:f + 1], 8, ("stack", "by_hand", "k_plain", "plain"), centre)
