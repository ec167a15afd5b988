#!/usr/bin/env python3
"""What a render under the parallel projection costs next to the plain render and next to the ray path.  Not a
test.

A 1920 x 1080 view into fp32 x 3, the legs timed against each other, alternately in one process, each on a scene object of
its own (same description, same camera), so that no call switches the projection:

  plain          (a) nt_render_device, the pinhole: for context
  parallel       (b) the same scene with set_parallel_projection(half_width)
  rays           (c) nt_render_rays_device on (b)'s own rays (Scene.parallel_rays: one origin a ray, one direction repeated):
                     what a caller had to do before the projection was a scene setting

on the golden 120-cell (a, b, c), whose half_width is tan(0.4) x the distance from the camera to the centre of the scene's
box -- the scene then fills the frame about as the 0.8 rad pinhole has it -- and, through the ray route, on BoxScene(6)
(half_width 1.5) and feature5_n5 (half the largest extent of its box) with (b) and (c) alone.

The chip is settled the way tools/lens_time.py settles it (untimed calls for 200 ms, then timed calls between
synchronisations); every leg reports the median of --rounds rounds of 20 calls and their spread.

  python3 tools/parallel_time.py [--rounds 9] [--frame 0]          one JSON line a scene"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--frame", type=int, default=0, help="camera of the golden sequence")
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402

W, H = 1920, 1080
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
REPS = 20
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
fst = fmt._as_struct()
opts = _lib.NtRenderOpts()
opts.device = dev.index
L = _lib.lib()
stream = C.c_void_p(st.cuda_stream)


def measure(label, make, n, origin, axes, half_width, want):
    scenes, frames = {}, {}
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name == "parallel":
            sc.set_parallel_projection(half_width)
        scenes[name] = sc
        frames[name] = torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev)
    if "rays" in want:
        org, fwd = scenes["parallel"].parallel_rays(W, H)
        origins = torch.from_numpy(org).to(dev).contiguous()
        directions = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(fwd, org.shape))).to(dev).contiguous()
        rays = _lib.NtRays()
        rays.count, rays.origins, rays.directions, rays.shared_origin = W * H, origins.data_ptr(), directions.data_ptr(), 0

    def leg(name):
        sc, frame = scenes[name], frames[name]
        if name == "rays":
            return lambda: _lib.check(L.nt_render_rays_device(sc._handle, C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(fst), C.byref(rays),
                                                              C.byref(opts), stream))
        return lambda: _lib.check(L.nt_render_device(sc._handle, C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(fst), C.byref(opts), stream))
    legs = {name: leg(name) for name in want}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = {}
    if "rays" in want:
        same["rays"] = float((frames["parallel"].view(H * W, 12) == frames["rays"].view(H * W, 12)).all(dim=1).float().mean())
    px = frames["parallel"].view(H * W, 12)
    not_background = float((px != px[0]).any(dim=1).float().mean())         # (pixel (0, 0) looks past every scene here)
    t0 = time.perf_counter()
    k = 0
    while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
        for fn in legs.values():
            fn()
        k += 1
        if k % 8 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():              # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(REPS):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REPS)
    out = {"scene": label, "n": n, "frame": args.frame, "pixels": W * H, "half_width": round(float(half_width), 6), "calls_a_round": REPS,
           "rounds": args.rounds, "pixels_with_the_parallel_renders_bytes": {k: round(v, 6) for k, v in same.items()},
           "pixels_unlike_pixel_0": round(not_background, 4), "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    if "rays" in ms:
        out["rays_over_parallel"] = round(out["rays"]["median_ms"] / out["parallel"]["median_ms"], 3)
        out["spreads_overlap"] = bool(max(out["parallel"]["min_ms"], out["rays"]["min_ms"]) <= min(out["parallel"]["max_ms"], out["rays"]["max_ms"]))
    if "plain" in ms:
        out["parallel_over_plain"] = round(out["parallel"]["median_ms"] / out["plain"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


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


def box(g):
    return np.asarray(g["aabb_start"], np.float32), np.asarray(g["aabb_end"], np.float32)


g = golden("cell120_n4")
make, n = composite(g)
lo, hi = box(g)
o = np.asarray(g["origins"][args.frame], np.float32)
hw = math.tan(0.4) * float(np.linalg.norm(o.astype(np.float64) - 0.5 * (lo.astype(np.float64) + hi)))
measure("cell120_n4", make, n, o, g["axes"][args.frame], hw, ("plain", "parallel", "rays"))
gb = golden("box_n6_1920x1080")
measure("BoxScene(6)", lambda: tracern.BoxScene(6), 6, gb["origins"][args.frame], gb["axes"][args.frame], 1.5, ("parallel", "rays"))
g5 = golden("feature5_n5")
make, n = composite(g5)
lo, hi = box(g5)
f5 = int(g5["frames"][0])
measure("feature5_n5", make, n, g5["origins"][f5], g5["axes"][f5], 0.5 * float((hi - lo).max()), ("parallel", "rays"))
