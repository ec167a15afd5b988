#!/usr/bin/env python3
"""What a render through a lens costs next to the plain render and next to the ray path.  Not a test.

A 1920 x 1080 view into fp32 x 3, the legs timed against each other, alternately in one process, each on a scene object
of its own (same description, same camera), so that no call switches a lens:

  plain          (a) nt_render_device, no lens: the scene's own route
  pinhole        (b) the same through Lens.pinhole -- identical pixels, so (b) - (a) is the cost of the mechanism alone
  fisheye        (c) through Lens.fisheye(fov 3.0)
  rays           (d) nt_render_rays_device on (b)'s directions, shared origin: what a lens cost before there were lenses

on the golden 120-cell (a, b, c, d), BoxScene(6) (a, b, d), the 120-cell lit -- shadows, two point lights, a global light,
30 % reflective -- and feature5_n5, whose materials are transparent (a, b).  (b) - (a) is set against the model of DESIGN 4.7:
16 + 16 + 12 bytes a pixel at the streaming rate.

The chip is settled the way tools/ray_colors_time.py settles it (untimed calls for 200 ms, then timed calls between
synchronisations); every leg reports the median of --rounds rounds of 20 calls and their spread.

  python3 tools/lens_time.py [--rounds 9] [--frame 0]          one JSON line a scene"""
import argparse
import ctypes as C
import json
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
from ntracer_amd import Lens, _lib, tracern  # noqa: E402

W, H = 1920, 1080
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
REPS = 20
STREAM_TB_S = 5.7           # what the chip streams
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


def measure(label, make, n, origin, axes, want):
    pinhole_lens = None
    scenes, frames, legs = {}, {}, {}
    for name in want:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        if name == "pinhole":
            pinhole_lens = Lens.pinhole(W, H, sc.fov)
            sc.set_lens(pinhole_lens)
        elif name == "fisheye":
            sc.set_lens(Lens.fisheye(W, H, 3.0))
        scenes[name] = sc
        frames[name] = torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev)
    if "rays" in want:
        cam = tracern.Camera(n)
        cam._origin, cam._axes = np.asarray(origin, np.float32), np.asarray(axes, np.float32)
        directions = torch.from_numpy(pinhole_lens.directions(cam)).to(dev).contiguous()
        one_origin = torch.from_numpy(np.asarray(origin, np.float32)).to(dev).contiguous()
        rays = _lib.NtRays()
        rays.count, rays.origins, rays.directions, rays.shared_origin = W * H, one_origin.data_ptr(), directions.data_ptr(), 1

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
    same = {name: float((frames["plain"].view(H * W, 12) == frames[name].view(H * W, 12)).all(dim=1).float().mean())
            for name in want if name in ("pinhole", "rays")}
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
    out = {"scene": label, "n": n, "frame": args.frame, "pixels": W * H, "calls_a_round": REPS, "rounds": args.rounds,
           "pixels_with_the_plain_renders_bytes": {k: round(v, 6) for k, v in same.items()}, "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    if "pinhole" in ms:
        out["pinhole_minus_plain_ms"] = round(out["pinhole"]["median_ms"] - out["plain"]["median_ms"], 4)
        out["model_44_bytes_a_pixel_ms_at_%g_TB_s" % STREAM_TB_S] = round(W * H * 44 / (STREAM_TB_S * 1e12) * 1e3, 4)
    if "rays" in ms and "pinhole" in ms:
        out["rays_over_pinhole"] = round(out["rays"]["median_ms"] / out["pinhole"]["median_ms"], 3)
    print(json.dumps(out), flush=True)


def golden(name):
    return np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))


def composite(g, lit=False):
    n = int(g["dimension"])

    def make():
        if not lit:
            sc = tracern.CompositeScene.from_flat(n, g)
            if "shadows" in g:
                sc.set_params_flat({k: g[k] for k in PARAM_KEYS if k in g})
            return sc
        flat = {k: g[k] for k in tracern._FLAT_KEYS}
        m = np.array(flat["materials"], np.float32).copy()
        m[:, 7] = 0.3
        flat["materials"] = m
        sc = tracern.CompositeScene.from_flat(n, flat)
        lo, hi = np.asarray(g["aabb_start"], np.float32), np.asarray(g["aabb_end"], np.float32)
        ctr, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
        strength = float(np.linalg.norm(ext)) ** (n - 1)
        gdir = np.resize(np.array([0.2, -0.9, 0.3, 0.1], np.float32), n)
        sc.set_params_flat(dict(shadows=1, camera_light=1, max_reflect_depth=4, bg_gradient_axis=1, ambient=np.array([0.02, 0.02, 0.03], np.float32),
                                bg1=np.array([1, 1, 1], np.float32), bg2=np.array([0, 0, 0], np.float32), bg3=np.array([0, 1, 1], np.float32),
                                point_light_pos=np.array([ctr + ext * 3.0 * np.resize(np.array([1.0, 0.8, -0.9, 0.4], np.float32), n),
                                                          ctr + ext * 0.15 * np.resize(np.array([-0.5, 0.3, 0.2, -0.4], np.float32), n)], np.float32),
                                point_light_color=np.array([[40.0 * strength] * 3, [0.5 * strength] * 3], np.float32),
                                global_light_dir=np.array([gdir / np.linalg.norm(gdir)], np.float32),
                                global_light_color=np.array([[0.4, 0.4, 0.5]], np.float32)))
        return sc
    return make, n


g = golden("cell120_n4")
make, n = composite(g)
measure("cell120_n4", make, n, g["origins"][args.frame], g["axes"][args.frame], ("plain", "pinhole", "fisheye", "rays"))
gb = golden("box_n6_1920x1080")
measure("BoxScene(6)", lambda: tracern.BoxScene(6), 6, gb["origins"][args.frame], gb["axes"][args.frame], ("plain", "pinhole", "rays"))
make, n = composite(g, lit=True)
measure("cell120_n4 lit", make, n, g["origins"][args.frame], g["axes"][args.frame], ("plain", "pinhole"))
g5 = golden("feature5_n5")
make, n = composite(g5)
f5 = int(g5["frames"][0])
measure("feature5_n5", make, n, g5["origins"][f5], g5["axes"][f5], ("plain", "pinhole"))
