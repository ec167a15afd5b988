#!/usr/bin/env python3
"""What supersampling costs.  One process, one JSON line per leg; every leg is settled the way bench.py
settles (untimed calls for 200 ms, then timed calls between synchronisations) and reports the median of ROUNDS rounds with
their spread (min .. max).

  python3 tools/ss_time.py [--tree DIR] [--rounds 7] [--scratch-mb M] leg ...

legs (scene: box6 | cell120; 1920 x 1080 throughout):
  device:SCENE:S:FRAMES   nt_render_frames_device, FRAMES frames a call, RGBX8, the scene's factor set to S: ms a call
  hires:SCENE:S:FRAMES    the same entry point drawing the S*1920 x S*1080 plain fp32 x 3 frames with one ray a pixel -- the
                          first stage of the supersampled call on its own, and what a library without the feature can do
  dropin:SCENE:S          BlockingRenderer().render(bytearray, RGBX8, scene) with the factor set to S: ms a frame, wall clock
  dropin_hires:SCENE:S    ... drawing the S*1920 x S*1080 fp32 x 3 frame into host memory with one ray a pixel (what a user
                          without the feature has to do before averaging on the CPU)

--tree DIR imports ntracer_amd from another checkout (a build of the parent commit: the yardstick legs hires / dropin_hires
and every leg with S = 1 run there unchanged; legs with S > 1 need the feature)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--scratch-mb", type=int, default=0, help="cap of the sample scratch (scene.set_supersampling_scratch_mb); 0: the default")
ap.add_argument("legs", nargs="+")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402

W, H = 1920, 1080
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
GOLDEN = os.path.join(HERE, "tests", "golden")
SETTLE_MS = 200.0


def make(scene):
    if scene == "box6":
        g = np.load(os.path.join(GOLDEN, "box_n6_1920x1080.npz"))
        return tracern.BoxScene(6), g["origins"], g["axes"]
    g = np.load(os.path.join(GOLDEN, "cell120_n4.npz"))
    return tracern.CompositeScene.from_flat(4, g), g["origins"], g["axes"]


def set_factor(sc, s):
    if s != 1:
        sc.set_supersampling(s)           # (AttributeError on a library without the feature)
        if args.scratch_mb:
            sc.set_supersampling_scratch_mb(args.scratch_mb)


def settle(fn):
    t0 = time.perf_counter()
    k = 0
    while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
        fn()
        k += 1
        if k % 8 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(min(ms)), 4), "max_ms": round(float(max(ms)), 4), "rounds": len(ms)}


def device_leg(scene, s, frames, hires):
    sc, origins, axes = make(scene)
    if hires:
        fmt = ntracer_amd.ImageFormat(s * W, s * H, [ntracer_amd.Channel(*c) for c in RGBF32])
    else:
        set_factor(sc, s)
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
    fst = fmt._as_struct()
    frame_bytes = fmt.pitch * fmt.height
    fb = torch.empty((frames, frame_bytes), dtype=torch.uint8, device="cuda")
    o = np.ascontiguousarray(origins[:frames], np.float32)
    a = np.ascontiguousarray(axes[:frames], np.float32)
    st = torch.cuda.current_stream()

    def go():
        _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(fb.data_ptr()), frame_bytes, frames, o.ctypes.data_as(_lib.f32p),
                                                      a.ctypes.data_as(_lib.f32p), C.byref(fst), None, C.c_void_p(st.cuda_stream)))
    for _ in range(3):
        go()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go()
    torch.cuda.synchronize()
    reps = max(2, min(50, int(60.0 / max((time.perf_counter() - t0) * 1e3, 0.05))))
    settle(go)
    ms = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            go()
        e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    out = spread(ms)
    out.update(frames_a_call=frames, calls_a_round=reps, rays_a_call=frames * s * s * W * H)
    out["Grays_s"] = round(out["rays_a_call"] / out["median_ms"] / 1e6, 2)
    return out


def dropin_leg(scene, s, hires):
    sc, origins, axes = make(scene)
    if hires:
        fmt = ntracer_amd.ImageFormat(s * W, s * H, [ntracer_amd.Channel(*c) for c in RGBF32])
    else:
        set_factor(sc, s)
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
    r = ntracer_amd.BlockingRenderer()
    buf = bytearray(fmt.pitch * fmt.height)
    k = [0]

    def go():
        f = k[0] % len(origins)
        k[0] += 1
        sc._set_camera_arrays(origins[f], axes[f])
        r.render(buf, fmt, sc)
    for _ in range(3):
        go()
    t0 = time.perf_counter()
    go()
    reps = max(3, min(40, int(100.0 / max((time.perf_counter() - t0) * 1e3, 0.05))))
    settle(go)
    ms = []
    for _ in range(args.rounds):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            go()
            t.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(np.median(t)))
    out = spread(ms)
    out.update(frames_a_round=reps, bytes_to_host=len(buf))
    return out


for leg in args.legs:
    parts = leg.split(":")
    kind, scene, s = parts[0], parts[1], int(parts[2])
    try:
        if kind in ("device", "hires"):
            res = device_leg(scene, s, int(parts[3]), kind == "hires")
        elif kind in ("dropin", "dropin_hires"):
            res = dropin_leg(scene, s, kind == "dropin_hires")
        else:
            raise SystemExit("unknown leg %r" % leg)
    except AttributeError as e:
        res = {"skipped": "this library has no supersampling (%s)" % e}
    res = dict({"leg": leg, "tree": os.path.relpath(ROOT, HERE), "scratch_mb": args.scratch_mb or "default"}, **res)
    print(json.dumps(res), flush=True)
    torch.cuda.empty_cache()
