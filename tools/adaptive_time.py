#!/usr/bin/env python3
"""What adaptive supersampling costs and saves.  One process, the chip settled, one JSON line per (scene, s);
the five legs of a line alternate within a round, and every leg reports the median of --rounds rounds with their spread:

  a  plain                       the factor 1
  b  full supersampling          the factor s
  c  adaptive, t = 0.1           the factor s, only the flagged pixels refined
  d  adaptive, t = -1            every pixel flagged: the refine route priced against (b), ray for ray
  e  adaptive, t = 2             no pixel flagged: the mechanism alone -- (e) - (a) against its model, one fp32 frame written and
                                 read (24 bytes a pixel) and two launches more

1920 x 1080 RGBX8 into device memory (nt_render_device), and the drop-in host call (BlockingRenderer.render into a bytearray)
for legs a, b and c.  Scenes: BoxScene(6), the golden 120-cell, the 120-cell lit (tools/lens_time.py's variant), feature5_n5.
The flagged share of each threshold is recorded with the line.

  python3 tools/adaptive_time.py [--rounds 7] [--factors 2,4] [--scenes box6,cell120,cell120lit,feature5] >> profiles/adaptive_time.jsonl"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frame", type=int, default=0, help="camera of the golden sequence")
ap.add_argument("--factors", default="2,4")
ap.add_argument("--scenes", default="box6,cell120,cell120lit,feature5")
ap.add_argument("--threshold", type=float, default=0.1)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402

W, H = 1920, 1080
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
SETTLE_MS = 200.0
STREAM_TB_S = 5.7           # what the chip streams
PARAM_KEYS = ("shadows", "camera_light", "max_reflect_depth", "bg_gradient_axis", "ambient", "bg1", "bg2", "bg3", "point_light_pos",
              "point_light_color", "global_light_dir", "global_light_color")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
fst = fmt._as_struct()
opts = _lib.NtRenderOpts()
opts.device = dev.index
L = _lib.lib()
stream = C.c_void_p(st.cuda_stream)


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
    return make


def spread(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


LEGS = (("a_plain", 1, None), ("b_full", 0, None), ("c_adaptive", 0, args.threshold), ("d_adaptive_all", 0, -1.0), ("e_adaptive_none", 0, 2.0))


def measure(label, make, origin, axes, s):
    scenes, frames = {}, {}
    for name, factor, t in LEGS:
        sc = make()
        sc._set_camera_arrays(origin, axes)
        sc.set_supersampling(factor or s)
        sc.set_adaptive_supersampling(t)
        scenes[name] = sc
        frames[name] = torch.zeros(fmt.pitch * H, dtype=torch.uint8, device=dev)

    def leg(name):
        sc, frame = scenes[name], frames[name]
        return lambda: _lib.check(L.nt_render_device(sc._handle, C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(fst), C.byref(opts), stream))
    legs = {name: leg(name) for name, _, _ in LEGS}
    reps = {}
    for name, fn in legs.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(2, min(20, int(40.0 / max((time.perf_counter() - t0) * 1e3, 0.05))))
    share = float(scenes["c_adaptive"].refinement_mask(W, H, device=dev).float().mean())
    same = {"d_equals_b": float((frames["d_adaptive_all"] == frames["b_full"]).float().mean()),
            "e_equals_a": float((frames["e_adaptive_none"] == frames["a_plain"]).float().mean())}
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():              # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps[name]):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps[name])
    out = {"scene": label, "s": s, "threshold": args.threshold, "flagged_share": round(share, 5), "pixels": W * H, "rounds": args.rounds,
           "calls_a_round": reps, "bytes_equal": {k: round(v, 6) for k, v in same.items()}, "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        out[name] = spread(v)
    a, b, c, d, e = (out[name]["median_ms"] for name, _, _ in LEGS)
    out["e_minus_a_ms"] = round(e - a, 4)
    out["model_24_bytes_a_pixel_ms_at_%g_TB_s" % STREAM_TB_S] = round(W * H * 24 / (STREAM_TB_S * 1e12) * 1e3, 4)
    out["c_over_b"] = round(c / b, 3)
    out["d_over_b"] = round(d / b, 3)
    out["break_even_share_by_d"] = round((b - e) / max(d - e, 1e-9), 4)      # the share at which (c) meets (b), if refining scales with it
    # the drop-in host call: legs a, b, c, a frame each in turn
    r = ntracer_amd.BlockingRenderer()
    buf = bytearray(fmt.pitch * H)
    host = {name: [] for name in ("a_plain", "b_full", "c_adaptive")}
    for name in host:
        r.render(buf, fmt, scenes[name])
    for _ in range(args.rounds):
        for name in host:
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                r.render(buf, fmt, scenes[name])
                t.append((time.perf_counter() - t0) * 1e3)
            host[name].append(float(np.median(t)))
    out["dropin"] = {name: spread(v) for name, v in host.items()}
    print(json.dumps(out), flush=True)


SCENES = {}
gb = golden("box_n6_1920x1080")
SCENES["box6"] = ("BoxScene(6)", lambda: tracern.BoxScene(6), gb["origins"][args.frame], gb["axes"][args.frame])
g = golden("cell120_n4")
SCENES["cell120"] = ("cell120_n4", composite(g), g["origins"][args.frame], g["axes"][args.frame])
SCENES["cell120lit"] = ("cell120_n4 lit", composite(g, lit=True), g["origins"][args.frame], g["axes"][args.frame])
g5 = golden("feature5_n5")
f5 = int(g5["frames"][0])
SCENES["feature5"] = ("feature5_n5", composite(g5), g5["origins"][f5], g5["axes"][f5])

for key in args.scenes.split(","):
    label, make, o, a = SCENES[key]
    for s in (int(v) for v in args.factors.split(",")):
        measure(label, make, o, a, s)
        torch.cuda.empty_cache()
