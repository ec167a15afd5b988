#!/usr/bin/env python3
"""What the colours of caller-supplied rays cost next to a render of the same rays.  Not a test.

On the golden 120-cell and on BoxScene(6): the camera's own unnormalised rays of a 1920 x 1080 view, made on the device in
row-major order (ray y * 1920 + x is pixel (x, y)), timed against each other, alternately in one process:

  render         nt_render_device into fp32 x 3: the scene's own route (the 120-cell: the packet walk; BoxScene: the tile
                 kernel with its stretch codes), rays from the camera, a 12-byte store a pixel
  rays           nt_ray_colors_device on the same rays, an origin a ray: 8 n bytes a ray in, 12 out
  rays_shared    ... with one shared origin: 4 n bytes a ray in
  image_shared   nt_render_rays_device into fp32 x 3, shared origin: the image epilogue instead of rgb[ray]

The chip is settled the way tools/query_time.py settles it (untimed calls for 200 ms, then timed calls between
synchronisations); every leg reports the median of --rounds rounds of 20 calls and their spread.

  python3 tools/ray_colors_time.py [--rounds 9] [--frame 0]          one JSON line a scene"""
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
STREAM_TB_S = 5.7           # what the chip streams

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
fst = fmt._as_struct()
opts = _lib.NtRenderOpts()
opts.device = dev.index
L = _lib.lib()


def measure(label, sc, n, origin, axes):
    sc._set_camera_arrays(origin, axes)
    count = W * H
    # ---- the view's own rays (flat_origin_ray_source, tracer.hpp:60-76), unnormalised, row-major
    ray = torch.arange(count, device=dev)
    fov_i = math.tan(sc.fov / 2) / (W / 2)
    ax = torch.from_numpy(np.asarray(axes, np.float32)).to(dev)
    sx = (fov_i * ((ray % W).float() - W / 2))[:, None]
    sy = (fov_i * ((ray // W).float() - H / 2))[:, None]
    directions = ((ax[2][None] + ax[0][None] * sx) - ax[1][None] * sy).contiguous()
    one_origin = torch.from_numpy(np.asarray(origin, np.float32)).to(dev).contiguous()
    origins = one_origin[None].repeat(count, 1).contiguous()
    frame = torch.empty(fmt.pitch * H, dtype=torch.uint8, device=dev)
    image = torch.empty(fmt.pitch * H, dtype=torch.uint8, device=dev)
    rgb = torch.empty((count, 3), dtype=torch.float32, device=dev)
    each, shared = _lib.NtRays(), _lib.NtRays()
    each.count, each.origins, each.directions, each.shared_origin = count, origins.data_ptr(), directions.data_ptr(), 0
    shared.count, shared.origins, shared.directions, shared.shared_origin = count, one_origin.data_ptr(), directions.data_ptr(), 1
    stream = C.c_void_p(st.cuda_stream)

    def render():
        _lib.check(L.nt_render_device(sc._handle, C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(fst), C.byref(opts), stream))

    def colours(rays):
        _lib.check(L.nt_ray_colors_device(sc._handle, C.byref(rays), rgb.data_ptr(), C.byref(opts), stream))

    def image_shared():
        _lib.check(L.nt_render_rays_device(sc._handle, C.c_void_p(image.data_ptr()), image.numel(), C.byref(fst), C.byref(shared), C.byref(opts), stream))

    legs = {"render": render, "rays": lambda: colours(each), "rays_shared": lambda: colours(shared), "image_shared": image_shared}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the same picture either way (the packet walk and the stretch codes change no pixel): the share of pixels whose bytes agree
    same = float((frame.view(H * W, 12) == image.view(H * W, 12)).all(dim=1).float().mean())
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
    out = {"scene": label, "n": n, "frame": args.frame, "rays": count, "calls_a_round": REPS, "rounds": args.rounds,
           "pixels_with_the_renders_bytes": round(same, 6), "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4),
                     "Mrays_s": round(count / float(np.median(v)) / 1e3, 1)}
    base = out["render"]["median_ms"]
    for name, bytes_a_ray in (("rays", 8 * n + 12), ("rays_shared", 4 * n + 12), ("image_shared", 4 * n + 12)):
        out[name]["times_the_render"] = round(out[name]["median_ms"] / base, 3)
        out[name]["traffic_ms_at_%g_TB_s" % STREAM_TB_S] = round(count * bytes_a_ray / (STREAM_TB_S * 1e12) * 1e3, 4)
    print(json.dumps(out), flush=True)


g = np.load(os.path.join(HERE, "tests", "golden", "cell120_n4.npz"))
measure("cell120_n4", tracern.CompositeScene.from_flat(4, g), 4, g["origins"][args.frame], g["axes"][args.frame])
gb = np.load(os.path.join(HERE, "tests", "golden", "box_n6_1920x1080.npz"))
measure("BoxScene(6)", tracern.BoxScene(6), 6, gb["origins"][args.frame], gb["axes"][args.frame])
