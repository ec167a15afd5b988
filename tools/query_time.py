#!/usr/bin/env python3
"""What a batched ray query costs next to the render of the same rays.  Not a test.

The rays are the primary rays of one 1920 x 1080 frame of the golden 120-cell, generated on the device in 8 x 8-tile order
(ray 64 t + 8 j + i is pixel (8 tx + i, 8 ty + j) of tile t = ty * 240 + tx), so that a wave of the query kernel holds the
rays a wave of the per-lane tile kernel holds.  Timed against each other, alternately in one process:

  render   nt_render_device, fp32 x 3, NTRACER_COMPOSITE_KERNEL=2: composite_kernel<4, false, false>, the same walk with the
           same lane-per-ray layout, plus the camera arithmetic, the shading and a 12-byte store a ray
  query    nt_intersect_rays_device on the same rays: 8 n bytes of loads and a 16-byte store a ray
  normals  ... with normal_origin / normal_dir: 8 n more bytes a ray
  boxed    the query on the rays that enter the scene's box only, started at their entry distance: what the render's
           aabb_distance test, which KDNode.intersects does not have, spares the render

The chip is settled the way tools/ss_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds and their spread.  The expectation the query is held against is the render's
time plus the query's extra traffic, count * (8 n + 16) bytes (8 n more with normals) at the rate the chip streams (DESIGN.md
4.1: 5.7 TB/s), with a margin of 10 % because the pool's boxes differ by several per cent even within one process.

  python3 tools/query_time.py [--rounds 9] [--frame 0]          one JSON line"""
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
os.environ["NTRACER_COMPOSITE_KERNEL"] = "2"          # the render leg: the plain per-lane tile kernel (a query does not read it)
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402

W, H, N = 1920, 1080, 4
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
SETTLE_MS = 200.0
STREAM_TB_S = 5.7
MARGIN = 1.10

g = np.load(os.path.join(HERE, "tests", "golden", "cell120_n4.npz"))
sc = tracern.CompositeScene.from_flat(N, g)
origin, axes = np.asarray(g["origins"][args.frame], np.float32), np.asarray(g["axes"][args.frame], np.float32)
sc._set_camera_arrays(origin, axes)
dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()

# ---- the frame's primary rays (flat_origin_ray_source, tracer.hpp:60-76) in 8 x 8-tile order, made on the device
ray = torch.arange(W * H, device=dev)
tile, within = ray // 64, ray % 64
x = (tile % (W // 8)) * 8 + within % 8
y = (tile // (W // 8)) * 8 + within // 8
fovI = math.tan(sc.fov / 2) / (W / 2)
ax = torch.from_numpy(axes).to(dev)
sx = (fovI * (x.float() - W / 2))[:, None]
sy = (fovI * (y.float() - H / 2))[:, None]
d = (ax[2][None] + ax[0][None] * sx) - ax[1][None] * sy
directions = (d / d.norm(dim=1, keepdim=True)).contiguous()
origins = torch.from_numpy(origin).to(dev)[None].repeat(W * H, 1).contiguous()
count = W * H

fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
fst = fmt._as_struct()
frame = torch.empty(fmt.pitch * H, dtype=torch.uint8, device=dev)
opts = _lib.NtRenderOpts()
opts.device = dev.index


def render():
    _lib.check(_lib.lib().nt_render_device(sc._handle, C.c_void_p(frame.data_ptr()), frame.numel(), C.byref(fst), C.byref(opts), C.c_void_p(st.cuda_stream)))


hits = torch.empty((count, 4), dtype=torch.int32, device=dev)
no, nd = torch.empty((count, N), device=dev), torch.empty((count, N), device=dev)
rays = _lib.NtRayBatch()
rays.count, rays.origins, rays.directions = count, origins.data_ptr(), directions.data_ptr()
plain, with_normals = _lib.NtRayResults(), _lib.NtRayResults()
plain.hits = with_normals.hits = hits.data_ptr()
with_normals.normal_origin, with_normals.normal_dir = no.data_ptr(), nd.data_ptr()


def query(res):
    _lib.check(_lib.lib().nt_intersect_rays_device(sc._handle, C.byref(rays), C.byref(res), C.byref(opts), C.c_void_p(st.cuda_stream)))


# ---- the render's head start, given to the query: composite_scene::aabb_distance drops the rays that never enter the scene's
# box before any walk and starts the others at their entry distance; KDNode.intersects has no such test.  The `boxed` leg is
# the query on the rays that enter the box only (still in tile order), with the entry distance as t_near.
lo, hi = (torch.from_numpy(np.asarray(g[k], np.float32)).to(dev)[None] for k in ("aabb_start", "aabb_end"))
t0s, t1s = (lo - origins) / directions, (hi - origins) / directions
entry = torch.minimum(t0s, t1s).amax(dim=1).clamp_min(0.0)
enters = torch.maximum(t0s, t1s).amin(dim=1) >= entry
b_origins, b_directions, b_t_near = origins[enters].contiguous(), directions[enters].contiguous(), entry[enters].contiguous()
boxed_rays = _lib.NtRayBatch()
boxed_rays.count, boxed_rays.origins, boxed_rays.directions, boxed_rays.t_near = int(enters.sum()), b_origins.data_ptr(), b_directions.data_ptr(), b_t_near.data_ptr()


def boxed():
    _lib.check(_lib.lib().nt_intersect_rays_device(sc._handle, C.byref(boxed_rays), C.byref(plain), C.byref(opts), C.c_void_p(st.cuda_stream)))


legs = {"render": render, "query": lambda: query(plain), "normals": lambda: query(with_normals), "boxed": boxed}
for fn in legs.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
query(plain)
torch.cuda.synchronize()
hit_rays = int((hits[:, 1] >= 0).sum())
t0 = time.perf_counter()
k = 0
while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
    for fn in legs.values():
        fn()
    k += 1
    if k % 8 == 0:
        torch.cuda.synchronize()
torch.cuda.synchronize()
REPS = 20
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

out = {"frame": args.frame, "rays": count, "rays_that_hit": hit_rays, "rays_that_enter_the_box": boxed_rays.count, "calls_a_round": REPS, "rounds": args.rounds,
       "device": torch.cuda.get_device_name(dev)}
for name, v in ms.items():
    rays_of_leg = boxed_rays.count if name == "boxed" else count
    out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4),
                 "Mrays_s": round(rays_of_leg / float(np.median(v)) / 1e3, 1)}
base = out["render"]["median_ms"]
for name, extra in (("query", 8 * N + 16), ("normals", 16 * N + 16)):
    traffic_ms = count * extra / (STREAM_TB_S * 1e12) * 1e3
    out[name]["expected_at_most_ms"] = round((base + traffic_ms) * MARGIN, 4)
    out[name]["within_expectation"] = out[name]["median_ms"] <= out[name]["expected_at_most_ms"]
print(json.dumps(out), flush=True)
