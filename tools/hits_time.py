#!/usr/bin/env python3
"""What a primary-hit pass costs next to the render of the same frames.  Not a test.

The golden 120-cell at 1920 x 1080, eight cameras of its golden sequence a call from a camera table.  The legs, alternately
in one process:

  render   nt_render_table_device into RGBX8: packet_numerators + composite_packet<4, 32, false, false>, 4 bytes a pixel
  hits     nt_primary_hits_table_device: the same walk, nothing shaded, one 16-byte record a pixel
  normals  ... with normal_origin / normal_dir: hits_normals<4, false> behind it, 32 more bytes a pixel that hit
  query    nt_intersect_rays_device on the primary rays of the table's FIRST frame alone, in 8 x 8-tile order
           (tools/query_time.py): the per-lane walk the callers had before; its time is for one frame

The chip is settled the way tools/ss_time.py settles it (untimed calls for 200 ms, then timed calls between synchronisations);
every leg reports the median of --rounds rounds and their spread, per call and per frame.  What `hits` is held against is
`render`, measured here, not any figure of its own: the render's time plus the 12 more bytes a pixel at the rate the chip
streams (5.7 TB/s) plus the larger of the two legs' spreads (max - min).

With --parent the library named by NTRACER_HIP_LIB is a build of the parent commit, which has no hit pass: `render` and
`query` alone (the A/B of the two builds alternates processes of the two kinds, as tools/lib_ab.sh does).

  python3 tools/hits_time.py [--rounds 9] [--parent]          one JSON line"""
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
ap.add_argument("--parent", action="store_true", help="the library is a build of the parent commit: no hit pass")
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, render, tracern  # noqa: E402

if args.parent:
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if not s[0].startswith("nt_primary_hits")]

W, H, N, FRAMES = 1920, 1080, 4, 8
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
SETTLE_MS = 200.0
STREAM_TB_S = 5.7

g = np.load(os.path.join(HERE, "tests", "golden", "cell120_n4.npz"))
sc = tracern.CompositeScene.from_flat(N, g)
cams = [20 * k for k in range(FRAMES)]                     # spread over the 160 cameras of the golden sequence
origins_h = np.ascontiguousarray(g["origins"][cams], np.float32)
axes_h = np.ascontiguousarray(g["axes"][cams], np.float32)
sc._set_camera_arrays(origins_h[0], axes_h[0])
table = render.CameraTable(N, origins_h, axes_h)
dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
L = _lib.lib()
opts = _lib.NtRenderOpts()
opts.device = dev.index

fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
fst = fmt._as_struct()
frame_bytes = fmt.pitch * H
image = torch.empty(FRAMES * frame_bytes, dtype=torch.uint8, device=dev)


def render_leg():
    _lib.check(L.nt_render_table_device(sc._handle, C.c_void_p(image.data_ptr()), frame_bytes, table._h, 0, FRAMES, C.byref(fst), C.byref(opts),
                                        C.c_void_p(st.cuda_stream)))


count = W * H
hits = torch.empty((FRAMES * count, 4), dtype=torch.int32, device=dev)
legs = {"render": render_leg}
if not args.parent:
    no, nd = torch.empty((FRAMES * count, N), device=dev), torch.empty((FRAMES * count, N), device=dev)
    plain, with_normals = _lib.NtHitBuffers(), _lib.NtHitBuffers()
    plain.hits = with_normals.hits = hits.data_ptr()
    with_normals.normal_origin, with_normals.normal_dir = no.data_ptr(), nd.data_ptr()

    def hits_leg(res):
        _lib.check(L.nt_primary_hits_table_device(sc._handle, W, H, C.byref(res), count, table._h, 0, FRAMES, C.byref(opts), C.c_void_p(st.cuda_stream)))
    legs["hits"] = lambda: hits_leg(plain)
    legs["normals"] = lambda: hits_leg(with_normals)

# ---- the first frame's primary rays (flat_origin_ray_source, tracer.hpp:60-76) in 8 x 8-tile order, made on the device
ray = torch.arange(count, device=dev)
tile, within = ray // 64, ray % 64
x = (tile % (W // 8)) * 8 + within % 8
y = (tile // (W // 8)) * 8 + within // 8
fovI = math.tan(sc.fov / 2) / (W / 2)
ax = torch.from_numpy(axes_h[0]).to(dev)
sx = (fovI * (x.float() - W / 2))[:, None]
sy = (fovI * (y.float() - H / 2))[:, None]
d = (ax[2][None] + ax[0][None] * sx) - ax[1][None] * sy
directions = (d / d.norm(dim=1, keepdim=True)).contiguous()
origins = torch.from_numpy(origins_h[0]).to(dev)[None].repeat(count, 1).contiguous()
qhits = torch.empty((count, 4), dtype=torch.int32, device=dev)
rays = _lib.NtRayBatch()
rays.count, rays.origins, rays.directions = count, origins.data_ptr(), directions.data_ptr()
qres = _lib.NtRayResults()
qres.hits = qhits.data_ptr()


def query_leg():
    _lib.check(L.nt_intersect_rays_device(sc._handle, C.byref(rays), C.byref(qres), C.byref(opts), C.c_void_p(st.cuda_stream)))


legs["query"] = query_leg
frames_of = {"render": FRAMES, "hits": FRAMES, "normals": FRAMES, "query": 1}

for fn in legs.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
pixels_that_hit = int((hits[:, 1] >= 0).sum()) if not args.parent else None
t0 = time.perf_counter()
k = 0
while (time.perf_counter() - t0) * 1e3 < SETTLE_MS:
    for fn in legs.values():
        fn()
    k += 1
    if k % 4 == 0:
        torch.cuda.synchronize()
torch.cuda.synchronize()
REPS = 10
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

out = {"build": "parent" if args.parent else "this tree", "frames_a_call": FRAMES, "cameras": cams, "pixels_a_frame": count, "pixels_that_hit": pixels_that_hit,
       "calls_a_round": REPS, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
for name, v in ms.items():
    f = frames_of[name]
    out[name] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4),
                 "median_ms_a_frame": round(float(np.median(v)) / f, 4)}
if "hits" in out:
    spread = max(out[k]["max_ms"] - out[k]["min_ms"] for k in ("render", "hits"))
    traffic_ms = FRAMES * count * 12 / (STREAM_TB_S * 1e12) * 1e3
    out["hits"]["expected_at_most_ms"] = round(out["render"]["median_ms"] + traffic_ms + spread, 4)
    out["hits"]["within_expectation"] = out["hits"]["median_ms"] <= out["hits"]["expected_at_most_ms"]
    out["query_a_frame_over_hits_a_frame"] = round(out["query"]["median_ms_a_frame"] / out["hits"]["median_ms_a_frame"], 2)
print(json.dumps(out), flush=True)
