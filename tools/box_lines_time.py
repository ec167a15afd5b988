#!/usr/bin/env python3
"""What BoxScene's face lines and hit buffers cost next to the plain render, and next to what a caller pays for the same picture
with the hit buffers alone.  Not a test.

BoxScene(6) and BoxScene(10) at 1920 x 1080 RGBX8, black lines at full strength, single frames and a 160-frame camera table (the
golden sequences of tests/golden, cycled to 160 cameras); the legs are timed against each other, alternately in one process,
each on a scene object of its own (same camera):

  plain        (a) the plain render
  lines        (b) the render with the setting on: box_lines, records in LDS
  hits         (c) nt_box_hits* alone into a tensor that is already there
  by_hand      (d) the same picture composed by a caller with (c): the plain fp32 x 3 render, face_hits, a torch stencil over the
                   records and a blend on the device, quantised to RGBX8
  lines_var    (e) (b) under NTRACER_FORCE_VAR=1: box_hits_var into scratch, box_lines_var behind it

The one condition: (b) below (d) in the same run by more than the spread of the two -- otherwise the fused kernel has no reason
to exist.  (b) / (a) and (c) / (a) are reported.  Before anything is timed the tool checks, on one frame in fp32 x 3, that (d)'s
picture is (b)'s bit for bit and that (e) gives (b)'s bytes.

The chip is settled the way tools/outline_time.py settles it (untimed calls for 200 ms, then timed calls between
synchronisations); every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs
under an alarm of --leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/box_lines_time.py [--rounds 7] [--reps 10] [--frames 160]    one JSON line a (scene, form), appended to
                                                                             profiles/box_lines_time.jsonl"""
import argparse
import ctypes as C
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
ap.add_argument("--frames", type=int, default=160, help="frames of the camera-table form")
ap.add_argument("--leg-timeout", type=int, default=60, help="seconds a leg's warm-up, settling calls or one timed round may take")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402
from ntracer_amd.render import CameraTable  # noqa: E402

W, H = args.width, args.height
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
COLOR, STRENGTH = (0.0, 0.0, 0.0), 1.0
SETTLE_MS = 200.0
LEGS = ("plain", "lines", "hits", "by_hand", "lines_var")

dev = torch.device("cuda", torch.cuda.current_device())
st = torch.cuda.current_stream()
fmt8 = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBX8])
fmt32 = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in RGBF32])
L = _lib.lib()


class limit:
    """the calls of one leg under an alarm of their own, up to the synchronisation that ends them"""
    def __enter__(self):
        signal.alarm(args.leg_timeout)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        signal.alarm(0)


def stencil(recs, frames):
    """the mask rule of include/ntracer_hip.h on records [frames * H * W][4] int32, in torch: bool [frames][H][W]"""
    r = recs.view(frames, H, W, 4)
    dist = r[..., 0].view(torch.float32)
    code = torch.where(r[..., 1] >= 0, 2 * r[..., 1] + r[..., 2], torch.full_like(r[..., 1], -1))
    hit = code >= 0
    mark = torch.zeros_like(hit)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
        yq, xq = slice(max(0, -dy) + dy, H - max(0, dy) + dy), slice(max(0, -dx) + dx, W - max(0, dx) + dx)
        cp, cq = code[:, ys, xs], code[:, yq, xq]
        mark[:, ys, xs] |= hit[:, ys, xs] & ((cq < 0) | ((cq != cp) & ~(dist[:, ys, xs] > dist[:, yq, xq])))
    return mark


def blended(frame32, mark, frames):
    """(P * (1 - strength)) + (color * strength) where the mask is set, on the big-endian fp32 x 3 frame: float32 [frames][H][W][3]"""
    P = frame32.view(torch.int32).view(frames, H, W, 3)
    P = ((P & 0xFF) << 24 | (P & 0xFF00) << 8 | (P >> 8) & 0xFF00 | (P >> 24) & 0xFF).view(torch.float32)      # byte swap
    col = torch.tensor(COLOR, dtype=torch.float32, device=dev) * STRENGTH
    return torch.where(mark[..., None], P * (1.0 - STRENGTH) + col, P)


def measure(n, fov, origins, axes, frames):
    single = frames == 1
    table = None if single else CameraTable(n, origins[:frames], axes[:frames])
    scenes = {}
    for name in LEGS:
        sc = tracern.BoxScene(n)
        sc.set_fov(fov)
        sc._set_camera_arrays(origins[0], axes[0])
        if name.startswith("lines"):
            sc.set_face_lines(COLOR, STRENGTH)
        scenes[name] = sc
    out8 = {name: torch.zeros(frames * fmt8.pitch * H, dtype=torch.uint8, device=dev) for name in ("plain", "lines", "lines_var")}
    hand32 = torch.zeros(frames * fmt32.pitch * H, dtype=torch.uint8, device=dev)
    recs = {name: torch.zeros((frames * W * H, 4), dtype=torch.int32, device=dev) for name in ("hits", "by_hand")}
    last = {}

    def render(sc, buf, fmt):
        fst = fmt._as_struct()
        if single:
            _lib.check(L.nt_render_device(sc._handle, C.c_void_p(buf.data_ptr()), fmt.pitch * H, C.byref(fst), None, C.c_void_p(st.cuda_stream)))
        else:
            _lib.check(L.nt_render_table_device(sc._handle, C.c_void_p(buf.data_ptr()), fmt.pitch * H, table._h, 0, frames, C.byref(fst), None,
                                                C.c_void_p(st.cuda_stream)))

    def hits(sc, buf):
        sc.face_hits(W, H, out=buf) if single else sc.face_hits(W, H, out=buf, table=table, first=0, count=frames)

    def by_hand():
        sc = scenes["by_hand"]
        render(sc, hand32, fmt32)
        hits(sc, recs["by_hand"])
        rgb = blended(hand32, stencil(recs["by_hand"], frames), frames)
        last["by_hand32"] = rgb
        q = (rgb * 255.0 + 0.5).to(torch.uint8)
        last["by_hand"] = torch.cat([q, torch.zeros_like(q[..., :1])], dim=-1)

    def lines_var():
        os.environ["NTRACER_FORCE_VAR"] = "1"           # (the switches are read at every call)
        try:
            render(scenes["lines_var"], out8["lines_var"], fmt8)
        finally:
            del os.environ["NTRACER_FORCE_VAR"]

    legs = {"plain": lambda: render(scenes["plain"], out8["plain"], fmt8), "lines": lambda: render(scenes["lines"], out8["lines"], fmt8),
            "hits": lambda: hits(scenes["hits"], recs["hits"]), "by_hand": by_hand, "lines_var": lines_var}
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": "BoxScene(%d)" % n, "n": n, "frames": frames, "width": W, "height": H, "format": "RGBX8", "strength": STRENGTH,
           "calls_a_round": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    # the checks: one frame of (b) in fp32 x 3 against (d)'s picture, (e) against (b)
    with limit():
        check = torch.zeros(fmt32.pitch * H, dtype=torch.uint8, device=dev)
        fst = fmt32._as_struct()
        _lib.check(L.nt_render_device(scenes["lines"]._handle, C.c_void_p(check.data_ptr()), fmt32.pitch * H, C.byref(fst), None,
                                      C.c_void_p(st.cuda_stream)))
        mine = blended(check, torch.zeros((1, H, W), dtype=torch.bool, device=dev), 1)           # (the render, byte-swapped)
        out["by_hand_is_the_render_bit_for_bit"] = bool(torch.equal(mine[0].view(torch.int32), last["by_hand32"][0].view(torch.int32)))
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(out8["lines"], out8["lines_var"]))
        changed = (out8["plain"].view(-1, 4) != out8["lines"].view(-1, 4)).any(dim=1)
        out["share_of_pixels_the_setting_changes"] = round(float(changed.float().mean()), 6)
        out["share_of_pixels_hit"] = round(float((recs["hits"][:, 1] >= 0).float().mean()), 6)
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
    out["lines_over_plain"] = round(out["lines"]["median_ms"] / out["plain"]["median_ms"], 3)
    out["hits_over_plain"] = round(out["hits"]["median_ms"] / out["plain"]["median_ms"], 3)
    out["lines_var_over_lines"] = round(out["lines_var"]["median_ms"] / out["lines"]["median_ms"], 3)
    out["lines_over_by_hand"] = round(out["lines"]["median_ms"] / out["by_hand"]["median_ms"], 4)
    out["lines_beat_by_hand_by_more_than_the_spread"] = bool(out["lines"]["max_ms"] < out["by_hand"]["min_ms"])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.join(HERE, "profiles"), exist_ok=True)
    with open(os.path.join(HERE, "profiles", "box_lines_time.jsonl"), "a") as f:
        f.write(line + "\n")
    del table


def cameras(name, count):
    g = np.load(os.path.join(HERE, "tests", "golden", name + ".npz"))
    o, a = np.asarray(g["origins"], np.float32), np.asarray(g["axes"], np.float32)
    idx = np.arange(count) % len(o)
    return float(g["fov"]), np.ascontiguousarray(o[idx]), np.ascontiguousarray(a[idx])


for n, name in ((6, "box_n6_1920x1080"), (10, "box_n10_4096x4096")):
    fov, o, a = cameras(name, max(args.frames, 1))
    measure(n, fov, o, a, 1)
    if args.frames > 1:
        measure(n, fov, o, a, args.frames)
