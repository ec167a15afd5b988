#!/usr/bin/env python3
"""What BoxScene's face shading costs next to the plain render, the face-line render and the hit buffers, and next to what a caller
pays for the same picture without it.  Not a test.

BoxScene(6) and BoxScene(10) at 1920 x 1080 RGBX8, single frames and a 160-frame camera table (the golden sequences of
tests/golden, cycled to 160 cameras).  The setting: face_palette(n), fog from 2 to 8 towards (0.5, 0.625, 0.75) at strength 0.875
on the faces only, no tint -- a tint needs the visible point, which a caller would have to rebuild from the camera; the fused
kernel has it in registers --; lines black at full strength.  The legs are timed against each other, alternately in one process,
each on a scene object of its own (same camera):

  plain          (a) the plain render
  lines          (b) the face-line render
  shaded         (c) the shaded render without lines: box_shaded<N, false>
  shaded_lines   (d) the shaded render with lines: box_shaded<N, true>
  hits           (e) nt_box_hits* alone into a tensor that is already there
  by_hand        (f) (c)'s picture composed by a caller: the plain fp32 x 3 render, face_hits and a torch expression on the device,
                     quantised to RGBX8
  by_hand_lines  (g) (d)'s picture likewise, with a torch stencil over the records
  shaded_var     (h) (d) under NTRACER_FORCE_VAR=1: box_hits_var into scratch, box_shaded_var behind it

The conditions: (c) below (f) and (d) below (g) in the same run by more than the spread of the two.  Before anything is timed the
tool checks, on one frame in fp32 x 3, whether (f)'s and (g)'s pictures are (c)'s and (d)'s bit for bit, and that (h) gives (d)'s
bytes.

The chip is settled the way tools/box_lines_time.py settles it (untimed calls for 200 ms, then timed calls between
synchronisations); every leg reports the median of --rounds rounds of --reps calls and their spread.  Every call of a leg runs
under an alarm of --leg-timeout seconds of its own, whose default action ends the process: a leg that hangs is not waited for.

  python3 tools/box_shading_time.py [--rounds 7] [--reps 10] [--frames 160] [--out FILE]    one JSON line a (scene, form), appended
                                                                        to FILE (profiles/box_shading_time.jsonl)"""
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
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "box_shading_time.jsonl"))
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402
import ntracer_amd  # noqa: E402
from ntracer_amd import _lib, tracern  # noqa: E402
from ntracer_amd.render import CameraTable  # noqa: E402

W, H = args.width, args.height
RGBX8 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1), (8, 0, 0, 0)]
RGBF32 = [(32, 1, 0, 0, 0, True), (32, 0, 1, 0, 0, True), (32, 0, 0, 1, 0, True)]
LINE_COLOR, LINE_STRENGTH = (0.0, 0.0, 0.0), 1.0
NEAR, FAR, FOG_COLOR, FOG_STRENGTH = 2.0, 8.0, (0.5, 0.625, 0.75), 0.875
SETTLE_MS = 200.0
LEGS = ("plain", "lines", "shaded", "shaded_lines", "hits", "by_hand", "by_hand_lines", "shaded_var")

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


def swapped(frame32, frames):
    """the big-endian fp32 x 3 frame as float32 [frames][H][W][3]"""
    P = frame32.view(torch.int32).view(frames, H, W, 3)
    return ((P & 0xFF) << 24 | (P & 0xFF00) << 8 | (P >> 8) & 0xFF00 | (P >> 24) & 0xFF).view(torch.float32)


def shaded_by_hand(frame32, recs, table, frames, lines):
    """the rule of include/ntracer_hip.h without a tint, from the plain frame (whose red channel is the shade of a hit pixel), the
    records and the table [2 n][3]: float32 [frames][H][W][3]"""
    P = swapped(frame32, frames)
    r = recs.view(frames, H, W, 4)
    hit = r[..., 1] >= 0
    code = torch.where(hit, 2 * r[..., 1] + r[..., 2], torch.zeros_like(r[..., 1]))
    B = torch.where(hit[..., None], P[..., :1] * table[code.long()], P)
    Q = B.clamp(0.0, 1.0)
    f = ((r[..., 0].view(torch.float32) - NEAR) * (1.0 / (FAR - NEAR))).clamp(0.0, 1.0)
    w = (f * FOG_STRENGTH)[..., None]
    fog = torch.tensor(FOG_COLOR, dtype=torch.float32, device=dev)
    Q = torch.where(hit[..., None], Q * (1.0 - w) + fog * w, Q)
    if lines:
        col = torch.tensor(LINE_COLOR, dtype=torch.float32, device=dev) * LINE_STRENGTH
        Q = torch.where(stencil(recs, frames)[..., None], Q * (1.0 - LINE_STRENGTH) + col, Q)
    return Q


def measure(n, fov, origins, axes, frames):
    single = frames == 1
    table = None if single else CameraTable(n, origins[:frames], axes[:frames])
    palette = ntracer_amd.face_palette(n)
    palette_dev = torch.tensor(palette.reshape(2 * n, 3), device=dev)
    scenes = {}
    for name in LEGS:
        sc = tracern.BoxScene(n)
        sc.set_fov(fov)
        sc._set_camera_arrays(origins[0], axes[0])
        if name in ("lines", "shaded_lines", "shaded_var"):
            sc.set_face_lines(LINE_COLOR, LINE_STRENGTH)
        if name.startswith("shaded"):
            sc.set_face_shading(palette, near=NEAR, far=FAR, color=FOG_COLOR, strength=FOG_STRENGTH)
        scenes[name] = sc
    out8 = {name: torch.zeros(frames * fmt8.pitch * H, dtype=torch.uint8, device=dev) for name in ("plain", "lines", "shaded", "shaded_lines", "shaded_var")}
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

    def by_hand(lines):
        def run():
            sc = scenes["by_hand"]
            render(sc, hand32, fmt32)
            hits(sc, recs["by_hand"])
            rgb = shaded_by_hand(hand32, recs["by_hand"], palette_dev, frames, lines)
            last["by_hand_lines32" if lines else "by_hand32"] = rgb[0]
            q = (rgb * 255.0 + 0.5).to(torch.uint8)
            last["q"] = torch.cat([q, torch.zeros_like(q[..., :1])], dim=-1)
        return run

    def shaded_var():
        os.environ["NTRACER_FORCE_VAR"] = "1"           # (the switches are read at every call)
        try:
            render(scenes["shaded_var"], out8["shaded_var"], fmt8)
        finally:
            del os.environ["NTRACER_FORCE_VAR"]

    legs = {name: (lambda name=name: render(scenes[name], out8[name], fmt8)) for name in ("plain", "lines", "shaded", "shaded_lines")}
    legs.update({"hits": lambda: hits(scenes["hits"], recs["hits"]), "by_hand": by_hand(False), "by_hand_lines": by_hand(True), "shaded_var": shaded_var})
    for fn in legs.values():
        with limit():
            for _ in range(2):
                fn()
    out = {"scene": "BoxScene(%d)" % n, "n": n, "frames": frames, "width": W, "height": H, "format": "RGBX8", "calls_a_round": args.reps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(dev)}
    # the checks: one frame of (c) and (d) in fp32 x 3 against the caller's pictures, (h) against (d)
    with limit():
        check = torch.zeros(fmt32.pitch * H, dtype=torch.uint8, device=dev)
        fst = fmt32._as_struct()
        for name, key in (("shaded", "by_hand32"), ("shaded_lines", "by_hand_lines32")):
            _lib.check(L.nt_render_device(scenes[name]._handle, C.c_void_p(check.data_ptr()), fmt32.pitch * H, C.byref(fst), None,
                                          C.c_void_p(st.cuda_stream)))
            mine = swapped(check, 1)[0]
            out[key[:-2] + "_is_the_render_bit_for_bit"] = bool(torch.equal(mine.view(torch.int32), last[key].view(torch.int32)))
            out[key[:-2] + "_greatest_difference"] = float((mine - last[key]).abs().max())
        out["the_two_routes_give_equal_bytes"] = bool(torch.equal(out8["shaded_lines"], out8["shaded_var"]))
        changed = (out8["plain"].view(-1, 4) != out8["shaded"].view(-1, 4)).any(dim=1)
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
    med = lambda name: out[name]["median_ms"]
    out["shaded_over_plain"] = round(med("shaded") / med("plain"), 3)
    out["shaded_over_hits"] = round(med("shaded") / med("hits"), 3)
    out["shaded_lines_over_lines"] = round(med("shaded_lines") / med("lines"), 3)
    out["shaded_var_over_shaded_lines"] = round(med("shaded_var") / med("shaded_lines"), 3)
    out["by_hand_over_shaded"] = round(med("by_hand") / med("shaded"), 2)
    out["by_hand_lines_over_shaded_lines"] = round(med("by_hand_lines") / med("shaded_lines"), 2)
    out["shaded_beats_by_hand_by_more_than_the_spread"] = bool(out["shaded"]["max_ms"] < out["by_hand"]["min_ms"])
    out["shaded_lines_beat_by_hand_by_more_than_the_spread"] = bool(out["shaded_lines"]["max_ms"] < out["by_hand_lines"]["min_ms"])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
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
