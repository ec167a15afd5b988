"""The "sure hit" bit of box_stretch_code2 (ntracer_amd/csrc/nt_box.hpp, NT_BOX_SETS_SURE), restated by
tools/box_sets_census.py's stretch_sure_hit -- without a GPU.  A stretch carries the bit when its sets are valid with C == T, no
slab can be left inside the window of tau its tests are made in, and |o_j| <= 4.5 on every axis of T; the tile kernel then
stores a near-tie row's pixels without the reference's square root and divisions, provided the smallest and the largest |d_i|
over T give the same bytes.

Cameras: the bench's rotation at frames 48 and 112 (|o_j| = 4.17 on the tie axes), 64 and 96 (|o_2| = 7.93: no stretch whose T
holds axis 2 may be flagged) and frame 48 again from 1.15 times the distance (|o_j| = 4.79 on the tie axes: between the limit and
the 5.33 at which the bound on the reference's rounding reaches 1 + FUZZ), and frames 52 and 108 (more flagged rows that must
fall back).  BoxScene(6) takes them from the bench's golden file,
the other dimensions of tests/test_box_tie_shortcut_gpu.py from the same rotation (tests/test_host_api.py's).

What the bit promises is checked against the oracle ray by ray on a seeded sample of flagged stretches: every ray a hit, at a
face of T.  The same sample counts the rows in which some ray's two candidate pixels differ -- the rows that must fall back."""
import functools
import math
import os
import sys

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
from ntracer_amd.wrapper import NTracer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_host_api as tha  # noqa: E402

F = np.float32
W, H = 1920, 1080
LIMIT = 4.5                       # NT_BOX_TIE_SURE_MAX_ORIGIN
BREAK_EVEN = 5.3                  # (4 + 3 * 5.33) u = 20 u
PAIR_NEAR, PAIR_FAR, STRESS = (48, 112), (64, 96), 48
MORE = (52, 108)                  # ... more flagged rows that must fall back
STRESS_SCALE = 1.15
SAMPLE, SEED = 1500, 11


@functools.lru_cache(maxsize=None)
def _rotation(n, scale):
    return tha.rotation_cameras(NTracer(n), -math.sqrt(n) * 4 * scale, max(PAIR_NEAR + PAIR_FAR + MORE) + 1)


@functools.lru_cache(maxsize=None)
def cameras(n):
    """(name, origin, axes): bench-48, bench-112, bench-64, bench-96, stress-48, bench-52, bench-108"""
    if n == 6:
        g = fx.load("box_n6_1920x1080")
        rot = [(np.asarray(g["origins"][k], F), np.ascontiguousarray(g["axes"][k], F)) for k in range(len(g["origins"]))]
    else:
        rot = _rotation(n, 1.0)
    cams = [("bench-%d" % k, ) + tuple(rot[k]) for k in PAIR_NEAR + PAIR_FAR]
    o, a = _rotation(n, STRESS_SCALE)[STRESS]
    return cams + [("stress-%d" % STRESS, o, a)] + [("bench-%d" % k, ) + tuple(rot[k]) for k in MORE]


def in_T(sets, j):
    return ((sets >> np.uint32(j)) & 1).astype(bool)


def origin_over_T(origin, sets):
    """max |o_j| over the axes of T, per stretch"""
    out = np.zeros(sets.shape, F)
    for j in range(len(origin)):
        out = np.where(in_T(sets, j), np.maximum(out, abs(F(origin[j]))), out)
    return out


def reference_dirs(v):
    """|d| of the reference's float d = v / |v|: the sum of squares in ascending order, one square root, n divisions"""
    sq = (v[:, 0] * v[:, 0]).astype(F)
    for j in range(1, v.shape[1]):
        sq = (sq + (v[:, j] * v[:, j]).astype(F)).astype(F)
    return np.abs((v / np.sqrt(sq).astype(F)[:, None]).astype(F))


def packed(shade, channels=fx.RGBX8):
    """the oracle's packed pixel of a hit of shade |d_i|"""
    return ob.pack_pixel((shade, F(shade * F(0.5)), F(shade * F(0.5))), channels)


def candidates_differ(origin, axes, w, h, y, col, sets, channels=fx.RGBX8):
    """some ray of the stretch has two faces of T whose pixels differ: the row cannot be stored from the set alone"""
    d = reference_dirs(census.rays_of(origin, axes, w, h, y, col))
    T = [j for j in range(d.shape[1]) if (int(sets) >> j) & 1]
    lo, hi = d[:, T].min(1), d[:, T].max(1)
    return any(a != b and packed(a, channels) != packed(b, channels) for a, b in zip(lo, hi))


def test_the_bit_on_the_bench_cameras():
    cams = {name: (o, a) for name, o, a in cameras(6)}
    for k in PAIR_NEAR:
        o, a = cams["bench-%d" % k]
        assert abs(np.abs(o[3:]).max() - 4.17) < 0.01
        code, sets, sure = census.stretch_sure_hit(o, a, W, H)
        assert int(((code == 14) & sure).sum()) >= 200, k
        assert (origin_over_T(o, sets)[sure] <= LIMIT).all()
    for k in PAIR_FAR:
        o, a = cams["bench-%d" % k]
        assert abs(abs(o[2]) - 7.93) < 0.01
        code, sets, sure = census.stretch_sure_hit(o, a, W, H)
        near_tie = (code == 14) & ((sets >> np.uint32(31)) != 0)
        with_axis_2 = near_tie & in_T(sets, 2)
        assert int(with_axis_2.sum()) >= 200 and not (with_axis_2 & sure).any(), k
        assert not (sure & (origin_over_T(o, sets) > LIMIT)).any()
        # (the tie sets without axis 2 are flagged as anywhere else)
        assert int((near_tie & sure).sum()) >= 200, k


def test_the_limit_on_the_origin_is_what_stops_the_stress_camera():
    name, o, a = cameras(6)[4]
    assert name.startswith("stress")
    assert LIMIT < np.abs(o[3:]).min() and np.abs(o[3:]).max() < BREAK_EVEN, o
    code, sets, sure = census.stretch_sure_hit(o, a, W, H)
    over = origin_over_T(o, sets) > LIMIT
    assert not (sure & over).any()
    _, _, wider = census.stretch_sure_hit(o, a, W, H, limit=F(BREAK_EVEN))
    assert int(((code == 14) & wider & over).sum()) >= 200
    assert not (sure & ~wider).any()


def test_flagged_and_unflagged_near_tie_rows_share_a_wave():
    """the 64 x 1 shape: slot s of wave w of a column strip is row w + stride * s"""
    stride = (H + 63) // 64
    shared = 0
    for name, o, a in cameras(6)[:2]:
        code, sets, sure = census.stretch_sure_hit(o, a, W, H)
        tie = code == 14
        for w in range(stride):
            rows = np.arange(w, H, stride)
            shared += int(((tie & sure)[rows].any(0) & (tie & ~sure)[rows].any(0)).sum())
    assert shared >= 10, shared


@functools.lru_cache(maxsize=None)
def flagged_sample():
    """(camera index, y, col, sets) of SAMPLE flagged near-tie stretches of the six bench cameras, seeded"""
    cams = cameras(6)
    rows = []
    for k in (0, 1, 2, 3, 5, 6):
        code, sets, sure = census.stretch_sure_hit(cams[k][1], cams[k][2], W, H)
        yy, cc = np.nonzero((code == 14) & sure)
        rows += [(k, int(y), int(c), int(sets[y, c])) for y, c in zip(yy, cc)]
    sel = np.random.default_rng(SEED).choice(len(rows), size=SAMPLE, replace=False)
    return [rows[i] for i in sel]


def test_every_ray_of_a_flagged_stretch_is_a_hit_at_a_face_of_T():
    cams = cameras(6)
    sample = flagged_sample()
    assert len(sample) >= 500
    osc = ob.OracleScene(6, cams[0][1], cams[0][2])
    rays = misses = outside = fall_back = 0
    for k, y, col, sets in sample:
        _, o, a = cams[k]
        osc.set_camera(o, a)
        xs = np.minimum(col * 64 + np.arange(64), W - 1)
        rgb = osc.colors_at(xs, np.full(64, y), W, H)
        # a hit is (s, s/2, s/2) with s = |d_i| > 0; the background (i, i, i) or (0, -i, -i)
        hit = (rgb[:, 0] > 0) & (rgb[:, 1] == (rgb[:, 0] * F(0.5)).astype(F)) & (rgb[:, 2] == rgb[:, 1])
        d = reference_dirs(census.rays_of(o, a, W, H, y, col))
        face_in_T = np.zeros(64, bool)
        for j in range(6):
            if (sets >> j) & 1:
                face_in_T |= rgb[:, 0] == d[:, j]
        rays += 64
        misses += int((~hit).sum())
        outside += int((hit & ~face_in_T).sum())
        fall_back += int(candidates_differ(o, a, W, H, y, col, sets))
    print({"rays": rays, "misses": misses, "hits outside T": outside, "rows whose candidates differ": fall_back})
    assert rays >= 32000
    assert misses == 0 and outside == 0
    # rows the kernel cannot store from the set alone are part of the sample (and not all of it)
    assert 50 <= fall_back <= len(sample) // 2, fall_back
