"""box_tile_kernel's edge rows (ntracer_amd/csrc/nt_box.hpp, NT_BOX_EDGE_ROWS) -- without a GPU.  A row sorted ray by ray (code
15) whose stretch has valid sets with |C| = 2 and T = C or |T| = 1 is classified on its two axes alone: box_classify_sets<2>
with a compile-time sets word, on dir[a], dir[b] of the axes a < b of C.  Restated here in numpy (classify_two) next to
tools/box_sets_census.py's restatement of the N-axis box_classify_sets (census.classify on T and C), and compared ray by ray.

Cameras: tests/test_box_tie_shortcut_host.py's -- the bench's rotation at frames 48, 112, 64, 96, 52 and 108 and frame 48 from
1.15 times the distance -- and frame 8 of the rotation, in N = 6 and 7 (the kernel has the path at N = 6, in launches large
enough for the kernel with the near-tie short cut; the classifiers are compared at both).  Asserted of their 630 x 200 frames before anything is compared (and before
tests/test_box_edge_rows_gpu.py renders anything): edge rows with T on the lower axis of C, on the upper axis and on both, each
with and without an unclear lane, and clear rows whose 2^-18 guard must fail.  (The kernel puts no cap on the sets words a wave
takes, so there is no wave with more than the cap to look for; the cameras' waves hold up to three.)"""
import functools
import os
import sys

import numpy as np
import pytest

import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_one_pass as top  # noqa: E402
import test_box_tie_shortcut_host as host  # noqa: E402
from ntracer_amd import distributed as ntd  # noqa: E402

F = np.float32
INF = F(np.inf)
W, H = tlg.W, tlg.H                     # 630 x 200
TALL, BAND = tlg.TALL, tlg.BAND
SETS_DIMS = (6, 7)                      # the dimensions that have box_classify_sets (NT_BOX_CLASSIFY_SETS_MIN_N .. _MAX_N)
EDGE_DIMS = (6, )                       # ... and of them those with a kernel for large launches, the one the edge rows are in (nt_inst_box.hip)
CONTROL_DIMS = (5, 8)
WORD_MASK = np.uint32(0x800fffff)       # what of a sets word the kernel compares: T, C and "valid"
LOWER, UPPER, BOTH = 1, 2, 3            # which of C's two axes are in T: bit 0 the lower, bit 1 the upper
SAMPLE, SEED = 3000, 23
EXTRA = 8


@functools.lru_cache(maxsize=None)
def cameras(n):
    """(name, origin, axes): tests/test_box_tie_shortcut_host.py's seven and frame 8 of the same rotation, whose 630 x 200 frame has
    an edge row of each kind with an unclear lane at N = 7 as well"""
    if n == 6:
        g = fx.load("box_n6_1920x1080")
        o, a = np.asarray(g["origins"][EXTRA], F), np.ascontiguousarray(g["axes"][EXTRA], F)
    else:
        o, a = host._rotation(n, 1.0)[EXTRA]
    return host.cameras(n) + [("bench-%d" % EXTRA, o, a)]


def edge_stretches(code, sets):
    """the stretch-rows the kernel's ballot picks: code 15, valid sets, T inside C, |C| = 2, T = C or |T| = 1"""
    T, Cs = sets & np.uint32(0x3ff), (sets >> np.uint32(10)) & np.uint32(0x3ff)
    nt, nc = census.popcount(T), census.popcount(Cs)
    return (code == 15) & ((sets >> np.uint32(31)) != 0) & ((T & ~Cs) == 0) & (nc == 2) & ((T == Cs) | (nt == 1))


def axes_of(sets):
    """(a, b, which): the axes a < b of C and which of them are in T"""
    s = int(sets)
    c = [j for j in range(10) if (s >> (10 + j)) & 1]
    assert len(c) == 2
    return c[0], c[1], ((s >> c[0]) & 1) | (((s >> c[1]) & 1) << 1)


def classify_two(m, o2, v2, v0, which):
    """box_classify_sets<2, WORD> on the arrays o2 = (o_a, o_b), v2 = (dir_a, dir_b) [L][2], WORD = valid | C = {0, 1} | T = which,
    m the margin of the whole origin: (verdict [L], x [L]) with x = v_K for a hit and dir[0] otherwise"""
    m1p = F(F(1.0) + m)
    L = len(v0)
    with np.errstate(all="ignore"):
        tn, tn2, vK = np.full(L, -INF, F), np.full(L, -INF, F), np.zeros(L, F)
        tnp, tfp = np.full(L, -INF, F), np.full(L, INF, F)
        for j in range(2):
            inv = census._rcp(v2[:, j])
            c0 = (-o2[j] * inv).astype(F)
            tfp = np.fmin(tfp, census._fma(np.abs(inv), m1p, c0))
            if (which >> j) & 1:
                nr = (c0 - np.abs(inv)).astype(F)
                tnp = np.fmax(tnp, census._fma(-np.abs(inv), m1p, c0))
                later = nr > tn
                tn2 = census._med3(tn, tn2, nr)
                vK = np.where(later, v2[:, j], vK)
                tn = np.fmax(tn, nr)
        miss = (tnp > tfp) | (tfp < 0)
        c = F(F(1.0) - m)
        total = np.zeros(L, F)
        for j in range(2):
            total = (total + np.fmax(np.abs(census._fma(v2[:, j], tn, o2[j])), c)).astype(F)
        inside = (total - F(F(2.0) * c)).astype(F) <= F(F(1.5) * m)
        sole = ((tn - tn2).astype(F) * np.abs(vK)).astype(F) > m
        front = (tn > F(1e-3)) & (tn < F(1e30))
        hit = ~miss & inside & sole & front
    verdict = np.where(hit, census.HIT, np.where(miss, census.MISS, census.UNCLEAR))
    return verdict, np.where(hit, vK, v0).astype(F)


def both_classifiers(origin, axes, w, h, y, col, sets):
    """one edge stretch-row: the two-axis verdicts and x, the N-axis verdicts and x, and the rays [64][n]"""
    o = np.asarray(origin, F)
    v = census.rays_of(origin, axes, w, h, y, col)
    a, b, which = axes_of(sets)
    two, x2 = classify_two(census._margin(o), o[[a, b]], v[:, [a, b]], v[:, 0], which)
    n = len(o)
    full, vK = census.classify(o, v, [j for j in range(n) if (int(sets) >> j) & 1], [a, b])
    return two, x2, full, np.where(full == census.HIT, vK, v[:, 0]).astype(F), v


def guard_must_fail(x, hit, v, maxval=255.0):
    """some lane's quotient (or its half, for a hit) lies within half the guard's width of a rounding boundary: the row's guard
    fails whatever the device's rounding (as tests/test_box_one_pass.py's guard_fails)"""
    vd = v.astype(np.float64)
    t = maxval * np.abs(x.astype(np.float64)) / np.sqrt((vd * vd).sum(1))
    near = lambda q: np.abs((q - np.floor(q)) - 0.5) < 0.5 * (q + 1.0) * 2.0 ** -18
    return bool((near(t) | (hit & near(0.5 * t))).any())


@functools.lru_cache(maxsize=None)
def frame_census(n, h, band):
    """the edge stretch-rows of the cameras' 630 x h frames (band: the rank's rows of them) by which axes are in T and by whether a
    lane is unclear; the clear ones whose guard must fail; the most sets words in one wave of a 64 x 1 launch"""
    rows = ntd.owned_rows(h, *BAND) if band else None
    ys = np.arange(h) if rows is None else rows
    out = {(which, unclear): 0 for which in (LOWER, UPPER, BOTH) for unclear in (False, True)}
    out.update({"guard": 0, "stored": 0, "words-a-wave": 0, "code-15": 0})
    stride = top.stride_of(len(ys))
    for _, o, a in cameras(n):
        code, sets = census.stretch_codes(o, a, W, h, rows=rows)
        out["code-15"] += int((code == 15).sum())
        if n not in SETS_DIMS:
            continue
        edge = edge_stretches(code, sets)
        for r, col in zip(*np.nonzero(edge)):
            two, x2, _, _, v = both_classifiers(o, a, W, h, int(ys[r]), int(col), sets[r, col])
            unclear = bool((two == census.UNCLEAR).any())
            out[(axes_of(sets[r, col])[2], unclear)] += 1
            if not unclear:
                fails = guard_must_fail(x2, two == census.HIT, v)
                out["guard"] += fails
                out["stored"] += not fails
        for col in np.nonzero(edge.any(0))[0]:
            for wv in range(stride):
                r = np.arange(wv, len(ys), stride)
                out["words-a-wave"] = max(out["words-a-wave"], len(set((sets[r, col][edge[r, col]] & WORD_MASK).tolist())))
    return out


def check_census(n):
    frames, bands = frame_census(n, H, False), frame_census(n, TALL, True)
    assert frames["code-15"] >= 1000 and bands["code-15"] >= 100, (n, frames, bands)
    if n in SETS_DIMS:
        for which in (LOWER, UPPER, BOTH):
            assert frames[(which, False)] >= 20 and frames[(which, True)] >= 1, (n, which, frames)
        assert frames["guard"] >= 5 and frames["stored"] >= 300, (n, frames)
        assert frames["words-a-wave"] >= 2, (n, frames)
        assert sum(bands[(which, False)] for which in (LOWER, UPPER, BOTH)) >= 20, (n, bands)


@pytest.mark.parametrize("n", SETS_DIMS + CONTROL_DIMS)
def test_cameras_hold_every_kind_of_edge_row(n):
    check_census(n)


def test_the_dimensions_are_the_header_s():
    import re
    src = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_box.hpp")).read()
    inst = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_inst_box.hip")).read()
    lo = int(re.search(r"#define NT_BOX_CLASSIFY_SETS_MIN_N (\d+)", src).group(1))
    hi = int(re.search(r"#define NT_BOX_CLASSIFY_SETS_MAX_N (\d+)", src).group(1))
    assert tuple(range(lo, hi + 1)) == SETS_DIMS
    # the switch is on, the path is in the kernel with TIE, and BoxScene(7) is built without that kernel
    assert re.search(r"#define NT_BOX_EDGE_ROWS 1\b", src) and "constexpr bool EDGE = TIE && " in src
    assert re.search(r"#if NT_INST_N == 7 && !defined\(NT_BOX_TIE_SHORTCUT\)\n(//.*\n)*#define NT_BOX_TIE_SHORTCUT 0", inst)
    assert EDGE_DIMS == tuple(n for n in SETS_DIMS if n != 7)


@functools.lru_cache(maxsize=None)
def edge_sample(n):
    """(camera index, w, h, y, col, sets) of SAMPLE edge stretch-rows of the cameras' 630 x 200 and 1920 x 1080 frames, seeded"""
    rows = []
    for k, (_, o, a) in enumerate(cameras(n)):
        for w, h in ((W, H), (host.W, host.H)):
            code, sets = census.stretch_codes(o, a, w, h)
            yy, cc = np.nonzero(edge_stretches(code, sets))
            rows += [(k, w, h, int(y), int(c), int(sets[y, c])) for y, c in zip(yy, cc)]
    sel = np.random.default_rng(SEED + n).choice(len(rows), size=min(SAMPLE, len(rows)), replace=False)
    return [rows[i] for i in sel]


@pytest.mark.parametrize("n", SETS_DIMS)
def test_two_axis_verdicts_equal_the_n_axis_ones_ray_by_ray(n):
    cams = cameras(n)
    sample = edge_sample(n)
    assert len(sample) >= 2000, len(sample)
    seen = {census.HIT: 0, census.MISS: 0, census.UNCLEAR: 0}
    kinds = {LOWER: 0, UPPER: 0, BOTH: 0}
    wrong = 0
    for k, w, h, y, col, sets in sample:
        _, o, a = cams[k]
        two, x2, full, xf, _ = both_classifiers(o, a, w, h, y, col, sets)
        # the same verdict, and the same component behind the pixel (bit for bit: a NaN never equals itself, and none may occur)
        wrong += int(((two != full) | (x2 != xf)).sum())
        for key in seen:
            seen[key] += int((two == key).sum())
        kinds[axes_of(sets)[2]] += 1
    print({"rows": len(sample), "rays": 64 * len(sample), "verdicts": seen, "kinds": kinds, "rays that differ": wrong})
    assert wrong == 0
    assert min(seen.values()) >= 100 and min(kinds.values()) >= 100, (seen, kinds)


@pytest.mark.parametrize("n", SETS_DIMS)
def test_valid_sets_have_T_inside_C(n):
    """the premise of picking T's axes among C's two"""
    for _, o, a in cameras(n):
        code, sets = census.stretch_codes(o, a, W, H)
        valid = (sets >> np.uint32(31)) != 0
        T, Cs = sets & np.uint32(0x3ff), (sets >> np.uint32(10)) & np.uint32(0x3ff)
        assert valid.any() and not (T[valid] & ~Cs[valid]).any() and (T[valid] != 0).all()
