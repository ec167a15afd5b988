"""The lean rows' guard of box_tile_kernel (ntracer_amd/csrc/nt_box.hpp: guard_clear<N>, nt_lean_budget_ulps, nt_lean_guard_log2)
-- without a GPU.  A culled or one-face row is stored from lean_quotient's t = |d| rsq(bb + m2bu sy + uu sy^2) when every lane's t
(and t/2 of a hit) keeps G (1 + t) clear of every k + 1/2; G = 2^-19 at N = 3..6 and 2^-18 beyond, from the budget
(11 N / 6 + 10) 2^-24 (1 + t) on the distance between t and the reference's quotient.

Restated here in fp32 numpy, one operation at a time (an fma through float64, as tools/box_sets_census.py has it): the
kernel's quadratic and quotient, with v_rsq_f32 as the rounded 1 / sqrt and as its neighbour on either side, and the reference's
fl(|d| / sqrtf(sum of squares, left to right)) with the exact product by maxval that `quantize` forms.  Over every pixel of every
culled and one-face stretch of the cameras' 630 x 200 frames, at maxval 255 and 1023:
  (a) the two quotients lie closer than the budget;
  (b) a lane whose guard passes rounds to the reference's integer, t and t/2;
  (c) at N = 3 and 6 there are rows with a lane between the old width and the new one and none inside the new one -- the rows
      whose path changes; at N = 8 the width is the old one and there is no such row to find;
  (d) there are rows with a lane inside the new width -- rows that still go ray by ray.

Cameras: frames 0, 48 and 112 of the bench's rotation (BoxScene(6): from its golden file) and tests/test_box_lean_groups.py's
stress, far and edge-on cameras (fixtures.stress_cameras' skewed-`up` and up-less orientations among them: the waves that never
take the quadratic)."""
import functools
import os
import re
import sys

import numpy as np
import pytest

import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_tie_shortcut_host as tie_host  # noqa: E402

F = np.float32
W, H = tlg.W, tlg.H                     # 630 x 200
COLS = tlg.COLS
DIMS = (3, 6, 8)
BENCH = (0, 48, 112)
MAXVALS = (255, 1023)                   # RGBX8 and 10-10-10-2
OLD_LOG2 = 18
U = 2.0 ** -24


def budget_ulps(n):
    """nt_lean_budget_ulps (nt_box.hpp; test_the_header_says_the_same holds the two together)"""
    return 11.0 * n / 6.0 + 10.0


def guard_log2(n):
    """nt_lean_guard_log2: the smallest power of two that leaves 1.5 times the budget, between 2^-20 and 2^-18"""
    for k in (20, 19):
        if 2.0 ** (24 - k) >= 1.5 * budget_ulps(n):
            return k
    return 18


def test_the_header_says_the_same():
    src = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_box.hpp")).read()
    assert "constexpr double nt_lean_budget_ulps(int n) { return 11.0 * n / 6.0 + 10.0; }" in src
    assert re.search(r"for \(int k = 20; k > 18; --k\)\n\s*if \(\(double\)\(1 << \(24 - k\)\) >= 1\.5 \* nt_lean_budget_ulps\(n\)\) return k;\n\s*return 18;", src)
    assert src.count("guard_clear<N>(") == 5 and "guard_clear(t" not in src
    assert [guard_log2(n) for n in range(3, 25)] == [19] * 4 + [18] * 18
    # the budget fits the width at every dimension the kernels are built for, 1.5 times below the cap
    for n in range(3, 25):
        assert 2.0 ** (24 - guard_log2(n)) >= (1.5 if guard_log2(n) > 18 else 1.0) * budget_ulps(n)


@functools.lru_cache(maxsize=None)
def cameras(n):
    """(name, origin, axes)"""
    if n == 6:
        g = fx.load("box_n6_1920x1080")
        rot = [(np.asarray(g["origins"][k], F), np.ascontiguousarray(g["axes"][k], F)) for k in BENCH]
    else:
        rot = [tie_host._rotation(n, 1.0)[k] for k in BENCH]
    cams = [("bench-%d" % k, ) + tuple(c) for k, c in zip(BENCH, rot)]
    return cams + [c for c in tlg.cameras(n) if not c[0].startswith("bench-")]


GPU_CAMERAS = ("bench-0", "bench-48", "bench-112", "far-0", "far-1", "edge-on-0", "edge-on-1", "skew-up-1.7", "no-up", "diagonal-0")


def gpu_cameras(n):
    """the ten of them that tests/test_box_lean_guard_gpu.py renders"""
    cams = [c for c in cameras(n) if c[0] in GPU_CAMERAS]
    assert len(cams) == len(GPU_CAMERAS)
    return cams


def guard_clear(t, log2):
    """guard_clear<N>: |fract(t) - 1/2| > fma(t, G, G), in fp32"""
    g = F(2.0 ** -log2)
    with np.errstate(invalid="ignore"):
        return np.abs(((t - np.floor(t)).astype(F) - F(0.5)).astype(F)) > census._fma(t, g, g)


class Frame:
    """one camera's 630 x h frame as the tile kernel and the reference see it"""

    def __init__(self, origin, axes, h=H, rows=None):
        right, up, fwd = (np.asarray(axes, F)[k] for k in range(3))
        self.n = n = len(fwd)
        half_w, half_h, fovI = census.screen(W, h)
        ys = np.arange(h) if rows is None else np.asarray(rows)
        x = np.minimum(np.arange(COLS * 64), W - 1)
        sx = (fovI * (x.astype(F) - half_w)).astype(F)
        self.sy = sy = (fovI * (ys.astype(F) - half_h)).astype(F)
        self.base = base = (fwd[None, :] + (right[None, :] * sx[:, None]).astype(F)).astype(F)           # [x][n]
        self.up = up
        bb, bu, uu = np.zeros(len(x), F), np.zeros(len(x), F), np.zeros(len(x), F)
        for j in range(n):
            bb = census._fma(base[:, j], base[:, j], bb)
            bu = census._fma(base[:, j], up[j], bu)
            uu = census._fma(up[j], up[j], uu)
        self.bb, self.bu, self.uu = bb, bu, uu
        with np.errstate(all="ignore"):
            lane_ok = (bu * bu).astype(F) <= ((bb * uu).astype(F) * F(0.0625)).astype(F)
        self.fastsq = lane_ok.reshape(COLS, 64).all(1)                                                      # per column strip
        self.code, _ = census.stretch_codes(origin, axes, W, h, rows=rows)
        # the reference: dir, its squares summed left to right, sqrtf
        with np.errstate(all="ignore"):
            self.dir = (base[None, :, :] - (up[None, None, :] * sy[:, None, None]).astype(F)).astype(F)    # [y][x][n]
            sq = (self.dir[:, :, 0] * self.dir[:, :, 0]).astype(F)
            for j in range(1, n):
                sq = (sq + (self.dir[:, :, j] * self.dir[:, :, j]).astype(F)).astype(F)
            self.len = np.sqrt(sq).astype(F)

    def quadratic(self, maxval):
        """the kernel's |dir|^2 / maxval^2: the coefficients scaled once a wave, two fma a row"""
        inv = F(F(1.0) / F(F(maxval) * F(maxval)))
        m2bu = ((F(-2.0) * self.bu).astype(F) * inv).astype(F)
        bbs, uus = (self.bb * inv).astype(F), (self.uu * inv).astype(F)
        sy = self.sy[:, None]
        return census._fma(sy, census._fma(sy, uus[None, :], m2bu[None, :]), bbs[None, :])                  # [y][x]

    def lean(self, K, maxval):
        """lean_quotient of dir[K]: three arrays [y][x], with rsq one ulp low, rounded, one ulp high"""
        with np.errstate(all="ignore"):
            r0 = (1.0 / np.sqrt(self.quadratic(maxval).astype(np.float64))).astype(F)
            d = np.abs(self.dir[:, :, K])
            return [(d * r).astype(F) for r in (np.nextafter(r0, F(0.0)), r0, np.nextafter(r0, F(np.inf)))]

    def reference(self, K, maxval):
        """the reference's shade |dir[K] / len| and its half, times maxval (exact in float64), and the integers they round to"""
        with np.errstate(all="ignore"):
            shade = np.minimum(np.abs((self.dir[:, :, K] / self.len).astype(F)), F(1.0))
        half = (shade * F(0.5)).astype(F)
        v, vh = shade.astype(np.float64) * maxval, half.astype(np.float64) * maxval
        return v, vh, np.floor(v + 0.5), np.floor(vh + 0.5)

    def stretches(self, K):
        """[y][x]: the pixels of the stretches the lean loops take with d = dir[K] -- culled ones for K = 0 and those of face K"""
        pick = (self.code == K + 1) | ((self.code == 0) if K == 0 else False)
        return np.repeat(pick & self.fastsq[None, :], 64, axis=1), np.repeat(self.code != 0, 64, axis=1)


@functools.lru_cache(maxsize=None)
def census_of(n, gpu=False):
    """over the cameras' (gpu: the GPU test's cameras') culled and one-face stretch-rows, both maxvals: the largest distance between the quotients in units of
    2^-24 (1 + t); lanes that pass the guard and round to another integer than the reference; the rows whose path changes; the
    rows that still fail"""
    new = guard_log2(n)
    out = {"pixels": 0, "rows": 0, "worst": 0.0, "wrong": 0, "spared": 0, "failing": 0, "failing-old": 0}
    for _, o, a in (gpu_cameras(n) if gpu else cameras(n)):
        fr = Frame(o, a)
        for maxval in MAXVALS:
            for K in sorted(set(np.maximum(fr.code[fr.code <= 13].astype(int) - 1, 0).tolist())):
                where, hit = fr.stretches(K)
                if not where.any():
                    continue
                hit = hit & where
                v, vh, rv, rvh = fr.reference(K, maxval)
                ts = fr.lean(K, maxval)
                for t in ts:
                    th = (t * F(0.5)).astype(F)
                    dist = np.abs(t.astype(np.float64) - v) / (1.0 + v)
                    disth = np.abs(th.astype(np.float64) - vh) / (1.0 + vh)
                    out["worst"] = max(out["worst"], float(dist[where].max()) / U, float(disth[hit].max()) / U if hit.any() else 0.0)
                    # (b) a clear lane rounds as the reference does (maxval clamps both)
                    q, qh = np.minimum(np.floor(t + F(0.5)), maxval), np.minimum(np.floor(th + F(0.5)), maxval)
                    clear, clearh = guard_clear(t, new), guard_clear(th, new)
                    out["wrong"] += int((where & clear & (q != rv)).sum()) + int((hit & clearh & (qh != rvh)).sum())
                # (c), (d): rows, on the rounded rsq
                t = ts[1]
                th = (t * F(0.5)).astype(F)
                fails = lambda log2: ((where & ~guard_clear(t, log2)) | (hit & ~guard_clear(th, log2))).reshape(len(fr.sy), COLS, 64).any(2)
                f_new, f_old = fails(new), fails(OLD_LOG2)
                out["spared"] += int((f_old & ~f_new).sum())
                out["failing"] += int(f_new.sum())
                out["failing-old"] += int(f_old.sum())
                out["rows"] += int(where.reshape(len(fr.sy), COLS, 64).any(2).sum())
                out["pixels"] += int(where.sum())
    return out


def check_census(n, gpu=False):
    """what tests/test_box_lean_guard_gpu.py relies on: its frames hold the rows whose path changes, and rows that still fail"""
    c = census_of(n, gpu)
    assert c["rows"] >= 5000 and c["failing"] >= 20, (n, c)
    if guard_log2(n) > OLD_LOG2:
        assert c["spared"] >= 20, (n, c)
    else:
        assert c["spared"] == 0 and c["failing"] == c["failing-old"], (n, c)


@pytest.mark.parametrize("n", DIMS)
def test_quotients_lie_within_the_budget_and_clear_lanes_round_alike(n):
    c = census_of(n)
    print({"n": n, "guard": "2^-%d" % guard_log2(n), "budget": budget_ulps(n), **c})
    assert c["pixels"] >= 500000
    assert c["worst"] < budget_ulps(n), (n, c)                # (a)
    assert c["wrong"] == 0, (n, c)                            # (b)


@pytest.mark.parametrize("n", DIMS + (10, ))
def test_cameras_hold_the_rows_whose_path_changes_and_rows_that_still_fail(n):
    check_census(n)                                           # (c), (d)
    check_census(n, gpu=True)


def test_the_widths_of_the_tested_dimensions():
    assert [guard_log2(n) for n in DIMS + (10, )] == [19, 19, 18, 18]
