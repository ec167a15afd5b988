#!/usr/bin/env python3
"""What box_tile_kernel's codes wave says about the 64-pixel stretches of a frame, restated in numpy (CPU, fp32, 1/x for
v_rcp_f32): box_stretch_code2 of ntracer_amd/csrc/nt_box.hpp -- the code of every stretch (0 culled, K + 1 one face, 14
near-tie, 15 sorted ray by ray) and, for codes 14 and 15, the stretch's sets (T: the faces that can be a ray's answer, C: the
coordinates one of them could fail at) -- and, ray by ray, the two classifiers of a code-15 row: box_classify over all N
slabs and box_classify_sets over T and C alone.

    python3 tools/box_sets_census.py [--sample 4000] [--seed 7]

prints, for the bench's 160 cameras of BoxScene(6) at 1920 x 1080 (tests/golden/box_n6_1920x1080.npz): the share of every row
class, the (|T|, |C|) table of the code-15 stretch-rows, and on a seeded sample of them the share of rows with an unclear lane
under each classifier and the number of rays whose "hit" or "miss" from the restricted classifier is not the full one's
verdict (which has to be zero).  tests/test_box_sets_census.py pins the shares; tests/test_box_classify_sets.py picks its
cameras with stretch_codes()."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MARGIN = F(1e-5)            # NT_BOX_MARGIN
INF = F(np.inf)


def _rcp(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (F(1.0) / x).astype(F)


def _fma(a, b, c):
    """fmaf: the product is exact in double; the second rounding (double -> float) almost never shows"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _med3(a, b, c):
    return np.fmax(np.fmin(a, b), np.fmin(np.fmax(a, b), c))


def _margin(origin):
    return F(MARGIN * F(F(1.0) + np.max(np.abs(origin))))


def screen(w, h, fov=0.8):
    half_w, half_h = F(w) / F(2), F(h) / F(2)
    fovI = F(np.tan(F(fov) / F(2))) / half_w
    return half_w, half_h, F(fovI)


TIE_SURE_MAX_ORIGIN = F(4.5)        # NT_BOX_TIE_SURE_MAX_ORIGIN


def stretch_codes(origin, axes, w, h, fov=0.8, rows=None):
    """codes and sets of every 64-pixel stretch of the rows `rows` (default: all h) of a w x h frame seen from (origin, axes):
    two arrays [len(rows)][ceil(w / 64)], uint32.  sets: bits 0..9 T, bits 10..19 C, bit 31 valid (N <= 10)."""
    return _stretch(origin, axes, w, h, fov, rows)[:2]


def stretch_sure_hit(origin, axes, w, h, fov=0.8, rows=None, limit=TIE_SURE_MAX_ORIGIN):
    """stretch_codes' two arrays and box_stretch_code2's "sure hit" bit (bit 24 of the device's sets word) as a third, bool: the
    stretch has valid sets with C == T, no slab can be left inside the window of tau that holds every test made there --
    (t_hi - t_lo) * max over all axes of (|vc_j| + g_j) <= 1 -- and |o_j| <= limit on every axis of T.  Every ray of such a stretch is a
    hit, at a face of T, for the reference (nt_box.hpp, NT_BOX_TIE_SURE_MAX_ORIGIN)."""
    return _stretch(origin, axes, w, h, fov, rows, limit)


def _stretch(origin, axes, w, h, fov=0.8, rows=None, limit=TIE_SURE_MAX_ORIGIN):
    org = np.asarray(origin, F)
    right, up, fwd = (np.asarray(axes, F)[k] for k in range(3))
    n = len(org)
    half_w, half_h, fovI = screen(w, h, fov)
    ys = np.arange(h) if rows is None else np.asarray(rows)
    ncols = (w + 63) // 64
    col = np.broadcast_to(np.arange(ncols)[None, :], (len(ys), ncols)).reshape(-1)
    y = np.broadcast_to(ys[:, None], (len(ys), ncols)).reshape(-1)
    m = _margin(org)
    hh = F(F(F(1.0) + F(F(2.0) * m)) + F(1e-3))
    sxc = (fovI * (((col * 64).astype(F) + F(31.5)) - half_w)).astype(F)
    sy = (fovI * (y.astype(F) - half_h)).astype(F)
    spread = F(F(32.0) * fovI)
    S = len(col)
    with np.errstate(all="ignore"):
        tlo, thi = np.zeros(S, F), np.full(S, INF, F)
        vc, g = [], []
        for j in range(n):
            v = ((fwd[j] + right[j] * sxc).astype(F) - (up[j] * sy).astype(F)).astype(F)
            gj = F(_fma(spread, np.abs(right[j]), F(1e-6)))
            vc.append(v)
            g.append(gj)
            pa, qa = (v + gj).astype(F), F(-hh - org[j])
            pb, qb = (v - gj).astype(F), F(hh - org[j])
            ra, rb = (qa * _rcp(pa)).astype(F), (qb * _rcp(pb)).astype(F)
            ap, bp = pa >= 0, pb >= 0
            tlo = np.fmax(np.fmax(tlo, np.where(ap, ra, -INF)), np.where(bp, -INF, rb))
            thi = np.fmin(np.fmin(thi, np.where(ap, INF, ra)), np.where(bp, rb, INF))
        live = ~(tlo > thi)
        code = np.where(live, 15, 0).astype(np.uint32)
        tn, tn2 = np.full(S, -INF, F), np.full(S, -INF, F)
        vK, gK, oK, K = np.zeros(S, F), np.zeros(S, F), np.zeros(S, F), np.zeros(S, np.int64)
        for j in range(n):
            nr = ((np.where(vc[j] < 0, F(1.0), F(-1.0)) - org[j]).astype(F) * _rcp(vc[j])).astype(F)
            tn2 = _med3(tn, tn2, nr)
            later = nr > tn
            vK, gK, oK, K = np.where(later, vc[j], vK), np.where(later, g[j], gK), np.where(later, org[j], oK), np.where(later, j, K)
            tn = np.fmax(tn, nr)
        vKa, vKb = (vK - gK).astype(F), (vK + gK).astype(F)
        one = live & (K < 13) & (vKa * vKb > 0)
        num = (np.where(vK < 0, F(1.0), F(-1.0)) - oK).astype(F)
        t1, t2 = (num * _rcp(vKa)).astype(F), (num * _rcp(vKb)).astype(F)
        t_lo, t_hi = (np.fmin(t1, t2) * F(1.0 - 1e-6)).astype(F), (np.fmax(t1, t2) * F(1.0 + 1e-6)).astype(F)
        rK = ((m * _rcp((np.abs(vK) - gK).astype(F))).astype(F) * F(1.0 + 1e-6)).astype(F)
        ok = one & (t_lo > F(1e-3)) & (t_hi < F(1e30))
        for j in range(n):
            va, vb = (vc[j] - g[j]).astype(F), (vc[j] + g[j]).astype(F)
            pmax = (org[j] + np.fmax(vb * t_lo, vb * t_hi)).astype(F)
            pmin = (org[j] + np.fmin(va * t_lo, va * t_hi)).astype(F)
            lim = (F(F(F(1.0) - m) - F(1e-4)) - ((np.abs(vc[j]) + g[j]).astype(F) * rK).astype(F)).astype(F)
            ok &= (K == j) | ((pmax <= lim) & (pmin >= -lim))
        code = np.where(ok, (K + 1).astype(np.uint32), code)
        tie = (code == 15) & ~(((tn - tn2).astype(F) * np.abs(vK)).astype(F) > m)
        code = np.where(tie, 14, code).astype(np.uint32)
        sets = np.zeros(S, np.uint32)
        sure = np.zeros(S, bool)
        if n <= 10:
            rA, rB, rV = [], [], []
            TN, TH = np.full(S, -INF, F), np.full(S, -INF, F)
            for j in range(n):
                va, vb = (vc[j] - g[j]).astype(F), (vc[j] + g[j]).astype(F)
                nm = (np.where(vc[j] < 0, F(1.0), F(-1.0)) - org[j]).astype(F)
                e1, e2 = (nm * _rcp(va)).astype(F), (nm * _rcp(vb)).astype(F)
                lo, hi = np.fmin(e1, e2), np.fmax(e1, e2)
                same = va * vb > 0
                A = np.where(same, (lo - (np.abs(lo) * F(1e-6)).astype(F)).astype(F), -INF).astype(F)
                B = np.where(same, (hi + (np.abs(hi) * F(1e-6)).astype(F)).astype(F), INF).astype(F)
                V = np.where(same, (np.abs(vc[j]) - g[j]).astype(F), F(0.0)).astype(F)
                rA.append(A); rB.append(B); rV.append(V)
                TN, TH = np.fmax(TN, A), np.fmax(TH, B)
            vmin = np.full(S, INF, F)
            for j in range(n):
                vmin = np.where(rB[j] >= TN, np.fmin(vmin, rV[j]), vmin)
            M = ((m * _rcp(vmin)).astype(F) * F(1.0 + 1e-5)).astype(F)
            T, Cs = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
            s_lo = np.full(S, INF, F)
            for j in range(n):
                inT = rB[j] >= (TN - M).astype(F)
                T |= np.where(inT, np.uint32(1 << j), np.uint32(0))
                s_lo = np.where(inT, np.fmin(s_lo, rA[j]), s_lo)
            s_hi = TH
            for j in range(n):
                va, vb = (vc[j] - g[j]).astype(F), (vc[j] + g[j]).astype(F)
                pmax = (org[j] + np.fmax(vb * s_lo, vb * s_hi)).astype(F)
                pmin = (org[j] + np.fmin(va * s_lo, va * s_hi)).astype(F)
                lim = F(F(F(1.0) - m) - F(1e-4))
                inC = ((T >> np.uint32(j)) & 1).astype(bool) | ~((pmax <= lim) & (pmin >= -lim))
                Cs |= np.where(inC, np.uint32(1 << j), np.uint32(0))
            valid = (vmin > 0) & (s_lo > F(1e-3)) & (s_hi < F(1e30))
            sets = np.where(valid & (code >= 14), np.uint32(0x80000000) | (Cs << np.uint32(10)) | T, np.uint32(0)).astype(np.uint32)
            # the "sure hit" bit
            wmax, omax_T = np.zeros(S, F), np.zeros(S, F)
            for j in range(n):
                inT = ((T >> np.uint32(j)) & 1).astype(bool)
                wmax = np.fmax(wmax, np.fmax(np.abs((vc[j] - g[j]).astype(F)), np.abs((vc[j] + g[j]).astype(F))))
                omax_T = np.where(inT, np.fmax(omax_T, np.abs(org[j])), omax_T)
            with np.errstate(invalid="ignore"):
                sure = (sets != 0) & (Cs == T) & (((s_hi - s_lo).astype(F) * wmax).astype(F) <= F(1.0)) & (omax_T <= F(limit))
    return code.reshape(len(ys), ncols), sets.reshape(len(ys), ncols), sure.reshape(len(ys), ncols)


SPAN_MAX_N = 10             # NT_BOX_SPAN_MAX_N
SPAN_SLACK = 1e-4           # NT_BOX_SPAN_SLACK
SPAN_TAU_MIN = 1e-3         # NT_BOX_SPAN_TAU_MIN
SPAN_NONE = (F(-np.inf), F(np.inf))
SPAN_EMPTY = (F(np.inf), F(-np.inf))


def strip_span(origin, axes):
    """nt_box_strip_span (ntracer_amd/csrc/nt_box_span.hpp) in numpy, float64: the interval (lo, hi) of sx outside which no ray of
    the camera comes within h of the cube at a tau > 0 -- the extremes of a / tau over the vertices of
    P = { -h - o_j <= tau fwd_j + a right_j - b up_j <= h - o_j } -- as two fp32 numbers.  SPAN_NONE (-inf, inf): no statement;
    SPAN_EMPTY (inf, -inf): no ray at all."""
    import itertools
    org = np.asarray(origin, F)
    ax = np.asarray(axes, F)
    n = len(org)
    if n < 3 or n > SPAN_MAX_N or not (np.isfinite(org).all() and np.isfinite(ax[:3]).all()):
        return SPAN_NONE
    right, up, fwd = (ax[k].astype(np.float64) for k in range(3))
    m = _margin(org)
    h = np.float64(F(F(F(1.0) + F(F(2.0) * m)) + F(1e-3)))
    omax = np.float64(np.max(np.abs(org)))
    c = np.stack([fwd, right, -up], 1)                       # [n][3]
    lo_b, hi_b = -h - org.astype(np.float64), h - org.astype(np.float64)
    length = np.sqrt((c * c).sum(1))

    def rel_of(i, j, k):
        # (the C++ function's det3, operation for operation: whether a determinant is zero AS COMPUTED decides here)
        a, b, d = c[i], c[j], c[k]
        det = a[0] * (b[1] * d[2] - b[2] * d[1]) - a[1] * (b[0] * d[2] - b[2] * d[0]) + a[2] * (b[0] * d[1] - b[1] * d[0])
        with np.errstate(all="ignore"):
            r = abs(det) / (length[i] * length[j] * length[k])
        return 0.0 if np.isnan(r) else r
    # an axis that forms a badly conditioned triple with two axes already taken is left out, constraint and all: a larger P
    keep = []
    for q in range(n):
        if not any(0.0 < rel_of(i, j, q) < 1e-6 for i, j in itertools.combinations(keep, 2)):
            keep.append(q)
    c, lo_b, hi_b, length = c[keep], lo_b[keep], hi_b[keep], length[keep]
    n = len(keep)
    gram = c.T @ c
    gscale = gram[0, 0] * gram[1, 1] * gram[2, 2]
    diag = np.diag(gram)
    if not (gscale > 0 and diag.min() >= 1e-6 * diag.max() and np.linalg.det(gram) > 1e-6 * gscale):
        return SPAN_NONE
    tri = np.array(list(itertools.combinations(range(n), 3)))
    mats = c[tri]                                             # [t][3][3]
    with np.errstate(all="ignore"):
        rel = np.abs(np.linalg.det(mats)) / length[tri].prod(1)
    good = np.where(np.isnan(rel), 0.0, rel) >= 1e-9        # (among the axes kept: at least 1e-6, or zero up to rounding)
    tri, mats = tri[good], mats[good]
    if len(tri) == 0:
        return SPAN_EMPTY
    side = np.array(list(itertools.product((0, 1), repeat=3)))                      # [8][3]
    rhs = np.where(side[None, :, :] == 1, hi_b[tri][:, None, :], lo_b[tri][:, None, :])   # [t][8][3]
    pts = np.linalg.solve(mats[:, None, :, :], rhs[..., None])[..., 0]              # [t][8][3]: tau, a, b
    val = pts @ c.T                                                                  # [t][8][n]
    tol = 1e-7 * (h + omax)
    own = np.zeros((len(tri), 1, n), bool)
    np.put_along_axis(own, tri[:, None, :], True, 2)
    inside = (own | ((val >= lo_b - tol) & (val <= hi_b + tol))).all(2)
    v = pts[inside]
    if len(v) == 0 or v[:, 0].max() <= -SPAN_TAU_MIN:
        return SPAN_EMPTY
    if not v[:, 0].min() > SPAN_TAU_MIN:
        return SPAN_NONE
    sx = v[:, 1] / v[:, 0]
    lo, hi = sx.min(), sx.max()
    lo -= SPAN_SLACK * (1.0 + abs(lo))
    hi += SPAN_SLACK * (1.0 + abs(hi))
    flo, fhi = F(lo), F(hi)
    if np.float64(flo) > lo:
        flo = np.nextafter(flo, F(-np.inf))
    if np.float64(fhi) < hi:
        fhi = np.nextafter(fhi, F(np.inf))
    return flo, fhi


def strip_sx(w, col, fov=0.8):
    """the sx of the first and of the last pixel of column strip `col` of a w-wide frame, as box_tile_kernel forms them"""
    half_w, _, fovI = screen(w, 1, fov)
    x0, x1 = col * 64, min(col * 64 + 63, w - 1)
    return F(fovI * F(F(x0) - half_w)), F(fovI * F(F(x1) - half_w))


def strips_kept(origin, axes, w, fov=0.8):
    """which of the ceil(w / 64) column strips box_tile_kernel's span test keeps: bool [ncols]"""
    lo, hi = strip_span(origin, axes)
    ncols = (w + 63) // 64
    out = np.ones(ncols, bool)
    for col in range(ncols):
        s0, s1 = strip_sx(w, col, fov)
        out[col] = not (max(s0, s1) < lo or min(s0, s1) > hi)
    return out


def popcount(x):
    x = np.asarray(x, np.uint32)
    return sum(((x >> np.uint32(k)) & 1).astype(np.int64) for k in range(10))


def set_sizes(sets):
    """(|T|, |C|) of valid sets"""
    return popcount(sets & np.uint32(0x3ff)), popcount((sets >> np.uint32(10)) & np.uint32(0x3ff))


def rays_of(origin, axes, w, h, y, col, fov=0.8):
    """the 64 unnormalised directions of stretch `col` of row y, as box_tile_kernel forms them: [64][n]"""
    right, up, fwd = (np.asarray(axes, F)[k] for k in range(3))
    half_w, half_h, fovI = screen(w, h, fov)
    x = np.minimum(col * 64 + np.arange(64), w - 1)
    sx = (fovI * (x.astype(F) - half_w)).astype(F)
    sy = F(fovI * F(F(y) - half_h))
    base = (fwd[None, :] + (right[None, :] * sx[:, None]).astype(F)).astype(F)
    return (base - (up * sy).astype(F)[None, :]).astype(F)


HIT, MISS, UNCLEAR = 0, 1, 2


def classify(origin, v, axes_T=None, axes_C=None):
    """box_classify (axes_T = axes_C = None: all N slabs) or box_classify_sets (the slabs of T, the coordinates of C) for the rays
    v [L][n]: (verdict [L], v_K [L])"""
    o = np.asarray(origin, F)
    n = len(o)
    if axes_C is None:
        axes_T = axes_C = list(range(n))
    m = _margin(o)
    m1p = F(F(1.0) + m)
    L = len(v)
    with np.errstate(all="ignore"):
        tn, tn2, vK = np.full(L, -INF, F), np.full(L, -INF, F), np.zeros(L, F)
        tnp, tfp = np.full(L, -INF, F), np.full(L, INF, F)
        for j in axes_C:
            inv = _rcp(v[:, j])
            c0 = (-o[j] * inv).astype(F)
            tfp = np.fmin(tfp, _fma(np.abs(inv), m1p, c0))
            if j in axes_T:
                nr = (c0 - np.abs(inv)).astype(F)
                tnp = np.fmax(tnp, _fma(-np.abs(inv), m1p, c0))
                later = nr > tn
                tn2 = _med3(tn, tn2, nr)
                vK = np.where(later, v[:, j], vK)
                tn = np.fmax(tn, nr)
        miss = (tnp > tfp) | (tfp < 0)
        c = F(F(1.0) - m)
        total = np.zeros(L, F)
        for j in axes_C:
            total = (total + np.fmax(np.abs(_fma(v[:, j], tn, o[j])), c)).astype(F)
        inside = (total - F(F(len(axes_C)) * c)).astype(F) <= F(F(1.5) * m)
        sole = ((tn - tn2).astype(F) * np.abs(vK)).astype(F) > m
        front = (tn > F(1e-3)) & (tn < F(1e30))
        hit = ~miss & inside & sole & front
    return np.where(hit, HIT, np.where(miss, MISS, UNCLEAR)), vK


def compare_classifiers(origin, axes, w, h, y, col, sets, fov=0.8):
    """one code-15 stretch-row with valid sets: (unclear lane under box_classify, under box_classify_sets, rays whose restricted
    hit / miss is not the full verdict)"""
    v = rays_of(origin, axes, w, h, y, col, fov)
    n = v.shape[1]
    T = [j for j in range(n) if (int(sets) >> j) & 1]
    Cx = [j for j in range(n) if (int(sets) >> (10 + j)) & 1]
    full, fK = classify(origin, v)
    part, pK = classify(origin, v, T, Cx)
    wrong = ((part == HIT) & ~((full == HIT) & (fK == pK))) | ((part == MISS) & (full != MISS))
    return bool((full == UNCLEAR).any()), bool((part == UNCLEAR).any()), int(wrong.sum())


def bench_census(sample=4000, seed=7, out=None):
    """the census of the bench's call: 160 cameras x 1080 rows x 30 stretches"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "box_n6_1920x1080.npz"))
    W, H = 1920, 1080
    origins, axes = np.asarray(g["origins"], F), np.asarray(g["axes"], F)
    counts = np.zeros(16, np.int64)
    pairs = {}
    rows15 = []                  # (camera, y, col, sets) of code-15 stretch-rows with valid sets
    invalid = 0
    for k in range(len(origins)):
        code, sets = stretch_codes(origins[k], axes[k], W, H)
        counts += np.bincount(code.reshape(-1), minlength=16)[:16]
        is15 = code == 15
        ok = is15 & ((sets >> np.uint32(31)) != 0)
        invalid += int((is15 & ~ok).sum())
        t, c = set_sizes(sets[ok])
        for key, cnt in zip(*np.unique(np.stack([t, c], 1), axis=0, return_counts=True)):
            pairs[tuple(int(q) for q in key)] = pairs.get(tuple(int(q) for q in key), 0) + int(cnt)
        yy, cc = np.nonzero(ok)
        rows15 += [(k, int(a), int(b), int(sets[a, b])) for a, b in zip(yy, cc)]
    total = int(counts.sum())
    n15 = int(counts[15])
    res = {"stretch_rows": total,
           "share": {"culled": counts[0] / total, "one_face": counts[1:14].sum() / total, "near_tie": counts[14] / total, "ray_by_ray": n15 / total},
           "code15_rows": n15, "code15_sets_not_valid": invalid / max(n15, 1),
           "pairs": {k: v / max(n15, 1) for k, v in sorted(pairs.items(), key=lambda kv: -kv[1])}}
    sel = np.random.default_rng(seed).choice(len(rows15), size=min(sample, len(rows15)), replace=False)
    uf = up_ = wrong = 0
    for i in sel:
        k, y, col, s = rows15[i]
        a, b, wr = compare_classifiers(origins[k], axes[k], W, H, y, col, s)
        uf += a
        up_ += b
        wrong += wr
    res["sample"] = {"rows": len(sel), "rays": 64 * len(sel), "rows_unclear_full": uf / len(sel), "rows_unclear_sets": up_ / len(sel),
                     "rays_where_sets_verdict_is_not_the_full_one": wrong}
    tsz, csz = np.array([k[0] for k in pairs]), np.array([k[1] for k in pairs])
    wgt = np.array(list(pairs.values()), np.float64)
    res["mean_T"], res["mean_C"] = float((tsz * wgt).sum() / wgt.sum()), float((csz * wgt).sum() / wgt.sum())
    if out is not None:
        p = lambda *a: print(*a, file=out)
        p("stretch-rows: %d" % total)
        for name, v in res["share"].items():
            p("  %-11s %5.1f %%" % (name, 100 * v))
        p("code-15 stretch-rows: %d; sets not valid %.1f %%; mean |T| = %.2f, mean |C| = %.2f of valid" % (n15, 100 * res["code15_sets_not_valid"], res["mean_T"], res["mean_C"]))
        p("  (|T|, |C|)   share of code-15 rows")
        for key, v in list(res["pairs"].items())[:12]:
            p("  %-12s %5.1f %%" % (key, 100 * v))
        s = res["sample"]
        p("sample of %d rows with valid sets (seed %d): an unclear lane in %.1f %% under box_classify, %.1f %% under box_classify_sets; "
          "%d of %d rays with a restricted verdict that is not the full one" % (s["rows"], seed, 100 * s["rows_unclear_full"], 100 * s["rows_unclear_sets"],
                                                                                 s["rays_where_sets_verdict_is_not_the_full_one"], s["rays"]))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    bench_census(a.sample, a.seed, out=sys.stdout)
