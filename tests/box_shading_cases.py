"""Expected BoxScene face-shading frames, shared by tests/test_box_shading_*.py: the rule of include/ntracer_hip.h ("BoxScene face
shading") restated in sequential fp32 numpy, every operation rounded to fp32 on its own, on what tests/box_hit_cases.py works out
from the oracle alone -- expected(n, k, w, h): dirs, dist, item, lane, mask -- and box_hit_cases.camera.  Nothing here comes from
the code under test.  Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import box_hit_cases as bc

f32 = np.float32

# (dimension, switches): the compile-time-N kernels at the smallest, the bench's and the largest dimension, the run-time-n
# kernels at their first dimension and under the switch
ROUTES = [(3, {}), (6, {}), (24, {}), (25, {}), (6, {"NTRACER_FORCE_VAR": "1"})]
route_id = lambda r: "n%d%s" % (r[0], "-force-var" if r[1] else "")
DIMS = (3, 6, 24, 25)
CAMERAS = {"faces": 2, "diagonal": 4, "on-plane": 1, "nothing": 3}      # box_hit_cases.CAMERA_NAMES
# no neighbour at all; a partial tile; wider and taller than the 64 x 32 tile both ways
SIZES = [(1, 1), (9, 7), (70, 37)]
SETTINGS = ("a", "b", "c", "d", "e")
LINE_COLOR, LINE_STRENGTH = (0.9, 0.2, 0.1), 0.75
FOG_COLOR, FOG_STRENGTH = (0.5, 0.625, 0.75), 0.875
TINT_COLORS = ((1.0, 0.25, 0.5), (0.25, 1.0, 0.75))


def views():
    return [(n, name, size) for n in DIMS for name in CAMERAS for size in SIZES]


def view_id(v):
    n, name, (w, h) = v
    return "n%d-%s-%dx%d" % (n, name, w, h)


def default_table(n):
    t = np.empty((n, 2, 3), f32)
    t[...] = (1.0, 0.5, 0.5)
    return t


@functools.lru_cache(maxsize=None)
def table(n):
    """[n][2][3] in [0, 1]: every entry with g != b, all 2n entries different"""
    k = np.random.default_rng(1000 + n).integers(1, 128, (n, 2, 3))
    k[..., 1] *= 2                                         # g a multiple of 2 / 256, b not
    k[..., 2] = 2 * k[..., 2] + 1
    t = k.astype(f32) / f32(256.0)
    assert (t[..., 1] != t[..., 2]).all() and len({tuple(c) for c in t.reshape(-1, 3)}) == 2 * n
    t.setflags(write=False)
    return t


def tint_axis(n):
    return np.array([(-1.0) ** k * (k + 1) for k in range(n)], f32)


@functools.lru_cache(maxsize=None)
def setting(n, name, w, h, which):
    """The keyword arguments of BoxScene.set_face_shading for setting `which` of the view (and "lines": those of set_face_lines, or
    None):
    a  colours only;
    b  fog only, on the background too, from the fp32 25th to the 75th percentile of the view's hit distances (1 to 2 for a view
       without a hit; a view whose percentiles coincide, one pixel, takes near and twice near);
    c  tint only, along a_k = (-1)^k (k + 1), not normalised, over [-0.5, 0.5]: g clamps at both ends (over [-1, 1] it does not
       at n = 3, where the diagonal view's sums stay below 0.59);
    d  all three: fog from half the least hit distance to twice the greatest (1 to 2 without a hit), the tint over
       +-(sum |a_k| + 1), which no visible point reaches: |x_k| <= 1 + fuzz;
    e  d with face lines of both kinds at strength 0.75."""
    e = bc.expected(n, CAMERAS[name], w, h)
    hit = e["item"] >= 0
    dists = e["dist"][hit]
    kw = {}
    if which in ("a", "d", "e"):
        kw["colors"] = table(n)
    if which == "b":
        near, far = (f32(np.percentile(dists, 25)), f32(np.percentile(dists, 75))) if hit.any() else (f32(1), f32(2))
        if not far > near:
            far = f32(near * f32(2))
        kw.update(near=float(near), far=float(far), color=FOG_COLOR, strength=FOG_STRENGTH, background=True)
    if which in ("d", "e"):
        near, far = (f32(f32(0.5) * dists.min()), f32(f32(2) * dists.max())) if hit.any() else (f32(1), f32(2))
        kw.update(near=float(near), far=float(far), color=FOG_COLOR, strength=FOG_STRENGTH, background=False)
    if which in ("c", "d", "e"):
        a = tint_axis(n)
        r = 0.5 if which == "c" else float(np.abs(a).sum() + 1)
        kw.update(tint_axis=tuple(float(v) for v in a), tint_range=(-r, r), tint_colors=TINT_COLORS)
    lines = dict(color=LINE_COLOR, strength=LINE_STRENGTH) if which == "e" else None
    return kw, lines


def clamp01(v):
    """max(0, min(1, v)) with +0 for a zero"""
    v = np.where(v > 0, v, f32(0)).astype(f32)
    return np.where(v < 1, v, f32(1)).astype(f32)


def shade(o, e, colors=None, near=None, far=None, color=(0, 0, 0), strength=1.0, background=False, tint_axis=None, tint_range=None,
          tint_colors=None, lines=None):
    """The rule on the expected data `e` of a view (box_hit_cases.expected) and the camera's origin `o`, with set_face_shading's
    arguments: dict of B, P, f, g, Q and rgb (Q with the lines drawn), float32"""
    D, dist, item, lane = e["dirs"], e["dist"], e["item"], e["lane"]
    H, W, n = D.shape
    o = np.asarray(o, f32)
    T = default_table(n) if colors is None else np.asarray(colors, f32)
    hit = item >= 0
    ii, ll = np.where(hit, item, 0), np.where(hit, lane, 0)
    shade_ = np.abs(np.take_along_axis(D, ii[..., None], axis=2)[..., 0]).astype(f32)
    B = (shade_[..., None] * T[ii, ll]).astype(f32)
    d0 = D[..., 0]
    bg = np.where((d0 > 0)[..., None], np.stack([d0, d0, d0], -1), np.stack([np.zeros_like(d0), -d0, -d0], -1)).astype(f32)
    B = np.where(hit[..., None], B, bg).astype(f32)
    P = clamp01(B)
    f = np.full((H, W), -1, f32)
    g = np.full((H, W), -1, f32)
    Q = P.copy()
    cue = near is not None or far is not None or tint_axis is not None
    if cue:
        fog = near is not None or far is not None
        fnear, ffar = (f32(0.0 if near is None else near), f32(far)) if fog else (f32(0), f32(1))
        fstrength = f32(strength) if fog else f32(0)
        fcolor = np.asarray(color if fog else (0, 0, 0), f32)
        inv_fog = f32(f32(1) / f32(ffar - fnear))
        with np.errstate(all="ignore"):
            fh = clamp01(((dist - fnear).astype(f32) * inv_fog).astype(f32))
        f = np.where(hit, fh, f32(1) if (fog and background) else f32(-1)).astype(f32)
        if tint_axis is not None:
            a = np.asarray(tint_axis, f32)
            lo, hi = f32(tint_range[0]), f32(tint_range[1])
            inv_tint = f32(f32(1) / f32(hi - lo))
            with np.errstate(all="ignore"):
                x = ((D * dist[..., None]).astype(f32) + o).astype(f32)
                s = (a[0] * x[..., 0]).astype(f32)
                for k in range(1, n):
                    s = (s + (a[k] * x[..., k]).astype(f32)).astype(f32)
                gh = clamp01(((s - lo).astype(f32) * inv_tint).astype(f32))
            g = np.where(hit, gh, f32(-1)).astype(f32)
            c_lo, c_hi = np.asarray(tint_colors[0], f32), np.asarray(tint_colors[1], f32)
            keep = (f32(1) - g).astype(f32)
            mix = ((c_lo * keep[..., None]).astype(f32) + (c_hi * g[..., None]).astype(f32)).astype(f32)
            Q = np.where((g >= 0)[..., None], (P * mix).astype(f32), Q).astype(f32)
        w_ = (f * fstrength).astype(f32)
        keep = (f32(1) - w_).astype(f32)
        fogged = ((Q * keep[..., None]).astype(f32) + (fcolor * w_[..., None]).astype(f32)).astype(f32)
        Q = np.where((f >= 0)[..., None], fogged, Q).astype(f32)
    rgb = Q
    if lines is not None:
        kinds = (1 if lines.get("silhouette", True) else 0) | (2 if lines.get("edges", True) else 0)
        st = f32(lines["strength"])
        lc = np.asarray(lines["color"], f32)
        marked = (e["mask"] & np.uint8(kinds)) != 0
        drawn = ((Q * f32(f32(1) - st)).astype(f32) + (lc * st).astype(f32)).astype(f32)
        rgb = np.where(marked[..., None], drawn, Q).astype(f32)
    return dict(B=B, P=P, f=f, g=g, Q=Q, rgb=rgb)


@functools.lru_cache(maxsize=None)
def expected(n, name, w, h, which):
    """shade() of setting `which` of the view, read-only"""
    kw, lines = setting(n, name, w, h, which)
    out = shade(bc.camera(n, CAMERAS[name])[0], bc.expected(n, CAMERAS[name], w, h), lines=lines, **kw)
    for a in out.values():
        a.setflags(write=False)
    return out
