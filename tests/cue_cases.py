"""Expected depth cue factors, shared by tests/test_depth_cue_host.py and tests/test_depth_cue_gpu.py, from the oracle alone.

For every pixel (x, y) of a width x height view of a golden scene from one of its golden cameras, nothing left out: the record
(dist, item, n_transparent) of primary_hit_cases.expected, the unit direction d of primary_hit_cases.rays, the camera's origin o,
and the definition of include/ntracer_hip.h restated in sequential fp32 numpy, every operation rounded to fp32 on its own --
    item >= 0:   f = clamp01((dist - fog_near) * inv_fog);  with a tint x_k = (d_k * dist) + o_k, s = axis_0 * x_0,
                 s = s + (axis_k * x_k) for k = 1 .. n - 1, g = clamp01((s - tint_lo) * inv_tint);  without one g = -1
    item < 0, fog_background set, n_transparent == 0:   f = 1, g = -1
    otherwise    f = -1, g = -1
with inv_fog = 1 / (fog_far - fog_near) and inv_tint = 1 / (tint_hi - tint_lo) formed once in fp32.  blend() is the render's
rule on the colours.  The parameters of a scene are fp32 constants taken once from the oracle's own records at 37 x 21 from the
scene's camera PARAM_CAMERA: fog_near / fog_far the 0.15 and 0.85 quantiles of the hit distances, tint_lo / tint_hi the same
quantiles of s.  Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import fixtures as fx
import primary_hit_cases as ph
import ray_query_cases as rq

f32 = np.float32

# (scene, switches): the route each takes is pinned in test_depth_cue_host.py (CUE_ROUTES)
CASES = [
    ("cell120_n4", {}),
    ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}),
    ("cell120_n4", {"NTRACER_FORCE_VAR": "1"}),
    ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
    ("simplex10_n10", {}),
    ("feature5_n5", {}),
    ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}),
    ("feature11_n11", {}),
    ("lit12_n12", {}),
    ("feature16_n16", {}),
]
# 1 x 1; one tile; a partial tile (where simplex10_n10 hits nothing); 3 x 2 blocks of the shading pass
SIZES = [(1, 1), (8, 8), (9, 7), (37, 21)]
W, H = 37, 21
BIG = (64, 48)                      # the routes of cell120_n4 against each other, once
CAMERAS = (0, 1)                    # camera 0 looks along a flat whose hidden coordinates are constant; camera 1 spreads them
PARAM_CAMERA = {"feature11_n11": 1}  # the camera the scene's parameters come from (0 unless named here)
SWITCHES = ph.SWITCHES
# (scene, variant of ray_color_cases.case_scene) of the renders: no lights, transparent materials and Solids (the general
# route), lights and shadows on batches alone (the FEAT shading pass), loose triangles
RENDERED = [("cell120_n4", ""), ("feature5_n5", ""), ("cell600_n4", "lit"), ("simplex10_n10", "")]

FOG_COLOR, FOG_STRENGTH = (0.75, 0.8125, 0.875), 0.875
TINT_COLORS = ((1.0, 0.5, 0.25), (0.25, 0.5, 1.0))

case_id = rq.case_id


def tint_axis(n):
    return np.array([(0.5, -0.25, 0.75, 1.0, -0.5)[k % 5] for k in range(n)], f32)


def clamp01(v):
    return np.maximum(f32(0), np.minimum(f32(1), v)).astype(f32)


def coordinate(name, width, height, k):
    """s [H][W] of the rule for every pixel (meaningless where nothing opaque is hit), from the oracle's d and dist"""
    e = ph.expected((name, {}), width, height, k)
    d = ph.rays(name, width, height, k)[0]
    o = ph.camera(name, k)[0]
    axis = tint_axis(d.shape[2])
    t = np.where(e["item"] >= 0, e["dist"], f32(0)).astype(f32)
    s = None
    for j in range(d.shape[2]):
        x = ((d[..., j] * t).astype(f32) + o[j]).astype(f32)
        term = (axis[j] * x).astype(f32)
        s = term if s is None else (s + term).astype(f32)
    return s


@functools.lru_cache(maxsize=None)
def setting(name, tint=True, background=False, strength=FOG_STRENGTH):
    """the depth cue of a scene: a dict of fp32 values (tint_axis None without a tint)"""
    k = PARAM_CAMERA.get(name, 0)
    e = ph.expected((name, {}), W, H, k)
    hit = e["item"] >= 0
    near, far = (f32(v) for v in np.quantile(e["dist"][hit].astype(np.float64), (0.15, 0.85)))
    lo, hi = (f32(v) for v in np.quantile(coordinate(name, W, H, k)[hit].astype(np.float64), (0.15, 0.85)))
    n = rq.scene(name)[1]
    return dict(fog_near=near, fog_far=far, fog_color=tuple(f32(c) for c in FOG_COLOR), fog_strength=f32(strength),
                fog_background=bool(background), tint_axis=tuple(tint_axis(n)) if tint else None, tint_lo=lo, tint_hi=hi,
                tint_color_lo=tuple(f32(c) for c in TINT_COLORS[0]), tint_color_hi=tuple(f32(c) for c in TINT_COLORS[1]))


def factors_of(dist, item, n_transparent, d, o, st):
    """(f, g) [H][W][2] fp32: the rule on records dist / item / n_transparent [H][W], directions d [H][W][n] and the origin o"""
    hit = item >= 0
    with np.errstate(all="ignore"):
        inv_fog = f32(f32(1) / f32(st["fog_far"] - st["fog_near"]))
        t = np.asarray(dist, f32)
        f = clamp01(((t - st["fog_near"]).astype(f32) * inv_fog).astype(f32))
        f = np.where(hit, f, f32(-1)).astype(f32)
        if st["fog_background"]:
            f = np.where(~hit & (n_transparent == 0), f32(1), f).astype(f32)
        g = np.full(item.shape, -1, f32)
        if st["tint_axis"] is not None:
            inv_tint = f32(f32(1) / f32(st["tint_hi"] - st["tint_lo"]))
            axis = np.asarray(st["tint_axis"], f32)
            s = None
            for j in range(d.shape[2]):
                x = ((d[..., j] * t).astype(f32) + o[j]).astype(f32)
                term = (axis[j] * x).astype(f32)
                s = term if s is None else (s + term).astype(f32)
            g = np.where(hit, clamp01(((s - st["tint_lo"]).astype(f32) * inv_tint).astype(f32)), f32(-1)).astype(f32)
    return np.stack([f, g], axis=2)


_FACTORS = {}


def expected(case, width, height, k, st):
    """(f, g) [H][W][2] fp32 of the view from the k-th golden camera under the setting st"""
    name, env = case
    key = (name, tuple(sorted(env.items())), width, height, k, tuple(sorted((a, b) for a, b in st.items())))
    if key not in _FACTORS:
        e = ph.expected(case, width, height, k)
        fg = factors_of(e["dist"], e["item"], e["n_transparent"], ph.rays(name, width, height, k)[0], ph.camera(name, k)[0], st)
        fg.setflags(write=False)
        _FACTORS[key] = fg
    return _FACTORS[key]


def blend(P, f, g, st):
    """the render's colours Q [H][W][3] fp32 from P [H][W][3] fp32 (clamped) and the factors"""
    P = np.asarray(P, f32)
    Q = P
    if st["tint_axis"] is not None:
        lo, hi = np.asarray(st["tint_color_lo"], f32), np.asarray(st["tint_color_hi"], f32)
        keep = (f32(1) - g).astype(f32)[..., None]
        mix = ((lo * keep).astype(f32) + (hi * g[..., None]).astype(f32)).astype(f32)
        Q = np.where((g >= 0)[..., None], (P * mix).astype(f32), Q).astype(f32)
    w = (f * st["fog_strength"]).astype(f32)[..., None]
    fog = np.asarray(st["fog_color"], f32)
    fogged = ((Q * (f32(1) - w).astype(f32)).astype(f32) + (fog * w).astype(f32)).astype(f32)
    return np.where((f >= 0)[..., None], fogged, Q).astype(f32)


def census(name):
    """(hits, (f = 0, between, f = 1), (g = 0, between, g = 1)) over the hit pixels at 37 x 21 from the scene's PARAM_CAMERA"""
    k = PARAM_CAMERA.get(name, 0)
    fg = expected((name, {}), W, H, k, setting(name))
    hit = fg[..., 0] >= 0
    out = [int(hit.sum())]
    for c in (0, 1):
        v = fg[..., c][hit]
        out.append((int((v == 0).sum()), int(((v > 0) & (v < 1)).sum()), int((v == 1).sum())))
    return tuple(out)


def check_not_vacuous(name):
    """at least three hit pixels at each end of either ramp and at least half of them strictly between"""
    hits, fs, gs = census(name)
    for lo, mid, hi in (fs, gs):
        assert lo >= 3 and hi >= 3 and 2 * mid >= hits, (name, hits, fs, gs)
    return hits, fs, gs


def scene_params(name):
    return fx.params_of(rq.scene(name)[0])
