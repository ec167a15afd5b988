"""View stacks (nt_scene_set_view_stack; include/ntracer_hip.h has the rule): what tests/test_view_stack_host.py and
tests/test_view_stack_gpu.py hold the library to.  Nothing here comes from the library.

The camera rule and the accumulation are restated in numpy with every operation rounded to float32 (numpy's multiply and add
are separate operations: no fma).  The colours come from the oracle -- OracleScene.set_camera(o_k, A_k), colors_at --, clamped as
the fp32 packer clamps them, and the bytes from the oracle's pack_pixel (ss_expected.pack).

The stacks, with `dist` the camera's distance from the scene's centre:
  disc      K = 5 on a disc of radius 0.06 dist in the right/up plane, focus = dist, weights 1/5
  slab      K = 5 along row 3 over +-0.1 dist, no focus, weights 1/5 (needs a hidden axis: not at n = 3)
  anaglyph  K = 2, +-0.05 dist along row 0, focus = dist, weights (1, 0, 0) and (0, 1, 1)
  one       K = 1, a zero offset, weight 1: the plain frame
  k64       K = 64, a seeded table with hidden components, focus = dist, seeded unequal weights whose red and green sums lie
            above 1 -- the packer's final clamp acts -- and whose blue sum lies below

check_shows asserts, from the oracle alone, that a case is not vacuous: at 37 x 21 at least 50 of the 777 pixels differ from the
plain frame by more than 1e-3 in some component."""
import functools

import numpy as np

import box_hit_cases as bc
import fixtures as fx
import oracle_binding as ob
import primary_hit_cases as ph
import ray_color_cases as rc
import ss_expected as sx

f32 = np.float32

SIZES = [(1, 1), (9, 7), (37, 21), (70, 37)]
SHOW_SIZE = (37, 21)
MIN_SHOWN = 50
STACKS = ("disc", "slab", "anaglyph", "one", "k64")
BOX_CAMERAS = (2, 4)                    # box_hit_cases.camera(n, k): "faces" and "diagonal"
BOX_FUSED_DIMS = (3, 6, 24)
BOX_FRAMES_DIMS = (25, 64)
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# (name, channels, reversed): 4-, 3-, 6- and 12-byte pixels, and a reversed one
FORMATS = [("rgbx8", fx.RGBX8, False), ("rgb24", RGB24, False), ("rgb16", fx.RGB16, False), ("rgbf32", fx.RGBF32, False),
           ("rgb24-reversed", RGB24, True)]
# (scene, environment, variant of ray_color_cases): the lean packet walk, colours above 1, transparency, run-time n, and the
# run-time-n kernels at a compile-time dimension
COMPOSITE = [("cell120_n4", {}, ""), ("cell600_n4", {}, "lit"), ("feature5_n5", {}, ""), ("feature11_n11", {}, ""),
             ("cell120_n4", {"NTRACER_FORCE_VAR": "1"}, "")]
SWITCHES = ph.SWITCHES + ("NTRACER_CHUNK_FRAMES",)


def composite_id(case):
    return rc.case_id(case) or case[0]


# ------------------------------------------------------------------ the rule
def rule_cameras(origin, axes, offsets, focus):
    """(origins [K][n], axes [K][n][n]) float32: the sample cameras of (origin, axes) by the rule, operation by operation"""
    o, A, E = np.asarray(origin, f32), np.asarray(axes, f32), np.asarray(offsets, f32)
    n = len(o)
    r = f32(1.0) / f32(focus) if focus else f32(0.0)
    origins, all_axes = np.zeros((len(E), n), f32), np.zeros((len(E), n, n), f32)
    for k, e in enumerate(E):
        s = (e[0] * A[0]).astype(f32)
        for j in range(1, n):
            s = (s + (e[j] * A[j]).astype(f32)).astype(f32)
        origins[k] = (o + s).astype(f32)
        all_axes[k] = A
        all_axes[k, 2] = (A[2] - (s * r).astype(f32)).astype(f32)
    return origins, all_axes


def clamp01(c):
    """the fp32 packer's clamp: v > 0 ? v : 0, then v < 1 ? v : 1"""
    c = np.asarray(c, f32)
    c = np.where(c > 0, c, f32(0.0))
    return np.where(c < 1, c, f32(1.0)).astype(f32)


def accumulate(frames, weights):
    """acc = 0; acc = acc + (w_k * c_k) in the order of k: frames [K][...][3] clamped colours, weights [K][3]"""
    acc = np.zeros(frames.shape[1:], f32)
    for k in range(len(frames)):
        acc = (acc + (np.asarray(weights[k], f32) * frames[k]).astype(f32)).astype(f32)
    return acc


# ------------------------------------------------------------------ the stacks
@functools.lru_cache(maxsize=None)
def stack(n, dist, name):
    """(offsets [K][n], focus or None, weights [K][3]) float32"""
    dist = float(dist)
    if name == "disc":
        K = 5
        e = np.zeros((K, n), f32)
        for k in range(1, K):
            rad, ang = 0.06 * dist * np.sqrt(k / (K - 1.0)), 2.399963229728653 * k
            e[k, 0], e[k, 1] = rad * np.cos(ang), rad * np.sin(ang)
        out = e, dist, np.full((K, 3), f32(1.0) / f32(K), f32)
    elif name == "slab":
        assert n > 3, "a slab needs a hidden axis"
        K = 5
        e = np.zeros((K, n), f32)
        e[:, 3] = np.linspace(-0.1 * dist, 0.1 * dist, K)
        out = e, None, np.full((K, 3), f32(1.0) / f32(K), f32)
    elif name == "anaglyph":
        e = np.zeros((2, n), f32)
        e[0, 0], e[1, 0] = -0.05 * dist, 0.05 * dist
        out = e, dist, np.asarray([[1, 0, 0], [0, 1, 1]], f32)
    elif name == "one":
        out = np.zeros((1, n), f32), None, np.ones((1, 3), f32)
    elif name == "k64":
        rng = np.random.default_rng(64 * n + 7)
        K = 64
        e = np.zeros((K, n), f32)
        m = min(n, 5)
        e[:, :m] = rng.uniform(-0.05 * dist, 0.05 * dist, (K, m))
        w = (rng.uniform(0.0, 2.0, (K, 3)) * np.asarray([2.5, 1.4, 0.6]) / K).astype(f32)
        assert w[:, 0].sum() > 1.5 and w[:, 1].sum() > 1.1 and w[:, 2].sum() < 0.9
        out = e, dist, w
    else:
        raise KeyError(name)
    for a in (out[0], out[2]):
        a.setflags(write=False)
    return out


def stacks_of(n):
    return tuple(s for s in STACKS if not (s == "slab" and n == 3))


# ------------------------------------------------------------------ BoxScene
def box_dist(n, k):
    return float(np.sqrt((bc.camera(n, k)[0].astype(np.float64) ** 2).sum()))


def box_stack(n, k, name):
    return stack(n, box_dist(n, k), name)


def _oracle_frames(osc, origins, axes, w, h):
    """[K][h][w][3]: the oracle's colours under every sample camera, clamped"""
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.ravel(), ys.ravel()
    out = np.zeros((len(origins), h, w, 3), f32)
    for k in range(len(origins)):
        osc.set_camera(origins[k], axes[k])
        out[k] = clamp01(osc.colors_at(xs, ys, w, h)).reshape(h, w, 3)
    return out


@functools.lru_cache(maxsize=None)
def box_plain(n, k, w, h):
    o, a = bc.camera(n, k)
    out = _oracle_frames(ob.OracleScene(n, o, a, fov=bc.FOV), o[None], a[None], w, h)[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def box_expected(n, k, name, w, h):
    """[h][w][3] float32: the sums of the rule, before the format's conversion and packing"""
    o, a = bc.camera(n, k)
    e, focus, wts = box_stack(n, k, name)
    origins, axes = rule_cameras(o, a, e, focus)
    out = accumulate(_oracle_frames(ob.OracleScene(n, o, a, fov=bc.FOV), origins, axes, w, h), wts)
    out.setflags(write=False)
    return out


def shown(rgb, plain):
    """pixels whose sum differs from the plain frame by more than 1e-3 in some component (both as the packer would clamp them)"""
    return int((np.abs(clamp01(rgb).astype(np.float64) - plain) > 1e-3).any(axis=-1).sum())


def check_box_shows(n, k, name):
    w, h = SHOW_SIZE
    cnt = shown(box_expected(n, k, name, w, h), box_plain(n, k, w, h))
    assert cnt >= MIN_SHOWN, (n, k, name, cnt)
    return cnt


# ------------------------------------------------------------------ composite scenes
def composite_camera(case, k=0):
    return ph.camera(case[0], k)


def composite_dist(case, k=0):
    n, flat, _ = rc.case_scene(case)
    ctr = 0.5 * (np.asarray(flat["aabb_start"], np.float64) + np.asarray(flat["aabb_end"], np.float64))
    return float(np.sqrt(((composite_camera(case, k)[0].astype(np.float64) - ctr) ** 2).sum()))


def composite_stack(case, name, k=0):
    return stack(rc.case_scene(case)[0], composite_dist(case, k), name)


def composite_cameras(case, name, k=0):
    e, focus, _ = composite_stack(case, name, k)
    return rule_cameras(*composite_camera(case, k), e, focus)


def composite_oracle(case, k=0):
    n, flat, params = rc.case_scene(case)
    o, a = composite_camera(case, k)
    return ob.OracleScene(n, o, a, fov=ph.fov_of(case[0]), flat=flat, params=params)


@functools.lru_cache(maxsize=None)
def _composite_frames(name, variant, stack_name, w, h):
    case = (name, {}, variant)
    origins, axes = composite_cameras(case, stack_name)
    out = _oracle_frames(composite_oracle(case), origins, axes, w, h)
    out.setflags(write=False)
    return out


def composite_frames(case, stack_name, w, h):
    """[K][h][w][3]: the oracle's clamped colours under the sample cameras (the switches of a case do not change a colour)"""
    return _composite_frames(case[0], case[2], stack_name, w, h)


def check_composite_shows(case, name):
    w, h = SHOW_SIZE
    o, a = composite_camera(case)
    plain = _oracle_frames(composite_oracle(case), o[None], a[None], w, h)[0]
    cnt = shown(accumulate(composite_frames(case, name, w, h), composite_stack(case, name)[2]), plain)
    assert cnt >= MIN_SHOWN, (case, name, cnt)
    return cnt


def pack(rgb, channels, reversed_=False):
    return sx.pack(rgb, channels, reversed_)
