"""What an adaptive supersampled render (scene.set_adaptive_supersampling(t) with a factor s > 1) must produce,
built from the oracle alone, and the cases tests/test_adaptive_host.py and tests/test_adaptive_gpu.py share.

The expected image of a W x H render:
  P      the oracle's plain frame in the fp32 x 3 format (each component clamped to [0, 1] by the oracle's packer);
  M      the supersampled image of tests/ss_expected.py (mean_colors);
  mask   contrast > t in fp32, the contrast of a pixel the largest |P[x,y][c] - P[x',y'][c]| over the components and the
         four neighbours inside the image (none inside: 0);
  pick   M where the mask is set, P elsewhere, packed by the oracle's pack_pixel.
A pixel is *undecided* when one of its |P[x,y][c] - P[x',y'][c]| lies within UNDECIDED = 1e-4 of t: the GPU's P is only
within 1e-5 of the oracle's on composite scenes, so the two may flag such a pixel differently; there the render may show
either variant.  Every case must meet, by the oracle alone (check_case):
  undecided pixels <= 0.5 % of the image; at least 20 flagged and 20 unflagged pixels; at least one flagged pixel whose
  supersampled colour differs from P by more than 1e-3 in a component, so that no case passes without refining.

A composite *case* is (golden scene, NTRACER_* switches, variant of ray_color_cases, factors); the camera is the golden's
camera 0, the view 203 x 117, t = 0.1.  The launch each case reaches (nt_adaptive.hpp launch_refine_fixed and
launch_adaptive_flag, nt_var.hip nt_launch_refine; `route` works it out by ray_color_cases.route's rules, which are
rays_enqueue's and enqueue_adaptive's alike, and test_adaptive_host.py checks that no launch is left out):
  cell600_n4                         refine_color<N,false,false>   batches alone, camera light only
  cell600_n4 STRICT_REFERENCE        refine_color<N,false,false>   ... the reference's exact walk
  cell600_n4 lit                     refine_color<N,true,false>    reflective, two point lights, a global light, shadows
  simplex10_n10                      refine_color<N,true,true>     loose triangles in the leaves
  simplex10_n10 FORCE_VAR            refine_color_var
  feature5_n5                        refine_color_t<N,true>        transparent materials, Solids
  feature5_n5 CLEAN_NORMALS          refine_color_t<N,false>
  feature11_n11, lit12_n12           refine_color_var_t<true>      run-time n
  feature11_n11 CLEAN_NORMALS        refine_color_var_t<false>
  BoxScene n = 3, 6, 10, 16 (4)      refine_box<N>
  BoxScene n = 27                    refine_box_var
  every render and mask call         adaptive_reset                the counter of the list
  every render                       adaptive_flag<false>
  every mask call                    adaptive_flag<true>

Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import fixtures as fx
import oracle_binding as ob
import ray_color_cases as rc
import ss_expected as sx
import support as sup

f32 = np.float32
W, H = 203, 117
T = 0.1
UNDECIDED = 1e-4
MAX_UNDECIDED = 0.005
MIN_PIXELS = 20
MIN_REFINE_DELTA = 1e-3

STRICT, CLEAN, VAR = rc.STRICT, rc.CLEAN, rc.VAR
SWITCHES = rc.SWITCHES

CASES = [
    ("cell600_n4", {}, "", (2, 3, 4)),
    ("cell600_n4", STRICT, "", (2,)),
    ("cell600_n4", {}, "lit", (2, 3)),
    ("simplex10_n10", {}, "", (2, 3)),
    ("simplex10_n10", VAR, "", (2,)),
    ("feature5_n5", {}, "", (2, 3)),
    ("feature5_n5", CLEAN, "", (2,)),
    ("feature11_n11", {}, "", (2, 3)),
    ("feature11_n11", CLEAN, "", (2,)),
    ("lit12_n12", {}, "", (2, 3)),
]
BOX_CASES = [(n, s) for n in (3, 6, 10, 16, 27) for s in (2, 3, 4)] + [(6, 8), (4, 5)]
FLAG_ROUTES = {"adaptive_reset": "every call", "adaptive_flag<false>": "every render", "adaptive_flag<true>": "every mask call"}


def case_id(case):
    return rc.case_id(case[:3])


def route(case):
    return rc.route(case[:3]).replace("rays_", "refine_")


def box_route(n):
    return rc.box_route(n).replace("rays_", "refine_")


def plain_colors(osc, w, h):
    """(h, w, 3) float32: the oracle's plain frame, clamped"""
    return osc.render(w, h, fx.RGBF32, threads=sup.worker_threads()).view(">f4").astype(f32).reshape(h, w, 3)


def _neighbour_deltas(P):
    """the |P[x,y][c] - P[x',y'][c]| of every pixel: a list of (h, w, 3) float32 arrays, -1 where the neighbour is outside"""
    out = []
    dy = np.abs(P[1:] - P[:-1]).astype(f32)
    dx = np.abs(P[:, 1:] - P[:, :-1]).astype(f32)
    for d, sl in ((dy, np.s_[1:]), (dy, np.s_[:-1]), (dx, np.s_[:, 1:]), (dx, np.s_[:, :-1])):
        a = np.full(P.shape, -1.0, f32)
        a[sl] = d
        out.append(a)
    return out


def contrast(P):
    c = np.zeros(P.shape[:2], f32)
    for a in _neighbour_deltas(P):
        c = np.maximum(c, a.max(axis=2))
    return c


def mask_of(P, t):
    return contrast(P) > f32(t)


def undecided_of(P, t):
    u = np.zeros(P.shape[:2], bool)
    for a in _neighbour_deltas(P):
        u |= ((a >= 0) & (np.abs(a.astype(np.float64) - float(f32(t))) <= UNDECIDED)).any(axis=2)
    return u


class Expected(object):
    """P, M, the mask and the undecided pixels of one (oracle scene, view, factor, threshold)"""

    def __init__(self, P, M, t):
        self.P, self.M, self.t = P, M, t
        self.mask = mask_of(P, t)
        self.undecided = undecided_of(P, t)
        self.pick = np.where(self.mask[..., None], M, P).astype(f32)
        self.other = np.where(self.mask[..., None], P, M).astype(f32)      # what an undecided pixel may show instead

    def image(self, channels, reversed_=False):
        return sx.pack(self.pick, channels, reversed_)

    def other_image(self, channels, reversed_=False):
        return sx.pack(self.other, channels, reversed_)


def expected(osc, w, h, s, t):
    return Expected(plain_colors(osc, w, h), sx.mean_colors(osc, w, h, s), t)


def check_case(e, what):
    """the conditions every case meets, by the oracle alone"""
    share = float(e.undecided.mean())
    flagged = int(e.mask.sum())
    delta = float(np.abs(e.M - e.P)[e.mask].max()) if flagged else 0.0
    print("%s: flagged %d of %d (%.2f %%), undecided %.3f %%, largest refinement %.3g" % (what, flagged, e.mask.size, 100.0 * flagged / e.mask.size, 100.0 * share, delta))
    assert share <= MAX_UNDECIDED, (what, share)
    assert flagged >= MIN_PIXELS and e.mask.size - flagged >= MIN_PIXELS, (what, flagged)
    assert delta > MIN_REFINE_DELTA, (what, delta)


# ------------------------------------------------------------------ composite cases
def case_oracle(case):
    """(n, flat, params, origin, axes, OracleScene) of a composite case: the golden's camera 0"""
    name, env, variant = case[:3]
    g = fx.load(name)
    n, flat, params = rc.case_scene((name, {}, variant))
    o, a = g["origins"][0], g["axes"][0]
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    return n, flat, params, o, a, ob.OracleScene(n, o, a, flat=flat, params=params, clean_normals=clean)


@functools.lru_cache(maxsize=None)
def _case_expected(name, envkey, variant, s, t):
    case = (name, dict(envkey), variant)
    osc = case_oracle(case)[5]
    return expected(osc, W, H, s, t)


def case_expected(case, s, t=T):
    name, env, variant = case[:3]
    # (the oracle's colours depend on NTRACER_CLEAN_NORMALS alone among the switches)
    key = tuple(sorted((k, v) for k, v in env.items() if k == "NTRACER_CLEAN_NORMALS"))
    return _case_expected(name, key, variant, s, t)


# ------------------------------------------------------------------ BoxScene cases
def box_cameras(n):
    import test_supersampling_gpu as tss
    return tss.box_cameras(n)


BOX_CAMERAS = (2, 7, 12)          # of box_cameras(n): stress cameras 14 and 58 (1 % and 2-3 % flagged at t = 0.1), and the diagonal one


@functools.lru_cache(maxsize=None)
def box_expected(n, s, camera, t=T, w=W, h=H):
    o, a = box_cameras(n)[camera]
    return expected(ob.OracleScene(n, o, a), w, h, s, t)
