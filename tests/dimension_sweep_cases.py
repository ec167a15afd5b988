"""Small cases at EVERY compile-time dimension, shared by tests/test_dispatch.py (their floors, on the CPU) and
tests/test_dimension_sweep_gpu.py: the dispatch over the dimension (csrc/nt_dispatch.hpp) reaches one launcher a dimension and
family, and the larger cases of the sibling tests sample five to seven dimensions each.  Every expected value is the oracle's.

BoxScene, n = 3 .. 24
  rays     every 15th ray of ray_color_cases.box_rays(n): 134 rays, two waves and a partial one
  refine   adaptive_cases.box_expected(n, 2, BOX_CAMERA) at a 16 x 16 view
CompositeScene, N = 3 .. 10: the opaque orthoplex of tests/test_composite_matrix.py (lean_flat(n), camera(n), params(n, "lit"))
  rays     the camera's own rays through a 13 x 10 lattice of a 97 x 61 view: 130 rays, for ray_colors, intersect_rays and -- with distance
           FLT_MAX, where _occludes' far-child rule lets some rays that hit go unblocked -- occludes_rays
  hits     the primary-hit records of a 9 x 7 view, as primary_hit_cases builds them
  The field of view of both views is view_fov(N), not the 0.8 of params(n, "lit"): seen from that camera under 0.8 the
  orthoplex covers 21 of the 63 pixels at N = 3 and 7 at N = 10 (it holds a ball of radius 1 / sqrt(N) only), so the floor
  below could not hold from N = 4 up.  view_fov(N) makes that ball's radius 2.5 pixels of the 9 x 7 view -- about 20 of its
  63 pixels -- while the view's corners, 5.7 pixels out, stay outside the polytope.

Floors, by the oracle alone (check_*): at least a quarter of a case's rays or pixels hit something and at least one misses;
the refine case flags pixels and leaves pixels unflagged; some of the rays are blocked and some are not.

Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import adaptive_cases as ac
import oracle_binding as ob
import primary_hit_cases as ph
import ray_color_cases as rc
import ray_query_cases as rq

f32 = np.float32
FLT_MAX = rq.FLT_MAX

BOX_STEP = 15                   # of box_rays(n)'s 2 000 rays
BOX_CAMERA = 12                 # of adaptive_cases.box_cameras(n): the diagonal one, the cube in the middle of the view
REFINE_VIEW = (16, 16)
RAY_LATTICE = (13, 10)          # columns, rows
HITS_VIEW = (9, 7)
INBALL_PIXELS = 2.5             # the radius of the orthoplex's inscribed ball in the 9 x 7 view


class Case(object):
    pass


def _freeze(c):
    for v in vars(c).values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


# ------------------------------------------------------------------ BoxScene
@functools.lru_cache(maxsize=None)
def box_rays(n):
    r = rc.box_rays(n)
    c = Case()
    c.origins = np.ascontiguousarray(r.origins[::BOX_STEP])
    c.directions = np.ascontiguousarray(r.directions[::BOX_STEP])
    c.ref = np.ascontiguousarray(r.ref[::BOX_STEP])
    c.hit = c.ref[:, 0] != c.ref[:, 1]              # the cube's colours are (s, s / 2, s / 2), the background's grey or cyan
    return _freeze(c)


def box_refine(n):
    """adaptive_cases.Expected of the case's view"""
    return ac.box_expected(n, 2, BOX_CAMERA, ac.T, *REFINE_VIEW)


def check_box(n):
    r = box_rays(n)
    assert 129 <= len(r.ref) <= 192 and len(r.ref) % 64, len(r.ref)
    assert r.hit.sum() * 4 >= len(r.hit) and not r.hit.all(), (n, int(r.hit.sum()), len(r.hit))
    e = box_refine(n)
    hit = e.P[..., 0] != e.P[..., 1]
    assert hit.sum() * 4 >= hit.size and not hit.all(), (n, int(hit.sum()))
    assert e.mask.any() and not e.mask.all(), (n, int(e.mask.sum()))
    assert np.abs(e.M - e.P)[e.mask].max() > ac.MIN_REFINE_DELTA, n          # (refining changes what is drawn)


# ------------------------------------------------------------------ CompositeScene
def view_fov(n, origin):
    """the field of view under which the ball of radius 1 / sqrt(n) round the centre of the scene, seen from `origin`, has a
    radius of INBALL_PIXELS pixels of the 9 x 7 view: tan(fov / 2) spans half its width"""
    sin_a = (1.0 / np.sqrt(n)) / float(np.linalg.norm(np.asarray(origin, np.float64)))
    tan_a = sin_a / np.sqrt(1.0 - sin_a * sin_a)
    return float(2.0 * np.arctan(tan_a * (HITS_VIEW[0] / 2.0) / INBALL_PIXELS))


@functools.lru_cache(maxsize=None)
def composite(n):
    import test_composite_matrix as tcm
    c = Case()
    c.n = n
    c.flat = tcm._scene_flat(tcm.lean_flat(n), "lit")
    c.params = tcm.params(n, "lit")
    c.origin, c.axes = tcm.camera(n)
    c.fov = view_fov(n, c.origin)
    prune = len(c.flat["solid_types"]) == 0          # (the library's rule, as ray_query_cases.batches has it)
    orc = rq.Oracle(n, c.flat, False, prune)
    lo, hi = np.asarray(c.flat["aabb_start"], f32), np.asarray(c.flat["aabb_end"], f32)

    # ---- rays: colours and closest hits
    cols, rows = RAY_LATTICE
    xs, ys = np.meshgrid(3 + 7 * np.arange(cols), 3 + 6 * np.arange(rows))
    c.directions = rc.camera_rays(c.axes, xs.ravel(), ys.ravel(), tcm.W, tcm.H, c.fov)
    count = len(c.directions)
    c.origins = np.ascontiguousarray(np.repeat(c.origin[None], count, axis=0))
    c.colours = rc.CentrePixel(n, c.flat, c.params, False, prune).colors(c.origins, c.directions)
    none = np.full(count, -1, np.int32)
    c.t_near, c.t_far = np.full(count, -FLT_MAX, f32), np.full(count, FLT_MAX, f32)
    c.none = none
    c.closest = orc.intersects(c.origins, c.directions, c.t_near, c.t_far, none, none)

    c.distance = np.full(count, FLT_MAX, f32)
    c.blocked = orc.occludes(c.origins, c.directions, c.distance, c.t_near, c.t_far, none, none)

    # ---- primary hits (primary_hit_cases._expected on this scene)
    w, h = HITS_VIEW
    osc = ob.OracleScene(n, c.origin, c.axes, c.fov)
    d = np.stack([osc.primary_dir(x, y, w, h) for y in range(h) for x in range(w)]).astype(f32)
    t0 = ph.aabb_distance(lo, hi, c.origin, d)
    enter = np.nonzero(t0 >= 0)[0]
    out = dict(dist=np.full(w * h, FLT_MAX, f32), item=np.full(w * h, -1, np.int32), lane=np.full(w * h, -1, np.int32),
               n_transparent=np.zeros(w * h, np.int32), normal_origin=np.zeros((w * h, n), f32), normal=np.zeros((w * h, n), f32))
    if len(enter):
        e_none = np.full(len(enter), -1, np.int32)
        r = orc.intersects(np.repeat(c.origin[None], len(enter), axis=0), d[enter], t0[enter], np.full(len(enter), FLT_MAX), e_none, e_none)
        for key in out:
            out[key][enter] = r[key]
    out["normal_origin"][out["item"] < 0] = 0
    out["normal"][out["item"] < 0] = 0
    c.hits = {key: v.reshape((h, w) + v.shape[1:]) for key, v in out.items()}
    return _freeze(c)


def check_composite(n):
    c = composite(n)
    hit = c.closest["item"] >= 0
    assert len(hit) == 130
    assert hit.sum() * 4 >= len(hit) and not hit.all(), (n, int(hit.sum()))
    assert len(np.unique(c.colours[hit], axis=0)) * 2 > hit.sum(), n               # (shaded, not one colour a facet)
    b = c.blocked["blocked"]
    assert b.sum() >= 5 and (~b).sum() >= 5 and not b[~hit].any(), (n, int(b.sum()), int(hit.sum()))
    item = c.hits["item"]
    assert (item >= 0).sum() * 4 >= item.size and (item < 0).any(), (n, int((item >= 0).sum()))
