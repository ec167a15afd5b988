"""Scenes, cases, the oracle's answers and their floors for the run-time-n CompositeScene kernels (csrc/nt_var.hip) at
n = 17 .. 64, shared by tests/test_high_dimension_host.py (the floors and the arithmetic, on the CPU) and
tests/test_high_dimension_gpu.py.

The scenes are this module's own.  A simplex record holds the UNNORMALISED face normal, whose length is (edge length)^(n - 1):
with the edges of test_composite_matrix.comb_flat (0.044 .. 0.088) that is 6e-13 at n = 11 and exactly 0 in fp32 from n = 33,
and such a scene shows background alone whatever the kernels do.  So the edges here are near 1:

wide_comb(n, stack_depth, filled)
    comb_flat's tree -- stack_depth - 2 splits on axis 2 cut the slab 0 <= z <= 1 into stack_depth - 1 cells, the chain of
    branches down the near side, every branch's far child a leaf -- with one batch of four unit-scale simplices flat in the
    plane through the middle of every cell in `filled` (default: all, always cell 0).  A cell that is not filled is a missing
    far child: its branch is pushed and popped all the same.
mixed(n)
    wide_comb(n, 4)'s tables under the native builder's tree: batches 1 and 2, batch 0's four triangles loose, two cubes and a
    sphere that shrink with the dimension (a cube of half-edge h has a half-diagonal of h sqrt(n)), and one cut in front of the
    builder's tree made by hand (see mixed).

A *case* is (scene, n, stack_depth, kind, clean): scene "wide" or "mixed" (stack_depth None: the builder's), kind one of
test_composite_matrix.params / materials, clean the normal mode (NTRACER_CLEAN_NORMALS=1).  The camera is comb_camera(n), the view
VIEW.  Per case, each computed once per process by the oracle and frozen: frame (the RGBF32 frame and the oracle's counters),
probes (colors_at on a lattice), rays (the camera's own rays through a lattice: colours, closest hits, occlusion), tilted (those rays with every hidden
coordinate non-zero), hits (the
primary-hit records) and refine (adaptive_cases.Expected at s = 2).

The kernel each call of a case reaches: route(case, call), by the rules of composite_route (nt_api.cpp) and the launchers."""
import functools

import numpy as np

import adaptive_cases as ac
import fixtures as fx
import oracle_binding as ob
import primary_hit_cases as ph
import ray_color_cases as rc
import ray_query_cases as rq
from ntracer_amd import _lib, tracern

f32 = np.float32
FLT_MAX = rq.FLT_MAX

VIEW = (37, 21)                 # ragged against the 8 x 8 tiles
SMALL_VIEW = (9, 7)             # of the five settings
THREADS = 16                    # the oracle's
# (n, stack_depth): 64 (16 n + 4 depth + 64) bytes of LDS a block; (59, 4) is the last size without the attribute (65 536
# exactly), (59, 5) the first with it, n >= 60 needs it at any depth
DIMS = ((17, 4), (33, 4), (59, 4), (59, 5), (60, 3), (64, 4))
MIXED_DIMS = (17, 59, 64)
WIDE_KINDS = ("unlit", "lit", "transparent_reflective")
MIXED_KINDS = ("lit", "transparent")
MAX_DEPTH_N64 = 368             # 163 840 bytes, 160 KiB exactly; one deeper is refused
MAX_DEPTH_FILLED = (0, 1, 180, 366)
LDS_ATTRIBUTE = 64 * 1024       # beyond it a kernel needs hipFuncAttributeMaxDynamicSharedMemorySize
LDS_LIMIT = 160 * 1024

CALLS = ("render", "colors_at", "ray_colors", "intersect", "occludes", "primary_hits", "refine")
KERNELS = ("composite_kernel_var", "composite_kernel_var_t<true>", "composite_kernel_var_t<false>",
           "query_closest_var", "query_closest_var_t<true>", "query_closest_var_t<false>", "query_occluded_var", "query_occluded_var_t",
           "hits_closest_var", "hits_closest_var_t<true>", "hits_closest_var_t<false>",
           "rays_color_var", "rays_color_var_t<true>", "rays_color_var_t<false>",
           "refine_color_var", "refine_color_var_t<true>", "refine_color_var_t<false>")


def lds_bytes(n, depth):
    """var_lds_bytes (nt_var.hip): ray 8 n, direction 4 n, scratch 4 n, stack 4 depth and mailbox 64 bytes a lane, 64 lanes"""
    return 64 * (16 * n + 4 * depth + 64)


class Case(object):
    pass


def _freeze(c):
    for v in vars(c).values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


def _tcm():
    import test_composite_matrix as tcm
    return tcm


# ------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def _wide_comb(n, stack_depth, filled):
    tcm = _tcm()
    K = stack_depth - 2
    cells = K + 1
    filled = tuple(range(cells)) if filled is None else filled
    assert all(0 <= c < cells for c in filled) and len(set(filled)) == len(filled) and 0 in filled
    zb = np.linspace(0.0, 1.0, cells + 1).astype(f32)
    rl = n * n + n + 1
    tuck = 0.3 / (n - 3)
    mats_obj = tcm._mats()
    eye = np.eye(n)
    recs, mats, batch_of = [], [], {}
    for c in filled:
        zc = float(zb[c] + zb[c + 1]) / 2
        batch, bm = [], []
        for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))):
            leg = 0.55 + 0.07 * ((c + q) % 4)
            v0 = np.full(n, -tuck * leg)
            v0[0], v0[1], v0[2] = sx * (0.04 + 0.05 * (c % 3)), sy * (0.03 + 0.04 * (c % 2)), zc
            pts = [v0] + [v0 + (sx if i == 0 else sy if i == 1 else 1) * leg * eye[i] for i in range(n) if i != 2]
            mi = (c + q) % 3
            batch.append(tracern.Triangle.from_points([list(p) for p in pts], mats_obj[mi])._record())
            bm.append(mi)
        batch_of[c] = len(recs)
        recs.append(batch)
        mats.append(bm)
    axis, split, left, right, items = [], [], [], [], []

    def leaf(c):
        if c not in batch_of:
            return -1                                   # (the library refuses a leaf without items: an empty cell is no child)
        axis.append(-1), split.append(0.0), left.append(len(items)), right.append(1)
        items.append((batch_of[c] << 2) | _lib.KIND_BATCH)
        return len(axis) - 1

    def branch(s, near, far):
        axis.append(2), split.append(s), left.append(near), right.append(far)
        return len(axis) - 1

    # (as comb_flat) from the deepest branch up: branch j (1 = root) splits at zb[K + 1 - j]; its far child holds cell K + 1 - j
    node = leaf(0)
    for j in range(K, 0, -1):
        node = branch(float(zb[K + 1 - j]), node, leaf(K + 1 - j))
    lo, hi = np.full(n, -1.0, f32), np.full(n, 1.0, f32)
    lo[2], hi[2] = 0.0, 1.0
    flat = dict(root=node, node_axis=np.asarray(axis, np.int32), node_split=np.asarray(split, f32), node_left=np.asarray(left, np.int32),
                node_right=np.asarray(right, np.int32), items=np.asarray(items, np.int32),
                batch_recs=np.asarray(recs, f32).reshape(-1, 4, rl), batch_mats=np.asarray(mats, np.int32).reshape(-1, 4),
                tri_recs=np.zeros((0, rl), f32), tri_mats=np.zeros(0, np.int32), solid_recs=np.zeros((0, 2 * n * n + n), f32),
                solid_types=np.zeros(0, np.int32), solid_mats=np.zeros(0, np.int32), materials=tcm.MATERIALS.copy(), aabb_start=lo, aabb_end=hi)
    for v in flat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return flat


def wide_comb(n, stack_depth, filled=None):
    return _wide_comb(n, stack_depth, None if filled is None else tuple(filled))


CUBE_AT, CUBE_SCALE = (-0.16, -0.2, 0.28), 0.18 * 1.4
SPHERE_AT, SPHERE_RADIUS = (0.15, 0.13, -0.05), 0.2
CUBE2_AT = (0.3, -0.1, 0.2)
FRONT_CUT = 0.05


@functools.lru_cache(maxsize=None)
def mixed(n):
    """wide_comb(n, 4) with batch 0 loose, two cubes of orientation (1.4 / sqrt(n)) 0.18 rot and a sphere of radius 0.2, under the
    native builder's tree with one cut grafted on top.

    Where the Solids are decides whether the two normal modes can be told apart.  The reference's first leaf loop hands the
    current hit's normal ray to every test as scratch, so a hit's normal is marked only by what a LATER leaf tests: a cube that
    is tested there (it writes before it knows the outcome), or a transparent primitive that is hit there in front of it.
    - `transparent`: the sphere ends just in front of the first plane of triangles, which makes the builder cut there; the first
      cube lies behind that plane, in both cells; a ray that finds it in the near cell, beyond the cut, goes on to the far cell
      and meets a transparent triangle in front of it, whose test marks the cube's normal.
    - `lit`: everything is opaque, and only a cube tested after the hit leaves a mark.  Where the builder cuts between Solids
      changes with the seeded rotation, so that cut is made by hand: a new root splits at z = FRONT_CUT, in front of everything
      but the sphere; its near child is a leaf of the sphere and the second cube, its far child the builder's tree over all
      the primitives.  The second cube's body lies wholly beyond the cut, so every ray that hits it goes on into the builder's
      tree, where the first cube is tested for the first time: all 37 .. 58 pixels of the second cube carry a marked normal.
    By the oracle, pixels of the frame that differ between the modes at n = 17, 59, 64: lit 42, 4, 2; transparent 134, 60, 56."""
    tcm = _tcm()
    rng = np.random.default_rng(7400 + n)
    rot, _ = np.linalg.qr(rng.standard_normal((n, n)))
    cube, sphere = np.zeros(n), np.zeros(n)
    cube[:3], sphere[:3] = CUBE_AT, SPHERE_AT
    # (a Solid's position is in its own coordinates: x = O (u + p), so p = O^-1 centre)
    co, so = (CUBE_SCALE / np.sqrt(n)) * rot, SPHERE_RADIUS * np.eye(n)
    solids = [(tracern.CUBE, np.linalg.solve(co, cube), co, 1), (tracern.SPHERE, np.linalg.solve(so, sphere), so, 2)]
    cube2 = np.zeros(n)
    cube2[:3] = CUBE2_AT
    solids.append((tracern.CUBE, np.linalg.solve(co, cube2), co, 1))
    flat = tcm._tables_tree(n, wide_comb(n, 4), [1, 2], [(0, lane) for lane in range(4)], solids)
    flat = {k: np.asarray(v) if isinstance(v, (list, tuple, np.ndarray)) else v for k, v in flat.items()}
    # ---- the cut in front: a new root splits at z = FRONT_CUT; its near child is a leaf of the sphere and the second cube, its
    # far child the builder's tree
    items = list(flat["items"])
    leaf_at = len(items)
    items += [(1 << 2) | _lib.KIND_SOLID, (2 << 2) | _lib.KIND_SOLID]
    nn = len(flat["node_axis"])
    flat["node_axis"] = np.concatenate([flat["node_axis"], [-1, 2]]).astype(np.int32)
    flat["node_split"] = np.concatenate([flat["node_split"], [0.0, FRONT_CUT]]).astype(f32)
    flat["node_left"] = np.concatenate([flat["node_left"], [leaf_at, nn]]).astype(np.int32)
    flat["node_right"] = np.concatenate([flat["node_right"], [2, int(flat["root"])]]).astype(np.int32)
    flat["items"] = np.asarray(items, np.int32)
    flat["root"] = nn + 1
    for v in flat.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return flat


def tree_depth(flat):
    """nodes on the longest path of the tree: the launch's stack_depth is max(depth + 1, 2) (fill_composite, nt_api.cpp)"""
    axis, left, right = flat["node_axis"], flat["node_left"], flat["node_right"]

    def d(node):
        if node < 0:
            return 0
        if axis[node] < 0:
            return 1
        return 1 + max(d(int(left[node])), d(int(right[node])))
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    return d(int(flat["root"]))


def stack_depth_of(flat):
    return max(tree_depth(flat) + 1, 2)


def face_normal_lengths(flat):
    """|face normal| of every simplex record, in fp32 as the kernels read it"""
    n = len(flat["aabb_start"])
    recs = np.concatenate([np.asarray(flat["batch_recs"], f32).reshape(-1, n * n + n + 1), np.asarray(flat["tri_recs"], f32).reshape(-1, n * n + n + 1)])
    fn = recs[:, 1:1 + n]
    return np.sqrt((fn * fn).sum(axis=1, dtype=f32))


# ------------------------------------------------------------------ cases
def core_cases():
    out = []
    for n, depth in DIMS:
        for kind in WIDE_KINDS:
            out.append(("wide", n, depth, kind, False))
    for n in MIXED_DIMS:
        for kind in MIXED_KINDS:
            for clean in (False, True):
                out.append(("mixed", n, None, kind, clean))
    return out


def refine_cases():
    """adaptive refine at s = 2: one opaque and one transparent case per n; at the n with a mixed scene the transparent one in
    clean mode too, the only way to refine_color_var_t<false>"""
    out = []
    for n, depth in DIMS:
        out.append(("wide", n, depth, "lit", False))
        out.append(("wide", n, depth, "transparent_reflective", False))
    for n in MIXED_DIMS:
        out.append(("mixed", n, None, "transparent", True))
    return out


def limit_cases():
    return [("deep", 64, MAX_DEPTH_N64, kind, False) for kind in WIDE_KINDS]


def case_id(case):
    scene, n, depth, kind, clean = case
    return "%s-n%d%s-%s%s" % (scene, n, "" if depth is None else "-d%d" % depth, kind, "-clean" if clean else "")


def env_of(case):
    return {"NTRACER_CLEAN_NORMALS": "1"} if case[4] else {}


def base_flat(case):
    scene, n, depth, kind, clean = case
    if scene == "wide":
        return wide_comb(n, depth)
    if scene == "deep":
        return wide_comb(n, depth, MAX_DEPTH_FILLED)
    return mixed(n)


@functools.lru_cache(maxsize=None)
def scene(case):
    """the flat scene, parameters, camera and oracle scene of a case"""
    tcm = _tcm()
    kind, clean, n = case[3], case[4], case[1]
    c = Case()
    c.case, c.n, c.clean = case, n, clean
    c.flat = tcm._scene_flat(base_flat(case), kind)
    c.params = tcm.params(n, kind)
    c.fov = c.params["fov"]
    c.origin, c.axes = tcm.comb_camera(n)
    c.stack_depth = stack_depth_of(c.flat)
    c.lds = lds_bytes(n, c.stack_depth)
    c.prune = len(c.flat["solid_types"]) == 0           # (the library's rule, as ray_query_cases.batches has it)
    c.osc = ob.OracleScene(n, c.origin, c.axes, fov=c.fov, flat=c.flat, params=c.params, clean_normals=clean)
    return _freeze(c)


def route(case, call):
    """the kernel `call` of CALLS lands on: composite_route's `faithful` (nt_api.cpp) and the launchers of nt_var.hip"""
    flat = scene(case).flat
    assert case[1] > 10
    opaque = bool((np.asarray(flat["materials"])[:, 6] >= 1).all())
    solids = len(flat["solid_types"]) > 0
    faithful = not opaque or (solids and not case[4])
    alias = "false" if case[4] else "true"
    if call == "occludes":
        return "query_occluded_var" if opaque else "query_occluded_var_t"
    stem = {"render": "composite_kernel_var", "colors_at": "composite_kernel_var", "ray_colors": "rays_color_var",
            "intersect": "query_closest_var", "primary_hits": "hits_closest_var", "refine": "refine_color_var"}[call]
    return "%s_t<%s>" % (stem, alias) if faithful else stem


def probe_lattice(w=VIEW[0], h=VIEW[1]):
    ys, xs = np.mgrid[0:h:3, 0:w:4]
    return xs.ravel(), ys.ravel()


def ray_lattice():
    """18 x 10 pixels of the view: 180 rays, two full waves and a partial one"""
    xs, ys = np.meshgrid(np.arange(1, VIEW[0], 2), np.arange(1, VIEW[1], 2))
    return xs.ravel(), ys.ravel()


@functools.lru_cache(maxsize=None)
def frame(case):
    """the oracle's RGBF32 frame of the view as (H, W * 3) big-endian floats, its counters, and colors_at on the probe lattice"""
    s = scene(case)
    w, h = VIEW
    c = Case()
    buf, c.counters = s.osc.render(w, h, fx.RGBF32, threads=THREADS, counters=True)
    c.frame = buf.view(">f4")
    c.xs, c.ys = probe_lattice()
    c.probes = s.osc.colors_at(c.xs, c.ys, w, h)
    _, c.centre = s.osc.colors_at([w // 2], [h // 2], w, h, counters=True)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def rays(case):
    """the camera's own rays through ray_lattice(): the oracle's colours, closest hits and -- with distance FLT_MAX -- occlusion"""
    s = scene(case)
    n = s.n
    c = Case()
    xs, ys = ray_lattice()
    c.directions = rc.camera_rays(s.axes, xs, ys, VIEW[0], VIEW[1], s.fov)
    count = len(c.directions)
    c.origins = np.ascontiguousarray(np.repeat(s.origin[None], count, axis=0))
    c.colours = rc.CentrePixel(n, s.flat, s.params, s.clean, s.prune).colors(c.origins, c.directions)
    orc = rq.Oracle(n, s.flat, s.clean, s.prune)
    c.none = np.full(count, -1, np.int32)
    c.t_near, c.t_far = np.full(count, -FLT_MAX, f32), np.full(count, FLT_MAX, f32)
    c.closest = orc.intersects(c.origins, c.directions, c.t_near, c.t_far, c.none, c.none)
    c.distance = np.full(count, FLT_MAX, f32)
    c.blocked = orc.occludes(c.origins, c.directions, c.distance, c.t_near, c.t_far, c.none, c.none)
    return _freeze(c)


TILT = 0.0015                   # hidden components of the tilted rays' origins and directions


@functools.lru_cache(maxsize=None)
def tilted(case):
    """the rays of rays(case) pushed out of the view's 3-space: every hidden coordinate of every origin and direction is +-TILT
    (signs alternating along the coordinates, and from ray to ray), so that no component of any n-vector of the walk or of the
    shading is zero.  TILT is small because the simplices are thin in the hidden coordinates: a point further than tuck * leg =
    0.0026 below a simplex's first vertex in one of them is outside it.  The oracle's colours, closest hits and occlusion."""
    s = scene(case)
    n = s.n
    base = rays(case)
    c = Case()
    count = len(base.directions)
    sign = np.where((np.arange(n - 3)[None, :] + np.arange(count)[:, None]) % 2 == 0, 1.0, -1.0)
    c.origins = np.array(base.origins, f32)
    c.directions = np.array(base.directions, f32)
    c.origins[:, 3:] = (TILT * sign).astype(f32)
    c.directions[:, 3:] = (-TILT * sign).astype(f32)
    assert (c.directions != 0).all() and (c.origins[:, 2:] != 0).all()
    c.colours = rc.CentrePixel(n, s.flat, s.params, s.clean, s.prune).colors(c.origins, c.directions)
    orc = rq.Oracle(n, s.flat, s.clean, s.prune)
    unit = (c.directions / np.sqrt((c.directions * c.directions).sum(axis=1, dtype=f32))[:, None]).astype(f32)
    c.unit = np.ascontiguousarray(unit)
    c.closest = orc.intersects(c.origins, c.unit, base.t_near, base.t_far, base.none, base.none)
    c.blocked = orc.occludes(c.origins, c.unit, base.distance, base.t_near, base.t_far, base.none, base.none)
    return _freeze(c)


def hit_records(n, flat, origin, axes, fov, w, h, clean, prune):
    """the primary-hit records of a view, as dimension_sweep_cases.composite builds them (primary_hit_cases._expected)"""
    orc = rq.Oracle(n, flat, clean, prune)
    lo, hi = np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32)
    osc = ob.OracleScene(n, origin, axes, fov)
    d = np.stack([osc.primary_dir(x, y, w, h) for y in range(h) for x in range(w)]).astype(f32)
    t0 = ph.aabb_distance(lo, hi, origin, d)
    enter = np.nonzero(t0 >= 0)[0]
    out = dict(dist=np.full(w * h, FLT_MAX, f32), item=np.full(w * h, -1, np.int32), lane=np.full(w * h, -1, np.int32),
               n_transparent=np.zeros(w * h, np.int32), normal_origin=np.zeros((w * h, n), f32), normal=np.zeros((w * h, n), f32))
    if len(enter):
        e_none = np.full(len(enter), -1, np.int32)
        r = orc.intersects(np.repeat(np.asarray(origin, f32)[None], len(enter), axis=0), d[enter], t0[enter], np.full(len(enter), FLT_MAX), e_none, e_none)
        for key in out:
            out[key][enter] = r[key]
    out["normal_origin"][out["item"] < 0] = 0
    out["normal"][out["item"] < 0] = 0
    out["d"] = d                                         # the primary directions, for what is derived from the records
    return {key: v.reshape((h, w) + v.shape[1:]) for key, v in out.items()}


@functools.lru_cache(maxsize=None)
def hits(case):
    s = scene(case)
    c = Case()
    c.hits = hit_records(s.n, s.flat, s.origin, s.axes, s.fov, VIEW[0], VIEW[1], s.clean, s.prune)
    return _freeze(c)


REFINE_S = 2


@functools.lru_cache(maxsize=None)
def refine(case):
    """adaptive_cases.Expected of the view at s = 2, t = adaptive_cases.T"""
    return ac.expected(scene(case).osc, VIEW[0], VIEW[1], REFINE_S, ac.T)


# ------------------------------------------------------------------ the five settings, n = 64, on their general routes
SETTING_CASES = (("wide", 64, 4, "lit", False), ("mixed", 64, None, "lit", False))
AO_K = 5
PARALLEL_HALF_WIDTH = 0.6
CAMERA_LAST = 0.1               # the settings' camera stands off the view's 3-space in the last coordinate


def setting_camera(n):
    """comb_camera(n) moved by CAMERA_LAST along the last axis: every hit point then has a non-zero last coordinate, so that
    coordinate 63 of the depth cue's tint axis -- and of everything else sized NT_DEV_MAX_DIM -- bears on the answer"""
    o, a = _tcm().comb_camera(n)
    o = o.copy()
    o[n - 1] = CAMERA_LAST
    return o, a


def ao_table(n):
    """AO_K unit directions that lean back towards the camera, every coordinate non-zero.  (sphere_directions' rows are spread
    over all n dimensions: at n = 64 they leave the scene's 3-space at once, and nothing is ever blocked.)"""
    t = np.zeros((AO_K, n))
    t[:, :3] = [(0.6, 0.2, -1.0), (-0.6, 0.3, -1.0), (0.3, -0.6, -1.0), (-0.2, 0.7, -1.0), (0.1, 0.1, -1.0)]
    t[:, 3:] = 0.02 * np.where(np.arange(n - 3) % 2 == 0, 1.0, -1.0)[None, :] * (1 + np.arange(AO_K))[:, None] / AO_K
    return np.ascontiguousarray(t / np.linalg.norm(t, axis=1)[:, None], f32)


@functools.lru_cache(maxsize=None)
def settings(case):
    """what the five settings must give on the SMALL_VIEW of a case, from the oracle through lens_cases, parallel_cases, ao_cases,
    outline_cases and cue_cases: each module's rule on this scene's own records, rays and camera"""
    import ao_cases as ao
    import cue_cases as cc
    import lens_cases as lc
    import outline_cases as oc
    import parallel_cases as pc
    s = scene(case)
    n = s.n
    w, h = SMALL_VIEW
    c = Case()
    c.origin, c.axes = setting_camera(n)
    colour = rc.CentrePixel(n, s.flat, s.params, s.clean, s.prune)
    c.plain = ob.OracleScene(n, c.origin, c.axes, fov=s.fov, flat=s.flat, params=s.params, clean_normals=s.clean).render(
        w, h, fx.RGBF32, threads=THREADS).view(">f4").astype(f32).reshape(h, w, 3)
    c.records = hit_records(n, s.flat, c.origin, c.axes, s.fov, w, h, s.clean, s.prune)
    rec = c.records
    # ---- a fisheye lens (lens_cases: the lens's own directions, the oracle's colour of each live pixel)
    c.lens = lc.LENSES["fisheye"](w, h)
    live = ~c.lens.masked.reshape(-1)
    v = c.lens.directions(lc.camera_of(c.origin, c.axes))
    c.lens_colours = np.zeros((w * h, 3), f32)
    c.lens_colours[live] = colour.colors(c.origin, v[live])
    # ---- the parallel projection (parallel_cases.parallel_rays: the header's formula)
    org, fwd = pc.parallel_rays(c.origin, c.axes, w, h, PARALLEL_HALF_WIDTH)
    c.parallel_colours = colour.colors(org, np.repeat(fwd[None], len(org), axis=0))
    # ---- ambient occlusion at K = 5 (ao_cases.blocked_of)
    c.ao_table = ao_table(n)
    c.ao = ao.blocked_of(n, s.flat, s.clean, s.prune, rec, rec["d"], c.ao_table, float(f32(ao.RADIUS)), float(f32(ao.BIAS)))
    # ---- outlines (outline_cases.mask_of)
    c.outline, c.outline_counts = oc.mask_of(rec["dist"], rec["item"], rec["lane"], rec["normal"], *oc.A)
    # ---- depth cues (cue_cases.factors_of): fog and tint ranges the 0.15 and 0.85 quantiles of this view, as cue_cases.setting
    hit = rec["item"] >= 0
    axis = cc.tint_axis(n)
    assert axis[n - 1] != 0
    near, far = (f32(q) for q in np.quantile(rec["dist"][hit].astype(np.float64), (0.15, 0.85)))
    t = np.where(hit, rec["dist"], f32(0)).astype(f32)
    coord = None
    for j in range(n):
        term = (axis[j] * ((rec["d"][..., j] * t).astype(f32) + c.origin[j]).astype(f32)).astype(f32)
        coord = term if coord is None else (coord + term).astype(f32)
    lo, hi = (f32(q) for q in np.quantile(coord[hit].astype(np.float64), (0.15, 0.85)))
    c.cue = dict(fog_near=near, fog_far=far, fog_color=tuple(f32(x) for x in cc.FOG_COLOR), fog_strength=f32(cc.FOG_STRENGTH),
                 fog_background=True, tint_axis=tuple(axis), tint_lo=lo, tint_hi=hi,
                 tint_color_lo=tuple(f32(x) for x in cc.TINT_COLORS[0]), tint_color_hi=tuple(f32(x) for x in cc.TINT_COLORS[1]))
    c.cue_factors = cc.factors_of(rec["dist"], rec["item"], rec["n_transparent"], rec["d"], c.origin, c.cue)
    # (the last coordinate bears on the tint: without it the factors differ)
    blind = dict(c.cue)
    blind["tint_axis"] = tuple(axis[:n - 1]) + (f32(0),)
    c.cue_blind = cc.factors_of(rec["dist"], rec["item"], rec["n_transparent"], rec["d"], c.origin, blind)
    return _freeze(c)


def check_settings(case):
    c = settings(case)
    w, h = SMALL_VIEW
    hit = c.records["item"] >= 0
    assert hit.sum() * 4 >= w * h and (~hit).any(), (case, int(hit.sum()))
    live = ~c.lens.masked.reshape(-1)
    assert live.sum() >= 20 and (~live).any() and len(np.unique(c.lens_colours[live], axis=0)) >= 10, case
    assert len(np.unique(c.parallel_colours, axis=0)) >= 4, case           # (flat facets under one direction: a colour a facet)
    b = c.ao["blocked"]
    assert (b == 0).any() and (b < 0).any(), (case, np.unique(b, return_counts=True))
    if case[0] == "mixed":
        # (wide_comb's facets all face the camera and the samples go to the side the primary ray came from, where that scene has
        # nothing: there every count is 0.  The Solids of mixed stand in front of the facets.)
        assert (b > 0).sum() >= 5, (case, np.unique(b, return_counts=True))
    assert (c.outline != 0).sum() >= 5 and (c.outline == 0).sum() >= 5, case
    f, g = c.cue_factors[..., 0], c.cue_factors[..., 1]
    assert ((f > 0) & (f < 1)).sum() >= 5 and ((g > 0) & (g < 1)).sum() >= 5, case
    assert (c.cue_factors[..., 1] != c.cue_blind[..., 1]).sum() >= 5, case


# ------------------------------------------------------------------ floors, by the oracle alone
MIN_TRANSPARENT = 20
MIN_BLOCKED = 5


def is_lit(kind):
    return kind != "unlit"


def is_transparent(kind):
    return kind in ("transparent", "transparent_reflective")


def check_scene(flat):
    ln = face_normal_lengths(flat)
    assert len(ln) and (ln >= 1e-20).all() and (ln <= 1e20).all(), (float(ln.min()), float(ln.max()))


def check_case(case):
    kind = case[3]
    s, fr, r, hh = scene(case), frame(case), rays(case), hits(case)
    w, h = VIEW
    check_scene(s.flat)
    cnt = fr.counters
    item = hh.hits["item"]
    assert (item >= 0).sum() * 4 >= w * h and (item < 0).sum() * 10 >= w * h, (case, int((item >= 0).sum()))
    assert cnt["hits"] * 4 >= w * h, (case, cnt)
    if is_lit(kind):
        assert cnt["shadow_rays"] > 0, (case, cnt)
    hit = r.closest["item"] >= 0
    assert 130 <= len(hit) <= 190 and len(hit) % 64
    assert hit.sum() * 4 >= len(hit) and (~hit).sum() * 10 >= len(hit), (case, int(hit.sum()))
    b = r.blocked["blocked"]
    assert b.sum() >= MIN_BLOCKED and (~b).sum() >= MIN_BLOCKED, (case, int(b.sum()))
    t = tilted(case)
    thit = t.closest["item"] >= 0
    assert thit.sum() * 4 >= len(thit) and (~thit).sum() * 10 >= len(thit), (case, int(thit.sum()))
    if is_transparent(kind):
        # more rays than pixels: a ray_color call a reflection (`rays`) where the kind reflects; `transparent` alone sends no
        # ray of that kind by definition -- a transparent hit is passed in the same walk -- so there the shadow rays count too
        traced = cnt["rays"] + (0 if kind == "transparent_reflective" else cnt["shadow_rays"])
        assert traced > w * h, (case, cnt)
        assert (r.closest["n_transparent"] > 0).sum() >= MIN_TRANSPARENT, (case, int((r.closest["n_transparent"] > 0).sum()))
        assert (hh.hits["n_transparent"] > 0).sum() >= MIN_TRANSPARENT, case
    if case[0] == "mixed":
        assert cnt["solid_tests"] > 0, (case, cnt)


def normal_mode_pixels(n, kind):
    """pixels of mixed(n)'s frame on which the oracle's default and clean answers differ"""
    a, b = frame(("mixed", n, None, kind, False)), frame(("mixed", n, None, kind, True))
    return int((np.asarray(a.frame) != np.asarray(b.frame)).reshape(VIEW[1], VIEW[0], 3).any(axis=2).sum())


def normal_mode_counts(n, kind):
    """on how many pixels or rays the oracle's default and clean answers of mixed(n) differ, family by family: the frame, the
    ray-lattice colours, the closest hits' normal rays, the primary hits' normal rays"""
    d, c = ("mixed", n, None, kind, False), ("mixed", n, None, kind, True)
    rd, rc_ = rays(d), rays(c)
    hd_, hc = hits(d).hits, hits(c).hits
    differ = lambda a, b: int((np.asarray(a) != np.asarray(b)).reshape(len(a), -1).any(axis=1).sum())
    return dict(frame=normal_mode_pixels(n, kind), ray_colours=differ(rd.colours, rc_.colours),
                query_normals=differ(rd.closest["normal_origin"], rc_.closest["normal_origin"]),
                hit_normals=int((hd_["normal_origin"] != hc["normal_origin"]).any(axis=2).sum()))


def check_normal_modes(n):
    """mixed: the oracle's default and clean answers differ somewhere, under both kinds and in every family that has a <true> /
    <false> pair or a faithful / plain pair of routes -- otherwise the pair is not told apart"""
    for kind in MIXED_KINDS:
        counts = normal_mode_counts(n, kind)
        # (a marked normal ORIGIN shows in a lit colour only where it flips a shadow ray -- the point light's falloff of
        # distance^(n - 1) leaves the global light alone -- so the 180 lattice rays need not show one; the frame does)
        assert counts["frame"] >= 1 and (counts["ray_colours"] >= 1 or kind == "lit"), (n, kind, counts)
        assert counts["query_normals"] >= 3 and counts["hit_normals"] >= 10, (n, kind, counts)
    d, c = refine(("mixed", n, None, "transparent", False)), refine(("mixed", n, None, "transparent", True))
    assert (d.M != c.M).any() and (d.P != c.P).any(), n


def check_refine(case):
    e = refine(case)
    assert e.mask.any() and not e.mask.all(), (case, int(e.mask.sum()))
    assert np.abs(e.M - e.P)[e.mask].max() > ac.MIN_REFINE_DELTA, case          # (refining changes what is drawn)
