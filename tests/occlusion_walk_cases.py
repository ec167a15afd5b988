"""Scenes, rays, a model of the walk and the oracle's answers for the far-child exit of the occlusion walks, shared by
tests/test_occlusion_walk_host.py (the floors, on the CPU) and tests/test_occlusion_walk_gpu.py.

The rule under test is the reference's far-child quirk (tracer.hpp:1298): at a branch the ray crosses at `t`, _occludes answers
"not occluded" for the frame when t < ldistance, and goes on into the far child with t_near = t otherwise.  The kernels carry it
in two forms: where the near child is EMPTY, as the line after kd_descend in trace_occluded_var / trace_occluded_var_t
(nt_var.hip) and in the own text of trace_occluded<N> / trace_occluded_t<N> (nt_composite.hpp) -- the *descent exit*; and where
the near child was walked first, as the `t < ldistance` of kd_resume_occluded and of the two fixed-N walkers' pops -- the
*pop rule*.  Rays that start outside the tree with a whole window never take the descent exit (every push is followed by a pop
with the same t, and t only grows along the walk), so the rays here start inside the slab or carry a t_near / t_far window.

Scenes: high_dimension_cases.wide_comb(n, 7, filled) -- six cells along z, the cells not in `filled` missing far children -- with
filled = (0, 1, 3) or (0, 3, 5), materials through test_composite_matrix._scene_flat ("lit": all opaque, "transparent": materials
0 and 2 half transparent), and a `loose` form in which cell 3's batch is stored as four KIND_TRIANGLE items in its leaf (the
cut-off form of the simplex test, and at fixed N the <N,true> kernel).

A *case* is (n, filled, kind, loose, forced): forced is NTRACER_FORCE_VAR=1.  Per case, computed once per process and frozen
(batch): the rays of four sets laid end to end -- I origins inside, in front of and behind the slab, W origins outside with a
window, S second legs from the oracle's hits, E edge rays -- the oracle's answers, and the model's with its census.

The model (walk) is the control of kd_descend and kd_resume_occluded in plain Python with fp32 arithmetic for t; a leaf is
answered by the oracle on a one-leaf scene.  It has the two rules as switches, so the host test can show that the rays tell a
walk without either rule from the right one, and it records what each ray met for the GPU test's failure message."""
import functools
from unittest import mock

import numpy as np

import high_dimension_cases as hd
import ray_query_cases as rq
from ntracer_amd import _lib

f32 = np.float32
FLT_MAX = rq.FLT_MAX
TILT = hd.TILT
TREE = 7                        # wide_comb's stack_depth: five splits, six cells, cell k between z = k / 6 and (k + 1) / 6
CELLS = TREE - 1
LOOSE_CELL = 3                  # in both patterns
PATTERNS = ((0, 1, 3), (0, 3, 5))
KINDS = ("lit", "transparent")
NATIVE_DIMS = (11, 33, 59, 64)
KERNELS = ("query_occluded<N,false>", "query_occluded<N,true>", "query_occluded_t<N>", "query_occluded_var", "query_occluded_var_t")
VAR_KERNELS = KERNELS[3:]
DISTANCES = (0.1, 0.2, 0.3, 0.45, 0.6, 0.9, 1.3, float(FLT_MAX))
N_I, N_W, N_S = 144, 56, 36
TIE = 1e-4                      # no distance within TIE (1 + t) of a t it is compared with
NUDGE = 1.0 + 1.5e-3
MAX_DROPPED = 0.05
# one seed a pattern, so that the first three coordinates of a pattern's rays are the same at every n; 8808 is a seed at which every
# floor of tests/test_occlusion_walk_host.py holds under both patterns and both kinds (the floors are asserted there, case by case)
SEEDS = {(0, 1, 3): 8808, (0, 3, 5): 8808}
OUTCOMES = ("exit at an empty near child", "through an empty near child", "pop skips the far child", "pop resumes the far child")

P1, P2 = PATTERNS
# (n, filled, kind, loose, forced) -> the kernel its occludes_rays reaches
CASES = (
    ((4, P1, "lit", False, False), "query_occluded<N,false>"),
    ((10, P2, "lit", False, False), "query_occluded<N,false>"),
    ((4, P2, "lit", True, False), "query_occluded<N,true>"),
    ((10, P1, "lit", True, False), "query_occluded<N,true>"),
    ((4, P1, "transparent", False, False), "query_occluded_t<N>"),
    ((10, P2, "transparent", True, False), "query_occluded_t<N>"),
    ((5, P1, "lit", False, True), "query_occluded_var"),
    ((10, P2, "lit", False, True), "query_occluded_var"),
    ((11, P1, "lit", False, False), "query_occluded_var"),
    ((33, P2, "lit", True, False), "query_occluded_var"),
    ((59, P1, "lit", False, False), "query_occluded_var"),
    ((64, P2, "lit", False, False), "query_occluded_var"),
    ((64, P1, "lit", True, False), "query_occluded_var"),
    ((5, P2, "transparent", False, True), "query_occluded_var_t"),
    ((10, P1, "transparent", False, True), "query_occluded_var_t"),
    ((11, P2, "transparent", False, False), "query_occluded_var_t"),
    ((33, P1, "transparent", False, False), "query_occluded_var_t"),
    ((59, P2, "transparent", True, False), "query_occluded_var_t"),
    ((64, P1, "transparent", False, False), "query_occluded_var_t"),
    ((64, P2, "transparent", False, False), "query_occluded_var_t"),
)


def case_id(case):
    n, filled, kind, loose, forced = case
    return "n%d-%s-%s%s%s" % (n, "".join(str(c) for c in filled), kind, "-loose" if loose else "", "-var" if forced else "")


def env_of(case):
    return {"NTRACER_FORCE_VAR": "1"} if case[4] else {}


def first_case_of(kernel):
    return next(c for c, k in CASES if k == kernel)


# ------------------------------------------------------------------ scenes
def _loosen(flat, batch):
    """`flat` with batch `batch` taken out of the batch table and stored as four loose triangles in its leaf"""
    f = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in flat.items()}
    f["tri_recs"], f["tri_mats"] = np.array(flat["batch_recs"][batch]), np.array(flat["batch_mats"][batch])
    f["batch_recs"], f["batch_mats"] = np.delete(flat["batch_recs"], batch, axis=0), np.delete(flat["batch_mats"], batch, axis=0)
    items = []
    for node in np.nonzero(flat["node_axis"] < 0)[0]:
        new = []
        for item in flat["items"][flat["node_left"][node]:flat["node_left"][node] + flat["node_right"][node]]:
            kind, idx = int(item) & 3, int(item) >> 2
            assert kind == _lib.KIND_BATCH
            if idx == batch:
                new += [(lane << 2) | _lib.KIND_TRIANGLE for lane in range(4)]
            else:
                new.append(((idx - (idx > batch)) << 2) | _lib.KIND_BATCH)
        f["node_left"][node], f["node_right"][node] = len(items), len(new)
        items += new
    f["items"] = np.asarray(items, np.int32)
    return f


@functools.lru_cache(maxsize=None)
def scene(case):
    """the flat scene of a case, its stack depth and LDS bytes, and the oracle over it in the library's mode"""
    import test_composite_matrix as tcm
    n, filled, kind, loose, forced = case
    assert filled in PATTERNS and kind in KINDS and LOOSE_CELL in filled
    c = hd.Case()
    c.case, c.n = case, n
    base = hd.wide_comb(n, TREE, filled)
    if loose:
        base = _loosen(base, filled.index(LOOSE_CELL))          # (wide_comb numbers the batches in the order of `filled`)
    c.flat = tcm._scene_flat(base, kind)
    c.params = tcm.params(n, kind)
    c.stack_depth = hd.stack_depth_of(c.flat)
    c.lds = hd.lds_bytes(n, c.stack_depth)
    c.prune = len(c.flat["solid_types"]) == 0                   # (the library's rule, as ray_query_cases.batches has it)
    c.oracle = rq.Oracle(n, c.flat, False, c.prune)
    return hd._freeze(c)


def route(case):
    """the kernel occludes_rays of a case lands on: test_ray_queries_host._route, the rule itself, read on this case's scene"""
    import test_ray_queries_host as host
    s = scene(case)
    with mock.patch.object(rq, "scene", lambda name: (None, s.n, s.flat)):
        return host._route(case_id(case), env_of(case), "occludes")


# ------------------------------------------------------------------ the model
class Leaves(object):
    """the leaves of a scene, each answered by the oracle on a scene whose root is that leaf"""

    def __init__(self, n, flat):
        self.n, self.flat = n, flat
        self.occ, self.hit = {}, {}
        opaque = np.array(flat["materials"], f32)
        opaque[:, 6] = 1.0
        for node in np.nonzero(np.asarray(flat["node_axis"]) < 0)[0]:
            f = dict(flat)
            f["root"] = int(node)
            self.occ[int(node)] = rq.Oracle(n, f, False, False)
            g = dict(f)
            g["materials"] = opaque
            self.hit[int(node)] = rq.Oracle(n, g, True, False)

    def occludes(self, node, o, d, distance, skip):
        """(blocked, n_transparent) of kd_leaf::occludes"""
        r = self.occ[node].occludes(o[None], d[None], [distance], [-FLT_MAX], [FLT_MAX], [skip[0]], [skip[1]])
        return bool(r["blocked"][0]), int(r["n_transparent"][0])

    def hit_t(self, node, o, d, skip):
        """t of the leaf's nearest primitive along the ray, whatever its material, or None"""
        r = self.hit[node].intersects(o[None], d[None], [-FLT_MAX], [FLT_MAX], [skip[0]], [skip[1]])
        return float(r["dist"][0]) if r["item"][0] >= 0 else None


class Walk(object):
    """what one ray's walk answered and met: blocked, n_transparent (of the leaves it tested), which OUTCOMES it took, the t of
    every split it compared with the distance (crossed) and of every leaf's nearest primitive (hits)"""
    __slots__ = ("blocked", "n_transparent", "took", "crossed", "hits")


def walk(flat, leaves, o, d, distance, t_near, t_far, skip, descent_exit=True, pop_rule=True):
    """_occludes (tracer.hpp:1258-1307) in the kernels' form: kd_descend's branch step on a stack of continuations, the caller's
    exit after a step that `crossed`, kd_resume_occluded's pops.  fp32 for t = (split - o) * (1 / d); the o == split tie goes by
    the direction's sign; a zero direction component goes right when o >= split."""
    axis, split, left, right = flat["node_axis"], flat["node_split"], flat["node_left"], flat["node_right"]
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    distance, t_near, t_far_root = f32(distance), f32(t_near), f32(t_far)
    w = Walk()
    w.blocked, w.n_transparent, w.took, w.crossed, w.hits = False, 0, [False] * 4, [], []
    node, stack, t_far = int(flat["root"]), [], t_far_root
    while True:
        while node >= 0:
            a = int(axis[node])
            if a < 0:
                ht = leaves.hit_t(node, o, d, skip)
                if ht is not None:
                    w.hits.append(ht)
                blocked, nt = leaves.occludes(node, o, d, distance, skip)
                w.n_transparent += nt
                if blocked:
                    w.blocked = True
                    return w
                node = -1
                break
            oa, da, s = o[a], d[a], f32(split[node])
            lo, hi = int(left[node]), int(right[node])
            if da != 0:
                if oa == s:
                    node = hi if da > 0 else lo
                    continue
                with np.errstate(over="ignore"):
                    t = f32(f32(s - oa) * f32(f32(1) / da))
                near, far = (hi, lo) if oa > s else (lo, hi)
                if t < 0 or t > t_far:
                    node = near
                elif t < t_near:
                    node = far
                elif near >= 0:
                    stack.append((t, far))
                    t_far = t
                    node = near
                else:                                   # crossed: no near child
                    w.crossed.append(float(t))
                    if descent_exit and t < distance:
                        w.took[0] = True
                        node = -1
                        break
                    w.took[1] = True
                    node, t_near = far, t
                continue
            node = hi if oa >= s else lo
        while True:                                     # the frame has returned false
            if not stack:
                return w
            t, far = stack.pop()
            if far < 0:
                continue
            w.crossed.append(float(t))
            if pop_rule and t < distance:
                w.took[2] = True
                continue
            w.took[3] = True
            node, t_near = far, t
            t_far = stack[-1][0] if stack else t_far_root
            break


# ------------------------------------------------------------------ rays
def _unit(v):
    return (v / np.sqrt((v * v).sum(axis=1, dtype=f32))[:, None]).astype(f32)


def _tilt(n, origins, directions, first=0):
    """for n >= 11 every hidden coordinate of every origin is +-TILT and of every direction -+TILT, the signs alternating along
    the coordinates and from ray to ray (high_dimension_cases.tilted); below, the hidden coordinates are zero"""
    if n >= 11:
        count = len(origins)
        sign = np.where((np.arange(n - 3)[None, :] + first + np.arange(count)[:, None]) % 2 == 0, 1.0, -1.0)
        origins[:, 3:] = (TILT * sign).astype(f32)
        directions[:, 3:] = (-TILT * sign).astype(f32)


def _edge_rays(flat):
    """set E: (origin xyz, direction xyz, distance) rows"""
    zb = [float(s) for s in sorted(set(np.asarray(flat["node_split"])[np.asarray(flat["node_axis"]) >= 0]))]
    width = 1.0 / CELLS
    rows = []
    for k, (cell, dist) in enumerate(((0, 0.6), (3, FLT_MAX), (2, 0.3), (4, FLT_MAX))):    # filled, filled, empty, empty: direction[2] == 0
        rows.append(((-0.5, 0.05 * k, (cell + 0.25) * width), (1.0, 0.1, 0.0), dist))
    for k, (s, dist) in enumerate(((zb[0], 0.45), (zb[2], FLT_MAX), (zb[4], 0.9))):        # direction[2] == 0 on a split: goes right
        rows.append(((-0.5, 0.02 * k, s), (1.0, -0.1, 0.0), dist))
    for k, s in enumerate(zb):                                                            # the origin on a split, both ways
        for sign in (1.0, -1.0):
            rows.append(((0.1 - 0.04 * k, 0.08, s), (0.05, -0.03 * sign, sign), FLT_MAX if (k + (sign > 0)) % 2 else 0.3))
    return rows


class Batch(object):
    pass


def _ties(w, distance):
    return distance < FLT_MAX and any(abs(float(distance) - t) <= TIE * (1.0 + abs(t)) for t in w.crossed + w.hits)


@functools.lru_cache(maxsize=None)
def batch(case):
    s = scene(case)
    n, flat, orc = s.n, s.flat, s.oracle
    filled = case[1]
    rng = np.random.default_rng(SEEDS[filled])                  # (the first three coordinates are a pattern's, whatever n)
    leaves = Leaves(n, flat)
    table = np.asarray(DISTANCES, f32)

    def rays(xyz_o, xyz_d, first):
        o, d = np.zeros((len(xyz_o), n), f32), np.zeros((len(xyz_o), n), f32)
        o[:, :3], d[:, :3] = xyz_o, xyz_d
        _tilt(n, o, d, first)
        return o, _unit(d)

    whole = lambda k: (np.full(k, -FLT_MAX, f32), np.full(k, FLT_MAX, f32))
    none = lambda k: np.full(k, -1, np.int32)
    # ---- I: origins inside, in front of and behind the slab; whole window
    oz = rng.uniform(-0.3, 1.3, N_I)
    up = np.arange(N_I) % 2 == 0
    o_i, d_i = rays(np.stack([rng.uniform(-0.3, 0.3, N_I), rng.uniform(-0.3, 0.3, N_I), oz], axis=1),
                    np.stack([rng.uniform(-0.15, 0.15, N_I), rng.uniform(-0.15, 0.15, N_I), np.where(up, 1.0, -1.0)], axis=1), 0)
    dist_i = rng.choice(table, N_I).astype(f32)
    tn_i, tf_i = whole(N_I)
    first_hit = orc.intersects(o_i, d_i, tn_i, tf_i, none(N_I), none(N_I))
    tied = np.nonzero((np.arange(N_I) % 4 == 3) & (first_hit["item"] >= 0))[0]
    factor = np.where(np.arange(len(tied)) % 2 == 0, f32(1 - 1e-3), f32(1 + 1e-3)).astype(f32)
    dist_i[tied] = (first_hit["dist"][tied] * factor).astype(f32)
    # ---- W: origins outside, half with a t_near window, half with a t_far window
    up_w = np.arange(N_W) % 2 == 0
    o_w, d_w = rays(np.stack([rng.uniform(-0.3, 0.3, N_W), rng.uniform(-0.3, 0.3, N_W), np.where(up_w, -0.4, 1.4)], axis=1),
                    np.stack([rng.uniform(-0.15, 0.15, N_W), rng.uniform(-0.15, 0.15, N_W), np.where(up_w, 1.0, -1.0)], axis=1), N_I)
    near_w = (np.arange(N_W) // 2) % 2 == 0
    tn_w = np.where(near_w, rng.uniform(0.1, 0.9, N_W), -FLT_MAX).astype(f32)
    tf_w = np.where(near_w, FLT_MAX, rng.uniform(0.3, 1.2, N_W)).astype(f32)
    dist_w = rng.choice(table, N_W).astype(f32)
    # ---- S: second legs from the oracle's hits of set I, the hit skipped, half of them reversed; those with a next hit first
    src = np.nonzero(first_hit["item"] >= 0)[0]
    at = (o_i[src] + first_hit["dist"][src, None] * d_i[src]).astype(f32)
    back = np.arange(len(src)) % 2 == 1
    o_s, d_s = rays(at[:, :3], np.where(back[:, None], -d_i[src, :3], d_i[src, :3]), N_I + N_W)
    si, sl = first_hit["item"][src].astype(np.int32), first_hit["lane"][src].astype(np.int32)
    tn_s, tf_s = whole(len(src))
    nxt = orc.intersects(o_s, d_s, tn_s, tf_s, si, sl)
    order = np.argsort(nxt["item"] < 0, kind="stable")[:N_S]
    o_s, d_s, si, sl, tn_s, tf_s = o_s[order], d_s[order], si[order], sl[order], tn_s[order], tf_s[order]
    has_next = nxt["item"][order] >= 0
    inside = np.arange(len(order)) % 2 == 0
    # (by the quirk a whole-window ray is blocked by the first leaf it reaches alone, and a second leg's first leaf holds only the
    # plane it left: so that a next hit can block at all, two of three legs that have one skip the cells before it with a t_near of
    # 0.9 of its distance -- every split between two filled cells' planes lies at 5 / 6 of the way or nearer)
    windowed = has_next & (np.arange(len(order)) % 3 != 2)
    tn_s = np.where(windowed, nxt["dist"][order] * f32(0.9), tn_s).astype(f32)
    next_t = np.where(has_next, nxt["dist"][order], f32(1)).astype(f32)
    dist_s = np.where(has_next, next_t * np.where(inside, f32(1 + 1e-3), f32(1 - 1e-3)), rng.choice(table, len(order))).astype(f32)
    lo_s = np.where(has_next, next_t * f32(1 - 1e-3), dist_s).astype(f32)
    hi_s = np.where(has_next, next_t * f32(1 + 1e-3), dist_s).astype(f32)
    # ---- E
    rows = _edge_rays(flat)
    o_e, d_e = rays(np.array([r[0] for r in rows], f32), np.array([r[1] for r in rows], f32), N_I + N_W + len(order))
    for k, r in enumerate(rows):
        o_e[k, 2] = f32(r[0][2])
        assert (d_e[k, 2] == 0) == (r[1][2] == 0)
    dist_e = np.array([r[2] for r in rows], f32)
    tn_e, tf_e = whole(len(rows))

    b = Batch()
    b.case = case
    sets = np.array(["I"] * N_I + ["W"] * N_W + ["S"] * len(order) + ["E"] * len(rows))
    origins, directions = np.concatenate([o_i, o_w, o_s, o_e]), np.concatenate([d_i, d_w, d_s, d_e])
    distance = np.concatenate([dist_i, dist_w, dist_s, dist_e]).astype(f32)
    t_near, t_far = np.concatenate([tn_i, tn_w, tn_s, tn_e]), np.concatenate([tf_i, tf_w, tf_s, tf_e])
    skip_item, skip_lane = np.concatenate([none(N_I + N_W), si, none(len(rows))]), np.concatenate([none(N_I + N_W), sl, none(len(rows))])
    if n >= 11:
        zero = directions == 0
        assert (origins[:, 3:] != 0).all() and zero[:, :2].sum() == 0 and zero[:, 3:].sum() == 0 and zero[sets != "E"].sum() == 0

    # ---- no distance ties with a t it is compared with: nudge the drawn distances, drop the rays that stay tied
    fixed = np.zeros(len(sets), bool)
    fixed[tied] = True
    fixed[sets == "S"] = has_next
    keep = np.ones(len(sets), bool)
    walks = [None] * len(sets)
    modes = ((True, True), (False, True), (True, False))
    for r in range(len(sets)):
        for attempt in range(4):
            args = (flat, leaves, origins[r], directions[r], distance[r], t_near[r], t_far[r], (int(skip_item[r]), int(skip_lane[r])))
            ws = [walk(*args, descent_exit=de, pop_rule=pr) for de, pr in modes]
            if not any(_ties(w, distance[r]) for w in ws):
                walks[r] = ws
                break
            if fixed[r]:
                break
            distance[r] = f32(distance[r] * f32(NUDGE))
        keep[r] = walks[r] is not None
    b.dropped = int((~keep).sum())
    b.total = len(sets)
    walks = [w for w in walks if w is not None]
    pick = lambda a: np.ascontiguousarray(a[keep])
    b.sets, b.origins, b.directions, b.distance = pick(sets), pick(origins), pick(directions), pick(distance)
    b.t_near, b.t_far, b.skip_item, b.skip_lane = pick(t_near), pick(t_far), pick(skip_item), pick(skip_lane)
    b.count = len(b.sets)
    # ---- the oracle's answers: the batch as it is, and with every distance FLT_MAX and no window
    b.ref = orc.occludes(b.origins, b.directions, b.distance, b.t_near, b.t_far, b.skip_item, b.skip_lane)
    b.far, (b.no_near, b.no_far) = np.full(b.count, FLT_MAX, f32), whole(b.count)
    b.ref_far = orc.occludes(b.origins, b.directions, b.far, b.no_near, b.no_far, b.skip_item, b.skip_lane)
    # ---- set S: the verdict just inside against just outside the next hit
    s_keep = keep[sets == "S"]
    so, sd, ssi, ssl = (pick(a)[b.sets == "S"] for a in (origins, directions, skip_item, skip_lane))
    a_lo = orc.occludes(so, sd, lo_s[s_keep], tn_s[s_keep], tf_s[s_keep], ssi, ssl)["blocked"]
    a_hi = orc.occludes(so, sd, hi_s[s_keep], tn_s[s_keep], tf_s[s_keep], ssi, ssl)["blocked"]
    b.s_flips = int((a_lo != a_hi).sum())
    # ---- the model: both rules, without the descent exit, without the pop rule
    b.model = {name: dict(blocked=np.array([w[k].blocked for w in walks]), n_transparent=np.array([w[k].n_transparent for w in walks], np.int32))
               for k, name in enumerate(("both", "no_descent_exit", "no_pop_rule"))}
    b.took = np.array([w[0].took for w in walks], bool).reshape(b.count, 4)
    b.crossed = tuple(tuple(w[0].crossed) for w in walks)
    b.hits = tuple(tuple(w[0].hits) for w in walks)
    for d in [b.ref, b.ref_far] + list(b.model.values()):
        for v in d.values():
            v.setflags(write=False)
    return hd._freeze(b)


def describe(case, r):
    """what the model's walk of ray `r` met, for a failure message"""
    b = batch(case)
    took = [OUTCOMES[k] for k in range(4) if b.took[r, k]] or ["no split compared with the distance"]
    return "ray %d of set %s: %s; distance %r, window (%r, %r), skip (%d, %d), split t %s, leaf hit t %s; oracle blocked %s, n_transparent %d" % (
        r, b.sets[r], ", ".join(took), float(b.distance[r]), float(b.t_near[r]), float(b.t_far[r]), int(b.skip_item[r]), int(b.skip_lane[r]),
        list(b.crossed[r]), list(b.hits[r]), bool(b.ref["blocked"][r]), int(b.ref["n_transparent"][r]))


def census(case):
    """per case, for the host test's report: rays, dropped, rays taking each outcome, rays on which each mutant differs"""
    b = batch(case)
    ref = b.ref["blocked"]
    differs = lambda m: int(((m["blocked"] != ref) | (m["n_transparent"] != b.ref["n_transparent"])).sum())
    return dict(rays=b.count, dropped=b.dropped, outcomes=[int(x) for x in b.took.sum(axis=0)],
                no_descent_exit=differs(b.model["no_descent_exit"]), no_pop_rule=differs(b.model["no_pop_rule"]),
                blocked=int(ref.sum()), transparent=int((b.ref["n_transparent"] > 0).sum()), s_flips=b.s_flips)
