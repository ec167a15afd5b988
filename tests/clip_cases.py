"""Expected results under clip planes, shared by tests/test_clip_host.py and tests/test_clip_gpu.py.  Nothing here comes from
the library: every reference is the oracle, or a numpy restatement pinned to the oracle by the host test.

Reference A -- planes that cut through primitives, opaque scenes made of batches and loose triangles.  `brute` is a
sequential-fp32 numpy brute force over all simplex records of a scene for every pixel of a view: simplex_batch_form /
simplex_scalar_form of ntracer_amd/csrc/nt_composite.hpp restated operation by operation (t = -(N.o + d) / (N.d), the edge tests
with NT_FUZZ), the window rule of include/ntracer_hip.h restated likewise, and the closest accepted t.  With no planes it must
give primary_hit_cases.expected's dist bit for bit on every pixel (test_clip_host.py); it holds for opaque scenes only.  A
pixel with a candidate within 1e-4 (1 + |bound|) of its t0 or t1 is `near`: only those may be left out of a comparison.
The planes come from the oracle's own records: with a = -(forward + 0.3 tilt) of the view's camera (tilt: its `right` row), the
offsets are quantiles of a . x over the plain hit points x.  `median`: one plane at the 0.5 quantile, which takes the near half
of what is seen away; `slab`: that plane and -a . x <= -q(0.2), so every ray has a finite t1; `eight`: the median plane and seven
planes that take little more away, across the view and along three other tilts, so that the far side stays.
The colour of an unlit scene's pixel depends only on its own simplex and d: `simplex_colors` asks the oracle for the colour of
the same ray in a scene that holds that simplex alone (ray_color_cases.CentrePixel), the background where nothing is hit.

Reference B -- whole primitives, every feature.  `twin` is a golden scene A with a copy B translated along axis 0 beyond A's
box, the two trees grafted under one root branch on axis 0, and the plane x_0 <= split between them.  The expected records and
frames are the oracle's on the same tree with B's leaves emptied: splits and box are then identical, so every quirk of the
walks is the same.  Variants as ray_color_cases makes them ("" unlit, "lit", "reflective") and "glass": "lit" with every third
simplex's material at opacity 0.5.  The lit variants get one global light more, shining from B towards A, so that B would
shadow A, and a point light beyond the plane is mirrored to A's far side.  Two cameras of its own: 0 sees A and B side by side;
1 stands beyond B, in the half-space that is cut away, and looks back through B at the side of A that mirrors B: its primary
walks start at t0 > 0.

Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import oracle_binding as ob
import primary_hit_cases as ph
import ray_color_cases as rc
import ray_query_cases as rq

f32 = np.float32
FLT_MAX = rq.FLT_MAX
FUZZ = f32(f32(1.1920928955078125e-07) * f32(10.0))
ONE_FUZZ = f32(f32(1.0) + FUZZ)
CLIP_MAX = 8

# Reference A: the scenes, the views and the plane sets
SCENES_A = ["cell120_n4", "cell600_n4", "orthoplex5_n5", "simplex7_n7", "simplex10_n10"]
PINNED = ["cell120_n4", "cell600_n4", "simplex7_n7", "simplex10_n10"]
W, H = 37, 21
SIZES = [(1, 1), (8, 8), (9, 7), (37, 21)]
CAMERAS = (0, 1)
KINDS = ("median", "slab", "eight")
NEAR_CAP = 0.02                     # share of a view's pixels that may be `near`
MIN_MOVED = MIN_UNCHANGED = MIN_LOST = 5

# Reference B
TWINS = [("cell600_n4", ""), ("cell600_n4", "lit"), ("cell600_n4", "reflective"), ("cell600_n4", "glass"), ("cell600_n4", "glass-split"),
         ("orthoplex5_n5", "lit"), ("simplex7_n7", "lit"), ("simplex10_n10", "lit")]
TWIN_CAMERAS = (0, 1)
MIN_TWIN_DIFF = 5                   # pixels of the twin's frame that B changes, by the oracle alone


def twin_id(t):
    return t[0] + ("," + t[1] if t[1] else "")


# ------------------------------------------------------------------ the window rule
def window(planes, o, d):
    """(t0, t1, empty) [count] of rays d [count][n] from the origin o [n] (or origins [count][n]) under planes = (normals
    [K][n], offsets [K]): the rule of include/ntracer_hip.h, every operation rounded to fp32 on its own"""
    normals, offsets = planes
    d = np.asarray(d, f32)
    o = np.broadcast_to(np.asarray(o, f32), d.shape)
    count, n = d.shape
    t0 = np.zeros(count, f32)
    t1 = np.full(count, FLT_MAX, f32)
    empty = np.zeros(count, bool)
    with np.errstate(all="ignore"):
        for a, b in zip(np.asarray(normals, f32).reshape(-1, n), np.asarray(offsets, f32).reshape(-1)):
            p = (a[0] * o[:, 0]).astype(f32)
            r = (a[0] * d[:, 0]).astype(f32)
            for j in range(1, n):
                p = (p + (a[j] * o[:, j]).astype(f32)).astype(f32)
                r = (r + (a[j] * d[:, j]).astype(f32)).astype(f32)
            s = (p - b).astype(f32)
            q = ((-s) / r).astype(f32)
            t1 = np.where((r > 0) & (q < t1), q, t1).astype(f32)
            t0 = np.where((r < 0) & (q > t0), q, t0).astype(f32)
            empty |= (r == 0) & (s > 0)
    empty |= t0 > t1
    return t0, t1, empty


NO_PLANES = (np.zeros((0, 1), f32), np.zeros(0, f32))


# ------------------------------------------------------------------ Reference A
@functools.lru_cache(maxsize=None)
def records(name):
    """(recs [R][rl], item [R], lane [R], scalar [R]) of every simplex of an opaque golden scene, batches first"""
    g, n, flat = rq.scene(name)
    return records_of(n, flat)


def records_of(n, flat):
    assert len(flat["solid_types"]) == 0 and (np.asarray(flat["materials"])[:, 6] >= 1).all()
    br = np.asarray(flat["batch_recs"], f32).reshape(-1, 4, n * n + n + 1)
    tr = np.asarray(flat["tri_recs"], f32).reshape(-1, n * n + n + 1)
    recs = np.concatenate([br.reshape(-1, br.shape[2]), tr])
    item = np.concatenate([np.repeat(np.arange(len(br), dtype=np.int32) << 2, 4), (np.arange(len(tr), dtype=np.int32) << 2) | 1])
    lane = np.concatenate([np.tile(np.arange(4, dtype=np.int32), len(br)), np.full(len(tr), -1, np.int32)])
    scalar = np.concatenate([np.zeros(4 * len(br), bool), np.ones(len(tr), bool)])
    for v in (recs, item, lane, scalar):
        v.setflags(write=False)
    return recs, item, lane, scalar


def _candidates(recs, scalar, n, o, d):
    """t [R][P] fp32 of every simplex for every ray, 0 where its own test rejects the ray (no cutoff: a brute force keeps the
    closest)"""
    R, P = len(recs), len(d)
    with np.errstate(all="ignore"):
        nrm = recs[:, 1:1 + n]
        denom = (nrm[:, 0:1] * d[None, :, 0]).astype(f32)
        no = np.broadcast_to((nrm[:, 0] * o[0]).astype(f32)[:, None], (R, 1))
        for k in range(1, n):
            denom = (denom + (nrm[:, k:k + 1] * d[None, :, k]).astype(f32)).astype(f32)
            no = (no + (nrm[:, k] * o[k]).astype(f32)[:, None]).astype(f32)
        t = ((-(no + recs[:, 0:1]).astype(f32)) / denom).astype(f32)
        sc = scalar[:, None]
        ok = np.where(sc, (denom != 0) & (t > 0), (denom != 0) & (t >= 0))
        pside = [(recs[:, 1 + n + k][:, None] - (o[k] + (t * d[None, :, k]).astype(f32)).astype(f32)).astype(f32) for k in range(n)]
        tot = np.zeros((R, P), f32)
        for e in range(n - 1):
            en = recs[:, 1 + 2 * n + e * n:1 + 2 * n + (e + 1) * n]
            area = (en[:, 0:1] * pside[0]).astype(f32)
            for k in range(1, n):
                area = (area + (en[:, k:k + 1] * pside[k]).astype(f32)).astype(f32)
            ok &= np.where(sc, ~((area < -FUZZ) | (area > ONE_FUZZ)), area >= -FUZZ)
            tot = (tot + area).astype(f32)
        ok &= tot <= ONE_FUZZ
        return np.where(ok & (t != 0), t, f32(0)).astype(f32)


@functools.lru_cache(maxsize=None)
def _brute_t(name, width, height, k):
    recs, item, lane, scalar = records(name)
    n = rq.scene(name)[1]
    d, _ = ph.rays(name, width, height, k)
    o = ph.camera(name, k)[0]
    t = _candidates(recs, scalar, n, o, d.reshape(-1, n))
    t.setflags(write=False)
    return t


def _near(t, bound):
    with np.errstate(all="ignore"):
        return np.abs(t - bound) <= f32(1e-4) * (f32(1) + np.abs(bound))


def brute(name, width, height, k, planes):
    """dist, item, lane [H][W] of the closest candidate the planes accept; unique [H][W]: one record alone reaches that dist;
    near [H][W]: some candidate lies within 1e-4 (1 + |bound|) of the ray's t0 or t1"""
    d, aabb = ph.rays(name, width, height, k)
    return brute_rays(records(name), rq.scene(name)[1], ph.camera(name, k)[0], d, aabb, planes, _brute_t(name, width, height, k))


def brute_rays(recs4, n, o, d, aabb, planes, t=None):
    """brute for any opaque scene: its records_of, the origin o, directions d [H][W][n] and their aabb_distance [H][W]"""
    recs, item, lane, scalar = recs4
    height, width = aabb.shape
    if t is None:
        t = _candidates(recs, scalar, n, o, d.reshape(-1, n))
    t0, t1, empty = window(planes, o, d.reshape(-1, n))
    enters = aabb.ravel() >= 0
    cand = t != 0
    ok = cand & ~empty[None] & enters[None] & (t >= t0[None]) & (t <= t1[None])
    tt = np.where(ok, t, f32(FLT_MAX)).astype(f32)
    best = tt.argmin(axis=0)
    dist = tt.min(axis=0)
    hit = dist < FLT_MAX
    out = dict(dist=np.where(hit, dist, f32(FLT_MAX)).astype(f32), item=np.where(hit, item[best], -1).astype(np.int32),
               lane=np.where(hit, lane[best], -1).astype(np.int32), unique=(tt == dist[None]).sum(axis=0) == 1,
               near=(cand & enters[None] & ~empty[None] & (_near(t, t0[None]) | (_near(t, t1[None]) & (t1 < FLT_MAX)[None]))).any(axis=0))
    out["unique"] &= hit
    res = {key: v.reshape(height, width) for key, v in out.items()}
    for v in res.values():
        v.setflags(write=False)
    return res


def _axes_normal(axes, row, sign=1.0):
    return (-(axes[2] + f32(0.3 * sign) * axes[row])).astype(f32)


@functools.lru_cache(maxsize=None)
def planes(name, kind, k=0):
    """(normals [K][n], offsets [K]) fp32 of a plane set for the view of camera k, from the oracle's records at 37 x 21"""
    n = rq.scene(name)[1]
    o, axes = ph.camera(name, k)
    e = ph.expected((name, {}), W, H, k)
    d = ph.rays(name, W, H, k)[0]
    hit = e["item"] >= 0
    x = o[None].astype(np.float64) + e["dist"][hit].astype(np.float64)[:, None] * d[hit].astype(np.float64)

    def q(a, quantile):
        return f32(np.quantile(x @ a.astype(np.float64), quantile))

    a = _axes_normal(axes, 0)
    normals, offsets = [a], [q(a, 0.5)]
    if kind == "slab":
        normals.append((-a).astype(f32))
        offsets.append(f32(-q(a, 0.2)))
    if kind == "eight":
        # the median plane, and seven planes that take little away, so that the far side stays: the outermost fiftieth of the
        # hit points to the right, to the left, above and below, and the nearest tenth along three other tilts (most of which
        # the median plane has taken already)
        for j, (row, sign) in enumerate(((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0))):
            aj = (f32(sign * (1.0 + 0.5 * j)) * axes[row]).astype(f32)       # (normals need not be unit vectors)
            normals.append(aj)
            offsets.append(q(aj, 0.98))
        for row, sign in ((1, 1.0), (1, -1.0), (0, -1.0)):
            aj = _axes_normal(axes, row, sign)
            normals.append(aj)
            offsets.append(q(aj, 0.9))
    assert kind in KINDS and len(normals) == {"median": 1, "slab": 2, "eight": 8}[kind]
    out = np.asarray(normals, f32), np.asarray(offsets, f32)
    for v in out:
        v.setflags(write=False)
    return out


def keep_all(name):
    """2 n planes that keep the whole scene box with room to spare: the plain render, byte for byte"""
    g, n, flat = rq.scene(name)
    lo, hi = np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32)
    normals, offsets = [], []
    for j in range(min(n, CLIP_MAX // 2)):
        for s in (1.0, -1.0):
            a = np.zeros(n, f32)
            a[j] = s
            normals.append(a)
            offsets.append(f32((hi[j] if s > 0 else -lo[j]) + 2.0 * (hi[j] - lo[j])))
    return np.asarray(normals, f32), np.asarray(offsets, f32)


def keep_nothing(name):
    """two planes whose keep-regions do not meet"""
    n = rq.scene(name)[1]
    a = np.zeros(n, f32)
    a[0] = 1
    return np.asarray([a, -a], f32), np.asarray([-1000.0, -1000.0], f32)


def census(name, kind, k):
    """(moved, unchanged, lost, near) pixels of the 37 x 21 view: hit pixels of the plain view that show another surface,
    the same one, or nothing under the planes -- all by the reference alone"""
    plain = brute(name, W, H, k, NO_PLANES)
    cut = brute(name, W, H, k, planes(name, kind, k))
    was = plain["item"] >= 0
    now = cut["item"] >= 0
    same = was & now & (cut["dist"].view(np.uint32) == plain["dist"].view(np.uint32))
    return int((was & now & ~same).sum()), int(same.sum()), int((was & ~now).sum()), int(cut["near"].sum())


@functools.lru_cache(maxsize=None)
def _single(name, item, lane):
    """the oracle's scene that holds one simplex of `name` alone, under the scene's own box and parameters"""
    g, n, flat = rq.scene(name)
    rl = n * n + n + 1
    f = dict(flat)
    if item & 3 == 0:
        rec = np.asarray(flat["batch_recs"], f32).reshape(-1, 4, rl)[item >> 2, lane]
        mat = int(np.asarray(flat["batch_mats"]).reshape(-1, 4)[item >> 2, lane])
        f.update(batch_recs=np.ascontiguousarray(np.repeat(rec[None, None], 4, axis=1)), batch_mats=np.full((1, 4), mat, np.int32),
                 tri_recs=np.zeros((0, rl), f32), tri_mats=np.zeros(0, np.int32), items=np.asarray([0], np.int32))
    else:
        rec = np.asarray(flat["tri_recs"], f32).reshape(-1, rl)[item >> 2]
        mat = int(np.asarray(flat["tri_mats"])[item >> 2])
        f.update(batch_recs=np.zeros((0, 4, rl), f32), batch_mats=np.zeros((0, 4), np.int32), tri_recs=np.ascontiguousarray(rec[None]),
                 tri_mats=np.asarray([mat], np.int32), items=np.asarray([1], np.int32))
    f.update(root=0, node_axis=np.asarray([-1], np.int32), node_split=np.zeros(1, f32), node_left=np.zeros(1, np.int32),
             node_right=np.ones(1, np.int32))
    import fixtures as fx
    return rc.CentrePixel(n, f, fx.params_of(g))


def simplex_colors(name, width, height, k, rec):
    """colours [H][W][3] fp32 of an unlit scene's view whose pixels show the simplices rec["item"] / rec["lane"] (< 0: nothing):
    the oracle's colour of each pixel's own ray in a scene of that simplex alone, its background where nothing is hit"""
    g, n, flat = rq.scene(name)
    import fixtures as fx
    o, axes = ph.camera(name, k)
    ys, xs = np.mgrid[0:height, 0:width]
    v = rc.camera_rays(axes, xs.ravel(), ys.ravel(), width, height, ph.fov_of(name))
    out = np.zeros((height * width, 3), f32)
    items, lanes = rec["item"].ravel(), rec["lane"].ravel()
    empty = dict(flat)
    rl = n * n + n + 1
    empty.update(batch_recs=np.zeros((0, 4, rl), f32), batch_mats=np.zeros((0, 4), np.int32), tri_recs=np.zeros((0, rl), f32),
                 tri_mats=np.zeros(0, np.int32), items=np.zeros(1, np.int32), root=0, node_axis=np.asarray([-1], np.int32),
                 node_split=np.zeros(1, f32), node_left=np.zeros(1, np.int32), node_right=np.zeros(1, np.int32))
    for it, ln in sorted(set(zip(items.tolist(), lanes.tolist()))):
        sel = np.nonzero((items == it) & (lanes == ln))[0]
        orc = rc.CentrePixel(n, empty, fx.params_of(g)) if it < 0 else _single(name, it, ln)
        out[sel] = orc.colors(o, v[sel])
    return out.reshape(height, width, 3)


# ------------------------------------------------------------------ Reference A above ten dimensions
HIGH = [(17, 4), (64, 4)]                       # (n, stack depth) of the wide combs of high_dimension_cases: the run-time-n kernels


@functools.lru_cache(maxsize=None)
def high(n, depth):
    """an unlit wide comb of high_dimension_cases from its own camera: (scene, d [H][W][n], aabb [H][W], one plane, plain
    and cut records by the brute force)"""
    import high_dimension_cases as hd
    s = hd.scene(("wide", n, depth, "unlit", False))
    w, h = hd.VIEW
    d = np.zeros((h, w, n), f32)
    for y in range(h):
        for x in range(w):
            d[y, x] = s.osc.primary_dir(x, y, w, h)
    o, axes = np.asarray(s.origin, f32), np.asarray(s.axes, f32)
    aabb = ph.aabb_distance(np.asarray(s.flat["aabb_start"], f32), np.asarray(s.flat["aabb_end"], f32), o, d.reshape(-1, n)).reshape(h, w)
    recs4 = records_of(n, s.flat)
    t = _candidates(recs4[0], recs4[3], n, o, d.reshape(-1, n))
    plain = brute_rays(recs4, n, o, d, aabb, NO_PLANES, t)
    hit = plain["item"] >= 0
    x = o[None].astype(np.float64) + plain["dist"][hit].astype(np.float64)[:, None] * d[hit].astype(np.float64)
    a = _axes_normal(axes, 0)
    # (the comb's simplices lie in a few planes across the view: the 0.3 quantile falls between two of them, where the median
    # falls on one and makes a fortieth of the view's pixels `near`)
    plane = (a[None].copy(), np.asarray([np.quantile(x @ a.astype(np.float64), 0.3)], f32))
    cut = brute_rays(recs4, n, o, d, aabb, plane, t)
    for v in (d, aabb) + plane:
        v.setflags(write=False)
    return s, d, aabb, plane, plain, cut


# ------------------------------------------------------------------ Reference B
def _translated(recs, n, shift):
    """simplex records moved by `shift` along axis 0: p1 moves, and d = -(N . p1) follows"""
    r = np.array(recs, f32).copy()
    r[..., 0] = (r[..., 0].astype(np.float64) - r[..., 1].astype(np.float64) * shift).astype(f32)
    r[..., 1 + n] = (r[..., 1 + n].astype(np.float64) + shift).astype(f32)
    return r


@functools.lru_cache(maxsize=None)
def twin(name, variant):
    """(n, flat of A and B grafted, flat with B's leaves emptied, params, (normals, offsets) of the plane, cameras)"""
    base = "lit" if variant in ("glass", "glass-split") else variant
    n, flat, params = rc.case_scene((name, {}, base))
    assert len(flat["solid_types"]) == 0
    flat, params = dict(flat), dict(params)
    lo, hi = np.asarray(flat["aabb_start"], np.float64), np.asarray(flat["aabb_end"], np.float64)
    ctr, ext = 0.5 * (lo + hi), 0.5 * (hi - lo)
    shift = float(2.5 * ext[0])
    split = f32(ctr[0] + 1.25 * ext[0])
    rl = n * n + n + 1
    br = np.asarray(flat["batch_recs"], f32).reshape(-1, 4, rl)
    tr = np.asarray(flat["tri_recs"], f32).reshape(-1, rl)
    bm = np.asarray(flat["batch_mats"], np.int32).reshape(-1, 4)
    tm = np.asarray(flat["tri_mats"], np.int32)
    mats = np.asarray(flat["materials"], f32)
    if variant in ("glass", "glass-split"):
        glass = mats.copy()
        glass[:, 6] = 0.5
        bm = np.where((np.arange(bm.size).reshape(bm.shape) % 3) == 0, bm + len(mats), bm).astype(np.int32)
        tm = np.where((np.arange(len(tm)) % 3) == 0, tm + len(mats), tm).astype(np.int32)
        mats = np.concatenate([mats, glass])
    items = np.asarray(flat["items"], np.int32)
    kind = items & 3
    items_b = np.where(kind == 0, ((items >> 2) + len(br)) << 2, (((items >> 2) + len(tr)) << 2) | 1).astype(np.int32)
    axis, left, right = (np.asarray(flat[key], np.int32) for key in ("node_axis", "node_left", "node_right"))
    nn = len(axis)
    leaf = axis < 0
    child = lambda c: np.where(c >= 0, c + nn, c)                          # noqa: E731
    left_b = np.where(leaf, left + len(items), child(left)).astype(np.int32)
    right_b = np.where(leaf, right, child(right)).astype(np.int32)
    lo2, hi2 = lo.copy(), hi.copy()
    hi2[0] = hi[0] + shift
    both = dict(flat)
    both.update(batch_recs=np.concatenate([br, _translated(br, n, shift)]), batch_mats=np.concatenate([bm, bm]),
                tri_recs=np.concatenate([tr, _translated(tr, n, shift)]), tri_mats=np.concatenate([tm, tm]), materials=mats,
                items=np.concatenate([items, items_b]), node_axis=np.concatenate([axis, axis, [0]]).astype(np.int32),
                node_split=np.concatenate([np.asarray(flat["node_split"], f32), (np.asarray(flat["node_split"], np.float64) +
                                           np.where(axis == 0, shift, 0.0)).astype(f32), [split]]).astype(f32),
                node_left=np.concatenate([left, left_b, [int(flat["root"])]]).astype(np.int32),
                node_right=np.concatenate([right, right_b, [int(flat["root"]) + nn]]).astype(np.int32), root=2 * nn,
                aabb_start=lo2.astype(f32), aabb_end=hi2.astype(f32))
    emptied = dict(both)
    nr = both["node_right"].copy()
    nr[nn:2 * nn][leaf] = 0
    emptied["node_right"] = nr
    if base in ("lit", "reflective"):
        # the lights stay on A's side of the plane: the outer point light goes to the far side of A
        pos = np.array(params["point_light_pos"], np.float64).reshape(-1, n)
        pos[:, 0] = np.where(pos[:, 0] > split, 2.0 * ctr[0] - pos[:, 0], pos[:, 0])
        params["point_light_pos"] = pos.astype(f32)
        g2 = np.zeros(n)
        g2[:3] = (-1.0, 0.1, 0.05)
        g2 /= np.linalg.norm(g2)
        params["global_light_dir"] = np.concatenate([np.asarray(params["global_light_dir"], f32).reshape(-1, n), g2[None].astype(f32)])
        params["global_light_color"] = np.concatenate([np.asarray(params["global_light_color"], f32).reshape(-1, 3), [[0.6, 0.55, 0.5]]]).astype(f32)
    plane_n = np.zeros((1, n), f32)
    plane_n[0, 0] = 1
    cams = []
    # (the cameras look at the middle of A's own points: a simplex fills little of its box, and a slice through the box's
    # centre can miss it)
    mid = np.concatenate([br.reshape(-1, rl), tr])[:, 1 + n:1 + 2 * n].astype(np.float64).mean(axis=0)
    for at, look in (((-3.0, 3.0), (4.2, -3.0)), ((5.5, 0.5), (-4.0, -0.4))):
        o = mid.copy()
        o[0], o[1] = ctr[0], ctr[1]
        o[0] += at[0] * ext[0]
        o[1] += at[1] * ext[1]
        fwd = np.zeros(n)
        fwd[0], fwd[1] = look[0] * ext[0], look[1] * ext[1]
        fwd /= np.linalg.norm(fwd)
        rgt = np.zeros(n)
        rgt[0], rgt[1] = -fwd[1], fwd[0]
        axes = np.eye(n)
        axes[0], axes[1], axes[2] = rgt, np.eye(n)[2], fwd
        if n > 3:
            axes[3:] = np.eye(n)[3:]
        cams.append((o.astype(f32), np.ascontiguousarray(axes, f32)))
    if variant == "glass-split":
        # the plane between the simplices of ONE batch: every batch keeps lanes 0 and 1 where they are and has lanes 2 and 3 at
        # B's place, and both trees list it.  What is expected is the oracle on the same tree with those two simplices of every
        # batch removed -- a record of zeroes, which no ray meets (N . d == 0) -- so that in A's leaves the batch is still tested
        # for what it keeps, and with B's leaves emptied as for every twin: nothing of what a batch keeps reaches into B's cells,
        # and a tree that listed it there would have the oracle test it on the way to A from camera 1, in cells that a primary
        # walk under the plane -- from max(aabb entry, t0) -- does not visit (with the reference's normal handling the order of
        # the tests shows in the colours: 2 pixels of camera 1, by the oracle alone)
        assert len(tr) == 0
        split_recs = np.array(both["batch_recs"][:len(br)])
        split_recs[:, 2:4] = both["batch_recs"][len(br):, 2:4]
        both.update(batch_recs=split_recs, batch_mats=bm, items=np.concatenate([items, items]))
        removed = split_recs.copy()
        removed[:, 2:4] = 0
        emptied.update(batch_recs=removed, batch_mats=bm, items=np.concatenate([items, items]))
    for d in (both, emptied):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return n, both, emptied, params, (plane_n, np.asarray([split], f32)), cams


# ------------------------------------------------------------------ one leaf by hand: a batch cut between its simplices
@functools.lru_cache(maxsize=None)
def one_leaf():
    """A 3-D scene of four batches in ONE leaf, every simplex a large triangle across the view at a depth z of its own (the
    other lanes: specks far outside the view), seen from the origin along +z, under the plane z >= 1:
        Q   lane 0 opaque at z = 3: the hit
        T   lane 0 transparent at z = 1.5
        P   lane 0 transparent at z = 2, lane 1 opaque at z = 0.5 -- cut away: the plane passes between P's simplices
        M   nothing in the view: a miss, the leaf's last test
    The reference's leaf trims its transparent hits with the distance of the LAST test (tracer.hpp:977-1086), so what the
    miss of M does after P matters: the expected records and colours are the oracle's on the same leaf with P's lane 1 removed
    (a record of zeroes).  (n, flat, flat with the simplex removed, params, (normals, offsets), (origin, axes))"""
    from ntracer_amd import Material, tracern
    n = 3
    opaque, glass = Material((1.0, 0.5, 0.25), 1.0), Material((0.25, 0.5, 1.0), 0.5)

    def across(z):
        return tracern.Triangle.from_points([(-50.0, -50.0, z), (50.0, -50.0, z), (0.0, 80.0, z)], opaque)._record()

    def speck(k):
        return tracern.Triangle.from_points([(90.0 + k, 90.0, 2.0), (90.5 + k, 90.0, 2.0), (90.0 + k, 90.5, 2.0)], opaque)._record()

    batches = [[across(3.0), speck(0), speck(1), speck(2)], [across(1.5), speck(3), speck(4), speck(5)],
               [across(2.0), across(0.5), speck(6), speck(7)], [speck(8), speck(9), speck(10), speck(11)]]
    recs = np.asarray(batches, f32)
    mats = np.asarray([[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    rl = n * n + n + 1
    flat = dict(root=0, node_axis=np.asarray([-1], np.int32), node_split=np.zeros(1, f32), node_left=np.zeros(1, np.int32),
                node_right=np.asarray([4], np.int32), items=(np.arange(4, dtype=np.int32) << 2), batch_recs=recs, batch_mats=mats,
                tri_recs=np.zeros((0, rl), f32), tri_mats=np.zeros(0, np.int32), solid_recs=np.zeros((0, 2 * n * n + n), f32),
                solid_types=np.zeros(0, np.int32), solid_mats=np.zeros(0, np.int32),
                materials=np.asarray([[1, 0.5, 0.25, 1, 1, 1, 1.0, 0, 0.5, 8], [0.25, 0.5, 1, 1, 1, 1, 0.5, 0, 0.5, 8]], f32),
                aabb_start=np.asarray([-100, -100, 0.25], f32), aabb_end=np.asarray([100, 100, 4], f32), batch_size=4)
    removed = dict(flat)
    r = recs.copy()
    r[2, 1] = 0
    removed["batch_recs"] = r
    z3 = np.zeros((0, 3), f32)
    params = dict(fov=f32(0.8), shadows=np.int32(0), camera_light=np.int32(1), max_reflect_depth=np.int32(0), bg_gradient_axis=np.int32(1),
                  ambient=np.asarray([0.05, 0.05, 0.05], f32), bg1=np.asarray([1, 1, 1], f32), bg2=np.zeros(3, f32), bg3=np.asarray([0, 1, 1], f32),
                  point_light_pos=z3, point_light_color=z3, global_light_dir=z3, global_light_color=z3)
    plane = (np.asarray([[0, 0, -1]], f32), np.asarray([-1.0], f32))
    cam = (np.zeros(3, f32), np.eye(3, dtype=f32))
    for d in (flat, removed):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return n, flat, removed, params, plane, cam


def one_leaf_views(which, width=9, height=7):
    """dist, item, lane, n_transparent [H][W] and frame [H][W][3] by the oracle: `which` "removed" (what the plane must give) or
    "whole" (the scene as it stands)"""
    n, flat, removed, params, plane, (o, axes) = one_leaf()
    f = removed if which == "removed" else flat
    sc = ob.OracleScene(n, o, axes, 0.8, flat=f, params=params)
    ys, xs = np.mgrid[0:height, 0:width]
    frame = np.asarray(sc.colors_at(xs.ravel().astype(np.int32), ys.ravel().astype(np.int32), width, height), f32).reshape(height, width, 3)
    d = np.asarray([sc.primary_dir(int(x), int(y), width, height) for x, y in zip(xs.ravel(), ys.ravel())], f32)
    t0 = ph.aabb_distance(np.asarray(f["aabb_start"], f32), np.asarray(f["aabb_end"], f32), o, d)
    assert (t0 >= 0).all()
    none = np.full(len(d), -1, np.int32)
    r = rq.Oracle(n, f, False, False).intersects(np.repeat(o[None], len(d), axis=0), d, t0, np.full(len(d), FLT_MAX), none, none)
    res = {key: r[key].reshape(height, width) for key in ("dist", "item", "lane", "n_transparent")}
    res["frame"] = frame
    return res


# ------------------------------------------------------------------ Reference A on two shells: a slab with something behind it
TWO_SHELLS = ["orthoplex5_n5", "simplex7_n7", "simplex10_n10"]


@functools.lru_cache(maxsize=None)
def two_shells(name):
    """The unlit twin of a golden scene as it stands, both halves, from a camera in front of A that looks along axis 0 with B
    behind A and a little beside it, under a slab that takes A away and keeps the near half of B: pixels of A move to B behind
    it, under a finite t1.  (n, flat, params, camera, d [H][W][n], aabb [H][W], the two planes, plain and cut records by the
    brute force)"""
    n, both, emptied, params, plane, cams = twin(name, "")
    flat_a = rq.scene(name)[2]
    lo_a, hi_a = np.asarray(flat_a["aabb_start"], np.float64), np.asarray(flat_a["aabb_end"], np.float64)
    ctr, ext = 0.5 * (lo_a + hi_a), 0.5 * (hi_a - lo_a)
    o = np.array(cams[0][0], np.float64)                   # (the hidden coordinates of the twin's cameras: the middle of A's points)
    o[0], o[1] = ctr[0] - 4.0 * ext[0], ctr[1] + 1.0 * ext[1]
    fwd = np.zeros(n)
    fwd[0], fwd[1] = 1.0 * ext[0], -0.15 * ext[1]
    fwd /= np.linalg.norm(fwd)
    axes = np.eye(n)
    axes[0, :2] = (-fwd[1], fwd[0])
    axes[0, 2:] = 0
    axes[1], axes[2] = np.eye(n)[2], fwd
    o, axes = o.astype(f32), np.ascontiguousarray(axes, f32)
    sc = ob.OracleScene(n, o, axes, ph.fov_of(name), flat=both, params=params)
    d = np.zeros((H, W, n), f32)
    for y in range(H):
        for x in range(W):
            d[y, x] = sc.primary_dir(x, y, W, H)
    lo, hi = np.asarray(both["aabb_start"], f32), np.asarray(both["aabb_end"], f32)
    aabb = ph.aabb_distance(lo, hi, o, d.reshape(-1, n)).reshape(H, W)
    recs4 = records_of(n, both)
    t = _candidates(recs4[0], recs4[3], n, o, d.reshape(-1, n))
    plain = brute_rays(recs4, n, o, d, aabb, NO_PLANES, t)
    # a = -(forward + 0.3 right); the nearer plane through the point between the shells, the farther through B's middle
    a = _axes_normal(axes, 0)
    nb = len(both["batch_recs"]) // 2
    nt = len(both["tri_recs"]) // 2
    pts = np.concatenate([np.asarray(both["batch_recs"][nb:], f32).reshape(-1, recs4[0].shape[1]), np.asarray(both["tri_recs"][nt:], f32)])
    b_mid = pts[:, 1 + n:1 + 2 * n].astype(np.float64).mean(axis=0)
    between = b_mid.copy()
    between[0] = float(plane[1][0])
    planes2 = (np.asarray([a, -a], f32), np.asarray([np.dot(a.astype(np.float64), between), -np.dot(a.astype(np.float64), b_mid)], f32))
    cut = brute_rays(recs4, n, o, d, aabb, planes2, t)
    for v in (d, aabb) + planes2:
        v.setflags(write=False)
    return n, both, params, (o, axes), d, aabb, planes2, plain, cut


def _twin_views(name, variant, k, width, height, which):
    n, both, emptied, params, plane, cams = twin(name, variant)
    o, axes = cams[k]
    flat = both if which == "both" else emptied
    prune = True                                            # (no Solids, no strict switch: the library prunes)
    sc = ob.OracleScene(n, o, axes, ph.fov_of(name), flat=flat, params=params, prune=prune)
    ys, xs = np.mgrid[0:height, 0:width]
    frame = np.asarray(sc.colors_at(xs.ravel().astype(np.int32), ys.ravel().astype(np.int32), width, height), f32).reshape(height, width, 3)
    d = np.zeros((height * width, n), f32)
    for i, (x, y) in enumerate(zip(xs.ravel(), ys.ravel())):
        d[i] = sc.primary_dir(int(x), int(y), width, height)
    t0 = ph.aabb_distance(np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32), o, d)
    count = width * height
    rec = dict(dist=np.full(count, FLT_MAX, f32), item=np.full(count, -1, np.int32), lane=np.full(count, -1, np.int32),
               n_transparent=np.zeros(count, np.int32))
    enter = np.nonzero(t0 >= 0)[0]
    if len(enter):
        none = np.full(len(enter), -1, np.int32)
        r = rq.Oracle(n, flat, False, prune).intersects(np.repeat(o[None], len(enter), axis=0), d[enter], t0[enter], np.full(len(enter), FLT_MAX),
                                                        none, none)
        for key in rec:
            rec[key][enter] = r[key]
    res = {key: v.reshape(height, width) for key, v in rec.items()}
    res["frame"] = frame
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def twin_expected(name, variant, k, width=W, height=H):
    """dist, item, lane, n_transparent [H][W] and frame [H][W][3] of the twin from its camera k with B's leaves emptied"""
    return _twin_views(name, variant, k, width, height, "emptied")


@functools.lru_cache(maxsize=None)
def twin_unclipped(name, variant, k, width=W, height=H):
    """the same of the twin as it stands: what the plane must take away"""
    return _twin_views(name, variant, k, width, height, "both")


def twin_census(name, variant, k):
    """(pixels whose record B changes, pixels whose colour B changes, pixels that show A) at 37 x 21, by the oracle alone"""
    a, b = twin_expected(name, variant, k), twin_unclipped(name, variant, k)
    rec = (a["item"] != b["item"]) | (a["n_transparent"] != b["n_transparent"])
    col = (np.abs(a["frame"] - b["frame"]) > 1e-4).any(axis=2)
    return int(rec.sum()), int(col.sum()), int((a["item"] >= 0).sum())


if __name__ == "__main__":
    import time
    for name in SCENES_A:
        for k in CAMERAS:
            t = time.time()
            if name in PINNED:
                e = ph.expected((name, {}), W, H, k)
                bad = int((brute(name, W, H, k, NO_PLANES)["dist"].view(np.uint32) != e["dist"].view(np.uint32)).sum())
            else:
                bad = -1
            print("%-14s camera %d: %d mismatches of %d without planes; (moved, unchanged, lost, near) %s  (%.1f s)"
                  % (name, k, bad, W * H, {kind: census(name, kind, k) for kind in KINDS}, time.time() - t))
    for t in TWINS:
        for k in TWIN_CAMERAS:
            print("%-24s camera %d: (records, colours changed by B, pixels of A) %r" % (twin_id(t), k, twin_census(t[0], t[1], k)))
