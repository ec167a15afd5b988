"""Expected outline masks, shared by tests/test_outlines_host.py and tests/test_outlines_gpu.py, from the oracle alone.

For every pixel (x, y) of a width x height view of a golden scene from one of its golden cameras, nothing left out: the record
(dist, item, lane) and the normal ray's direction nd of primary_hit_cases.expected, and the definition of include/ntracer_hip.h
restated in sequential fp32 numpy -- for each of the four neighbours q inside the image
    silhouette  if item(q) < 0
    nothing     if (item, lane)(q) == (item, lane)(p), or dist(p) > dist(q)
    crease      if c * c < cc * (la * lb),      c = nd(p).nd(q), la = nd(p).nd(p), lb = nd(q).nd(q), cc = crease_cos * crease_cos
    depth       if depth_gap > 0 and (dist(q) - dist(p)) > depth_gap * dist(p)
every dot product summed left to right (ao_cases.dot_lr), every operation rounded to fp32 on its own.  Besides the mask bytes
the pairs are counted by what became of them, and the crease test's distance from its threshold is kept, for the conditions
test_outlines_host.py asserts.  Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import ao_cases as ao
import fixtures as fx
import primary_hit_cases as ph
import ray_query_cases as rq

f32 = np.float32

SILHOUETTE, CREASE, DEPTH = 1, 2, 4

# (scene, switches): the route each takes is pinned in test_outlines_host.py (OUTLINE_ROUTES)
CASES = [
    ("cell120_n4", {}),
    ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}),
    ("cell120_n4", {"NTRACER_FORCE_VAR": "1"}),
    ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
    ("cell600_n4", {}),
    ("orthoplex5_n5", {}),
    ("simplex10_n10", {}),
    ("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}),
    ("feature5_n5", {}),
    ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}),
    ("feature11_n11", {}),
    ("feature16_n16", {}),
]
# 1 x 1: no neighbour at all; one column, one row; one tile; a partial tile; 17 x 17: neighbours in other 16 x 16 blocks both
# ways; 3 x 2 blocks
SIZES = [(1, 1), (1, 7), (7, 1), (8, 8), (9, 7), (17, 17), (37, 21)]
BIG = (64, 48)                      # cell120_n4 plain only
SWITCHES = ph.SWITCHES
# (crease_cos, depth_gap)
A = (0.995, 0.02)
B = (0.9, 0.0)
PARAMS = [("A", A), ("B", B)]
# (scene, variant of ray_color_cases.case_scene) of the renders: no lights, transparent materials and Solids, lights and
# shadows on batches alone, loose triangles -- the three instantiations of the shading pass and the general route
RENDERED = [("cell120_n4", ""), ("feature5_n5", ""), ("cell600_n4", "lit"), ("simplex10_n10", "")]

case_id = rq.case_id


def sizes(case):
    return SIZES + ([BIG] if case == CASES[0] else [])


def mask_of(dist, item, lane, normal, crease_cos, depth_gap):
    """(mask [H][W] uint8, counts): the rule on records dist / item / lane [H][W] and normal rows [H][W][n]"""
    height, width = item.shape
    n = normal.shape[2]
    dist, normal = np.asarray(dist, f32), np.asarray(normal, f32)
    cc = f32(f32(crease_cos) * f32(crease_cos))
    gap = f32(depth_gap)
    mask = np.zeros((height, width), np.uint8)
    counts = dict(silhouette=0, crease=0, depth=0, unmarked=0, farther=0, equal_dist=0, same=0, margin=np.inf, lengths=set())
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        # p runs over the pixels whose neighbour (x + dx, y + dy) lies inside the image
        ys = slice(max(0, -dy), height - max(0, dy))
        xs = slice(max(0, -dx), width - max(0, dx))
        yq = slice(max(0, -dy) + dy, height - max(0, dy) + dy)
        xq = slice(max(0, -dx) + dx, width - max(0, dx) + dx)
        ip, iq, lp, lq = item[ys, xs], item[yq, xq], lane[ys, xs], lane[yq, xq]
        dp, dq = dist[ys, xs], dist[yq, xq]
        if ip.size == 0:
            continue
        hit = ip >= 0
        sil = hit & (iq < 0)
        same = hit & (iq >= 0) & (iq == ip) & (lq == lp)
        farther = hit & (iq >= 0) & ~same & (dp > dq)
        cand = hit & (iq >= 0) & ~same & ~farther
        m = np.where(sil, SILHOUETTE, 0).astype(np.uint8)
        idx = np.nonzero(cand)
        if len(idx[0]):
            na = np.ascontiguousarray(normal[ys, xs][idx], f32).reshape(-1, n)
            nb = np.ascontiguousarray(normal[yq, xq][idx], f32).reshape(-1, n)
            c, la, lb = ao.dot_lr(na, nb), ao.dot_lr(na, na), ao.dot_lr(nb, nb)
            lhs = (c * c).astype(f32)
            rhs = (cc * (la * lb).astype(f32)).astype(f32)
            crease = lhs < rhs
            a, b = dp[idx], dq[idx]
            depth = (gap > 0) & ((b - a).astype(f32) > (gap * a).astype(f32))
            m[idx] |= np.where(crease, CREASE, 0).astype(np.uint8) | np.where(depth, DEPTH, 0).astype(np.uint8)
            counts["crease"] += int(crease.sum())
            counts["depth"] += int(depth.sum())
            counts["unmarked"] += int((~crease & ~depth).sum())
            counts["equal_dist"] += int((a == b).sum())
            with np.errstate(all="ignore"):
                rel = np.abs(lhs.astype(np.float64) - rhs.astype(np.float64)) / rhs.astype(np.float64)
            counts["margin"] = min(counts["margin"], float(rel.min()))
            counts["lengths"] |= set(np.round(np.sqrt(np.concatenate([la, lb]).astype(np.float64)), 3).tolist())
        counts["silhouette"] += int(sil.sum())
        counts["farther"] += int(farther.sum())
        counts["same"] += int(same.sum())
        mask[ys, xs] |= m
    counts["lengths"] = tuple(sorted(counts["lengths"]))
    return mask, counts


@functools.lru_cache(maxsize=None)
def _expected(name, envkey, width, height, k, crease_cos, depth_gap):
    e = ph.expected((name, dict(envkey)), width, height, k)
    mask, counts = mask_of(e["dist"], e["item"], e["lane"], e["normal"], crease_cos, depth_gap)
    mask.setflags(write=False)
    return mask, counts


def expected(case, width, height, params=A, k=0):
    """(mask [H][W] uint8, counts of the pairs) of the view from the k-th golden camera under params = (crease_cos, depth_gap)"""
    name, env = case
    return _expected(name, tuple(sorted(env.items())), width, height, k, float(params[0]), float(params[1]))


def blend(P, mask, color, strength):
    """the render's colours: P [H][W][3] fp32 (clamped), (P * (1 - strength)) + (color * strength) where the mask is set"""
    keep = f32(f32(1.0) - f32(strength))
    add = (np.asarray(color, f32) * f32(strength)).astype(f32)
    lined = ((P * keep).astype(f32) + add[None, None, :]).astype(f32)
    return np.where((mask != 0)[..., None], lined, P).astype(f32)


def crease_angle(crease_cos):
    """an angle whose float32 cosine is exactly crease_cos, for scene.set_outlines"""
    import math
    a = math.acos(float(crease_cos))
    for cand in (a, np.nextafter(a, 0), np.nextafter(a, 4), a - 1e-9, a + 1e-9):
        if f32(math.cos(float(cand))) == f32(crease_cos):
            return float(cand)
    raise AssertionError("no angle for crease_cos %r" % crease_cos)


def scene_params(name):
    return fx.params_of(rq.scene(name)[0])
