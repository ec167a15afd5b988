"""Expected primary-hit buffers, shared by tests/test_primary_hits_host.py and tests/test_primary_hits_gpu.py.

For every pixel (x, y) of a width x height view of a golden scene from one of its golden cameras, nothing left out:
d from nto_primary_dir, t0 from an fp32 numpy restatement of the oracle's aabb_distance (oracle/ntracer_oracle.c:643-662,
the same operations in the same order), and for t0 >= 0 the record of nto_kd_intersects(origin, d, t0, FLT_MAX, -1, -1),
called directly as ray_query_cases.Oracle does so that n_transparent survives a miss.  The oracle runs in the GPU's mode,
as ray_query_cases.batches has it: clean normals only under NTRACER_CLEAN_NORMALS=1, prune_beyond_hit exactly where the
library prunes.  The restatement is pinned by test_primary_hits_host.py against the counters of nto_colors_at.
Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import oracle_binding as ob
import ray_query_cases as rq

FLT_MAX = rq.FLT_MAX
f32 = np.float32

# (scene, switches) -> the kernel route it takes is pinned in test_primary_hits_host.py (HITS_ROUTES)
CASES = [
    ("cell600_n4", {}),
    ("cell600_n4", {"NTRACER_STRICT_REFERENCE": "1"}),
    ("cell600_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
    ("simplex7_n7", {}),
    ("simplex10_n10", {}),
    ("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}),
    ("simplex10_n10", {"NTRACER_COMPOSITE_KERNEL": "2"}),
    ("feature5_n5", {}),
    ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}),
    ("feature11_n11", {}),
    ("feature11_n11", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("lit12_n12", {}),
    ("feature16_n16", {}),
]
# 1 x 1; one tile; a partial tile; 5 x 3 tiles, so quads with absent waves; several quads each way
SIZES = [(1, 1), (8, 8), (9, 7), (37, 21), (64, 48)]
# the switches a primary-hit pass routes on
SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL")
# the scenes of the counter check
COUNTED = ["cell600_n4", "feature5_n5", "simplex7_n7", "simplex10_n10", "feature11_n11", "lit12_n12", "feature16_n16"]

case_id = rq.case_id


def aabb_distance(lo, hi, o, d):
    """composite_scene::aabb_distance as the oracle states it, in fp32, for rays d [count][n] from one origin: per ray the
    oracle's operations in the oracle's order (its early exits only skip work whose result it would not use)"""
    count, n = d.shape
    result = np.full(count, -1, f32)
    done = np.zeros(count, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            di = d[:, i]
            face = np.where(di > 0, lo[i], hi[i]).astype(f32)
            dist = ((face - o[i]).astype(f32) / di).astype(f32)
            neg = dist < 0                                   # dist = 0, skip = -1: axis i is tested too
            dist = np.where(neg, f32(0), dist).astype(f32)
            ok = ~done & (di != 0)
            for j in range(n):
                p = ((d[:, j] * dist).astype(f32) + o[j]).astype(f32)
                outside = (p >= hi[j]) | (p <= lo[j])
                ok &= ~(outside & neg) if j == i else ~outside
            result = np.where(ok, dist, result).astype(f32)
            done |= ok
    return result


def camera(name, k=0):
    """(origin, axes) of the k-th golden camera of a scene"""
    g = rq.scene(name)[0]
    f = int(g["frames"][k])
    return np.asarray(g["origins"][f], f32), np.asarray(g["axes"][f], f32)


def fov_of(name):
    g = rq.scene(name)[0]
    return float(g["fov"]) if "fov" in g else 0.8


@functools.lru_cache(maxsize=None)
def rays(name, width, height, k=0):
    """(directions [H][W][n], t0 [H][W]) of the view from the k-th golden camera"""
    g, n, flat = rq.scene(name)
    o, axes = camera(name, k)
    sc = ob.OracleScene(n, o, axes, fov_of(name))
    lo, hi = np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32)
    d = np.zeros((height, width, n), f32)
    for y in range(height):
        for x in range(width):
            d[y, x] = sc.primary_dir(x, y, width, height)
    t0 = aabb_distance(lo, hi, o, d.reshape(-1, n)).reshape(height, width)
    d.setflags(write=False)
    t0.setflags(write=False)
    return d, t0


@functools.lru_cache(maxsize=None)
def _expected(name, clean, prune, width, height, k):
    g, n, flat = rq.scene(name)
    o, _ = camera(name, k)
    d, t0 = rays(name, width, height, k)
    enter = np.nonzero(t0.ravel() >= 0)[0]
    count = width * height
    out = dict(dist=np.full(count, FLT_MAX, f32), item=np.full(count, -1, np.int32), lane=np.full(count, -1, np.int32),
               n_transparent=np.zeros(count, np.int32), normal_origin=np.zeros((count, n), f32), normal=np.zeros((count, n), f32))
    if len(enter):
        none = np.full(len(enter), -1, np.int32)
        r = rq.Oracle(n, flat, clean, prune).intersects(np.repeat(o[None], len(enter), axis=0), d.reshape(count, n)[enter], t0.ravel()[enter],
                                                        np.full(len(enter), FLT_MAX), none, none)
        for key in out:
            out[key][enter] = r[key]
    out["normal_origin"][out["item"] < 0] = 0              # (what a walk that found nothing left in o_hit.normal is not handed out)
    out["normal"][out["item"] < 0] = 0
    res = {key: v.reshape((height, width) + v.shape[1:]) for key, v in out.items()}
    res["t0"] = t0
    for v in res.values():
        v.setflags(write=False)
    return res


def expected(case, width, height, k=0):
    """dist, item, lane, n_transparent [H][W], normal_origin / normal [H][W][n] (zero where nothing opaque was hit) and t0"""
    name, env = case
    g, n, flat = rq.scene(name)
    prune = env.get("NTRACER_STRICT_REFERENCE") != "1" and len(flat["solid_types"]) == 0
    return _expected(name, env.get("NTRACER_CLEAN_NORMALS") == "1", prune, width, height, k)
