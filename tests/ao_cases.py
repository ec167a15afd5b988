"""Expected ambient-occlusion counts, shared by tests/test_ao_host.py and tests/test_ao_gpu.py, from the oracle alone.

For every pixel (x, y) of a width x height view of a golden scene from its golden camera 0, nothing left out: the record and the
normal ray of primary_hit_cases.expected, the primary direction d of primary_hit_cases.rays, and the definition of
include/ntracer_hip.h restated in sequential fp32 numpy --
    side = -dot(d, nd),  b = side < 0 ? -bias : bias,  o' = no + nd * b,
    s = dot(nd, t_k),  v = ((s < 0) != (side < 0)) ? -t_k : t_k,
every dot product summed left to right, every operation rounded to fp32 on its own -- and the K samples answered by
ray_query_cases.Oracle.intersects (nto_kd_intersects with t_near = 0, t_far = radius and the primary hit as the skip target) in
the mode ray_query_cases.batches picks for the case.  blocked = number of samples with item >= 0 and dist <= radius, -1 for a
pixel without an opaque hit.  Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import fixtures as fx
import primary_hit_cases as ph
import ray_query_cases as rq
from ntracer_amd import sphere_directions

f32 = np.float32

# (scene, switches): the route each takes is pinned in test_ao_host.py (AO_ROUTES)
CASES = [
    ("cell120_n4", {}),
    ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}),
    ("cell120_n4", {"NTRACER_FORCE_VAR": "1"}),
    ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
    ("feature5_n5", {}),
    ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}),
    ("feature16_n16", {}),
    ("orthoplex5_n5", {}),
    ("simplex10_n10", {}),          # (a second convex control: the fixed-n kernel's instantiation for leaves with unbatched triangles)
]
SIZES = [(1, 1), (8, 8), (9, 7), (37, 21)]
BIG = (64, 48)                      # cell120_n4 plain only
SWITCHES = ph.SWITCHES
K, SEED, RADIUS, BIAS = 8, 1, 1.0, 1e-3

case_id = rq.case_id


def sizes(case):
    return SIZES + ([BIG] if case == CASES[0] else [])


def table(n, count=K, seed=SEED):
    return sphere_directions(n, count, seed)


def dot_lr(a, b):
    """row-wise dot product of two [count][n] fp32 arrays, summed left to right in fp32"""
    s = (a[:, 0] * b[:, 0]).astype(f32)
    for k in range(1, a.shape[1]):
        s = (s + (a[:, k] * b[:, k]).astype(f32)).astype(f32)
    return s


def blocked_of(n, flat, clean, prune, e, d, T, radius, bias):
    """the rule on the primary-hit records e (dist / item / lane / normal_origin / normal [H][W]...) and the primary directions
    d [H][W][n] of any flat scene: what _expected returns"""
    height, width = e["item"].shape
    count = len(T)
    hit = np.nonzero(e["item"].ravel() >= 0)[0]
    blocked = np.full(width * height, -1, np.int32)
    dist = np.full((width * height, count), rq.FLT_MAX, f32)
    item = np.full((width * height, count), -1, np.int32)
    if len(hit):
        dd = np.ascontiguousarray(d.reshape(-1, n)[hit], f32)
        no = np.ascontiguousarray(e["normal_origin"].reshape(-1, n)[hit], f32)
        nd = np.ascontiguousarray(e["normal"].reshape(-1, n)[hit], f32)
        side = (-dot_lr(dd, nd)).astype(f32)
        b = np.where(side < 0, f32(-f32(bias)), f32(bias)).astype(f32)
        o2 = (no + (nd * b[:, None]).astype(f32)).astype(f32)
        orc = rq.Oracle(n, flat, clean, prune)
        si, sl = e["item"].ravel()[hit], e["lane"].ravel()[hit]
        zero, far = np.zeros(len(hit), f32), np.full(len(hit), f32(radius))
        total = np.zeros(len(hit), np.int32)
        for k in range(count):
            tk = np.repeat(T[k][None], len(hit), axis=0)
            s = dot_lr(nd, tk)
            flip = (s < 0) != (side < 0)
            v = np.where(flip[:, None], -tk, tk).astype(f32)
            r = orc.intersects(o2, v, zero, far, si, sl)
            total += ((r["item"] >= 0) & (r["dist"] <= f32(radius))).astype(np.int32)
            dist[hit, k] = r["dist"]
            item[hit, k] = r["item"]
        blocked[hit] = total
    out = dict(blocked=blocked.reshape(height, width), dist=dist.reshape(height, width, count), item=item.reshape(height, width, count),
               hit=(e["item"] >= 0))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, clean, prune, width, height, tkey, radius, bias):
    g, n, flat = rq.scene(name)
    T = np.frombuffer(tkey, f32).reshape(-1, n)
    env = dict([("NTRACER_CLEAN_NORMALS", "1")] if clean else [])
    if not prune:
        env["NTRACER_STRICT_REFERENCE"] = "1"               # (primary_hit_cases.expected: no pruning, whatever the scene)
    e = ph.expected((name, env), width, height)
    d, _ = ph.rays(name, width, height, 0)
    return blocked_of(n, flat, clean, prune, e, d, T, radius, bias)


def expected(case, width, height, T=None, radius=RADIUS, bias=BIAS):
    """blocked [H][W] int32, the samples' dist / item [H][W][K] as the oracle answered them, and hit [H][W]"""
    name, env = case
    g, n, flat = rq.scene(name)
    T = table(n) if T is None else np.ascontiguousarray(T, f32)
    prune = env.get("NTRACER_STRICT_REFERENCE") != "1" and len(flat["solid_types"]) == 0
    return _expected(name, env.get("NTRACER_CLEAN_NORMALS") == "1", prune, width, height, T.tobytes(), float(f32(radius)), float(f32(bias)))


def shade(P, blocked, count, strength):
    """the render's colours: P [H][W][3] fp32 (clamped) times f = 1 - strength * blocked / K, each operation in fp32"""
    a = np.where(blocked < 0, f32(0), blocked.astype(f32) / f32(count)).astype(f32)
    f = (f32(1.0) - (f32(strength) * a).astype(f32)).astype(f32)
    return (P * f[..., None]).astype(f32)


def scene_params(name):
    return fx.params_of(rq.scene(name)[0])
