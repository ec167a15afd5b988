"""Ray sets and oracle answers shared by tests/test_ray_queries_host.py and tests/test_ray_queries_gpu.py.

A *case* is a golden scene with a set of NTRACER_* switches.  For each case the rays of the three sets the tests run --
(A) the golden cameras' primary rays, (B) second legs from the oracle's hit points, (C) seeded edge cases with t_near /
t_far windows -- are laid end to end in ONE closest-hit batch and ONE occlusion batch, so that a case costs one pass of
the oracle (nto_kd_intersects / nto_kd_occludes, ray by ray, nothing left out) and the GPU test can send the whole batch,
or any prefix of it, in one launch.  Everything is computed once per process and never modified afterwards."""
import ctypes as C
import functools

import numpy as np

import fixtures as fx
import oracle_binding as ob

FLT_MAX = np.float32(3.4028234663852886e38)
SEED = 20240611
N_EDGE = 500            # rays of set (C) a scene

# (scene, switches): every row of QUERY_ROUTES in test_ray_queries_host.py names one of these
CASES = [
    ("cell600_n4", {}),
    ("cell600_n4", {"NTRACER_STRICT_REFERENCE": "1"}),
    ("feature5_n5", {}),
    ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}),
    ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("simplex7_n7", {}),
    ("simplex10_n10", {}),
    ("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}),
    ("feature11_n11", {}),
    ("feature11_n11", {"NTRACER_CLEAN_NORMALS": "1"}),
    ("lit12_n12", {}),
    ("feature16_n16", {}),
]


def case_id(case):
    name, env = case
    return name + "".join("," + k[len("NTRACER_"):] for k in sorted(env))


@functools.lru_cache(maxsize=None)
def scene(name):
    g = fx.load(name)
    n = int(g["dimension"])
    return g, n, fx.flat_of(g)


class Oracle(object):
    """nto_kd_intersects / nto_kd_occludes over arrays of rays"""

    def __init__(self, n, flat, clean_normals, prune):
        self.n = n
        self.sc = ob.OracleScene(n, np.zeros(n, np.float32), np.eye(n, dtype=np.float32), flat=flat, clean_normals=clean_normals, prune=prune)

    def intersects(self, o, d, t_near, t_far, skip_item, skip_lane):
        L, n, count = ob.lib(), self.n, len(o)
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        out = dict(dist=np.full(count, FLT_MAX, np.float32), item=np.full(count, -1, np.int32), lane=np.full(count, -1, np.int32),
                   n_transparent=np.zeros(count, np.int32), normal_origin=np.zeros((count, n), np.float32),
                   normal=np.zeros((count, n), np.float32))
        dist, kind, index, lane, nt = C.c_float(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        row = n * 4
        po, pd = o.ctypes.data, d.ctypes.data
        pno, pnd = out["normal_origin"].ctypes.data, out["normal"].ctypes.data
        f32p = ob.f32p
        for i in range(count):
            r = L.nto_kd_intersects(C.byref(self.sc.s), C.cast(po + i * row, f32p), C.cast(pd + i * row, f32p), float(t_near[i]), float(t_far[i]),
                                    int(skip_item[i]), int(skip_lane[i]), C.byref(dist), C.byref(kind), C.byref(index), C.byref(lane),
                                    C.cast(pno + i * row, f32p), C.cast(pnd + i * row, f32p), C.byref(nt))
            out["n_transparent"][i] = nt.value
            if r:
                out["dist"][i] = dist.value
                out["item"][i] = (index.value << 2) | kind.value
                out["lane"][i] = lane.value
        return out

    def occludes(self, o, d, distance, t_near, t_far, skip_item, skip_lane):
        L, n, count = ob.lib(), self.n, len(o)
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        out = dict(blocked=np.zeros(count, bool), n_transparent=np.zeros(count, np.int32))
        nt = C.c_int32()
        row = n * 4
        po, pd = o.ctypes.data, d.ctypes.data
        f32p = ob.f32p
        for i in range(count):
            r = L.nto_kd_occludes(C.byref(self.sc.s), C.cast(po + i * row, f32p), C.cast(pd + i * row, f32p), float(distance[i]),
                                  float(t_near[i]), float(t_far[i]), int(skip_item[i]), int(skip_lane[i]), C.byref(nt))
            out["blocked"][i] = bool(r)
            out["n_transparent"][i] = nt.value
        return out


def _unit(v):
    v = np.asarray(v, np.float32)
    return (v / np.sqrt((v * v).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def primary_rays(name):
    """set (A): (origins, directions, rays per frame) of every golden frame's golden pixels, directions from nto_primary_dir"""
    g, n, flat = scene(name)
    w, h = int(g["width"]), int(g["height"])
    fov = float(g["fov"]) if "fov" in g else 0.8
    xs, ys = g["xs"], g["ys"]
    os_, ds = [], []
    for f in g["frames"]:
        sc = ob.OracleScene(n, g["origins"][f], g["axes"][f], fov)
        os_.append(np.repeat(np.asarray(g["origins"][f], np.float32)[None], len(xs), axis=0))
        ds.append(np.stack([sc.primary_dir(int(x), int(y), w, h) for x, y in zip(xs, ys)]))
    return np.concatenate(os_), np.concatenate(ds), len(xs)


class Batches(object):
    pass


@functools.lru_cache(maxsize=None)
def _batches(name, clean, prune):
    g, n, flat = scene(name)
    orc = Oracle(n, flat, clean, prune)
    rng = np.random.default_rng(SEED)
    lo, hi = np.asarray(g["aabb_start"], np.float32), np.asarray(g["aabb_end"], np.float32)

    # ---- (A)
    oa, da, per_frame = primary_rays(name)
    na = len(oa)
    none_i = np.full(na, -1, np.int32)
    ra = orc.intersects(oa, da, np.full(na, -FLT_MAX), np.full(na, FLT_MAX), none_i, none_i)

    # ---- (B): from the hit point of every ray of (A) that hit, towards a random point of the scene's box
    hit = np.nonzero(ra["item"] >= 0)[0]
    ob_ = (oa[hit] + ra["dist"][hit, None] * da[hit]).astype(np.float32)
    to = (lo + (hi - lo) * rng.random((len(hit), n), dtype=np.float32)).astype(np.float32) - ob_
    length = np.sqrt((to * to).sum(axis=1, dtype=np.float32)).astype(np.float32)
    db = (to / length[:, None]).astype(np.float32)
    sib, slb = ra["item"][hit].copy(), ra["lane"][hit].copy()

    # ---- (C): origins inside the box; every fifth direction with a component exactly 0; every seventh origin exactly on
    # the root's split plane
    oc = (lo + (hi - lo) * rng.random((N_EDGE, n), dtype=np.float32)).astype(np.float32)
    dc = _unit(rng.standard_normal((N_EDGE, n)))
    dc[np.arange(0, N_EDGE, 5), rng.integers(0, n, len(range(0, N_EDGE, 5)))] = 0.0
    root = int(flat["root"])
    if root >= 0 and int(flat["node_axis"][root]) >= 0:
        oc[::7, int(flat["node_axis"][root])] = np.float32(flat["node_split"][root])
    nc_i = np.full(N_EDGE, -1, np.int32)
    rc = orc.intersects(oc, dc, np.full(N_EDGE, -FLT_MAX), np.full(N_EDGE, FLT_MAX), nc_i, nc_i)
    # windows at 0.5x and 1.5x of the unwindowed distance: around the hit, beyond it, before it, and inverted
    base = np.where(rc["item"] >= 0, rc["dist"], np.float32(1.0)).astype(np.float32)
    pat = np.arange(N_EDGE) % 4
    tn = np.select([pat == 0, pat == 1, pat == 2], [0.5 * base, 1.5 * base, np.full(N_EDGE, -FLT_MAX)], 1.5 * base).astype(np.float32)
    tf = np.select([pat == 0, pat == 1, pat == 2], [1.5 * base, np.full(N_EDGE, FLT_MAX), 0.5 * base], 0.5 * base).astype(np.float32)

    b = Batches()
    b.n, b.name = n, name
    b.per_frame, b.n_a, b.n_b = per_frame, na, len(hit)
    # closest hit: A | B | C unwindowed | C windowed
    b.i_slices = dict(A=slice(0, na), B=slice(na, na + len(hit)), C=slice(na + len(hit), na + len(hit) + N_EDGE),
                      CW=slice(na + len(hit) + N_EDGE, na + len(hit) + 2 * N_EDGE))
    b.i_origins = np.ascontiguousarray(np.concatenate([oa, ob_, oc, oc]))
    b.i_directions = np.ascontiguousarray(np.concatenate([da, db, dc, dc]))
    b.i_t_near = np.concatenate([np.full(na + len(hit) + N_EDGE, -FLT_MAX, np.float32), tn])
    b.i_t_far = np.concatenate([np.full(na + len(hit) + N_EDGE, FLT_MAX, np.float32), tf])
    b.i_skip_item = np.concatenate([none_i, sib, nc_i, nc_i]).astype(np.int32)
    b.i_skip_lane = np.concatenate([none_i, slb, nc_i, nc_i]).astype(np.int32)
    rb = orc.intersects(ob_, db, np.full(len(hit), -FLT_MAX), np.full(len(hit), FLT_MAX), sib, slb)
    rcw = orc.intersects(oc, dc, tn, tf, nc_i, nc_i)
    b.i_ref = {k: np.concatenate([ra[k], rb[k], rc[k], rcw[k]]) for k in ra}
    # occlusion: A with distance = FLT_MAX | B with the leg's length and the skip | C windowed, distance = FLT_MAX
    b.o_slices = dict(A=slice(0, na), B=slice(na, na + len(hit)), CW=slice(na + len(hit), na + len(hit) + N_EDGE))
    b.o_origins = np.ascontiguousarray(np.concatenate([oa, ob_, oc]))
    b.o_directions = np.ascontiguousarray(np.concatenate([da, db, dc]))
    b.o_distance = np.concatenate([np.full(na, FLT_MAX, np.float32), length, np.full(N_EDGE, FLT_MAX, np.float32)])
    b.o_t_near = np.concatenate([np.full(na + len(hit), -FLT_MAX, np.float32), tn])
    b.o_t_far = np.concatenate([np.full(na + len(hit), FLT_MAX, np.float32), tf])
    b.o_skip_item = np.concatenate([none_i, sib, nc_i]).astype(np.int32)
    b.o_skip_lane = np.concatenate([none_i, slb, nc_i]).astype(np.int32)
    b.o_ref = orc.occludes(b.o_origins, b.o_directions, b.o_distance, b.o_t_near, b.o_t_far, b.o_skip_item, b.o_skip_lane)
    for v in list(vars(b).values()) + list(b.i_ref.values()) + list(b.o_ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def batches(case):
    """The two batches of a case with the oracle in the GPU's mode: clean normals only under NTRACER_CLEAN_NORMALS=1, and
    prune_beyond_hit wherever the library prunes -- not under strict_reference, and never in a scene with Solids (nt_api.cpp:
    the reference's own trees leave solids out of cells they reach; on the rays here the two walks agree on every hit and
    every count, and differ only in the marks missed cubes leave on o_hit.normal.origin).  NTRACER_FORCE_VAR changes the
    kernels, not the answers: it shares the default's batches."""
    name, env = case
    g, n, flat = scene(name)
    prune = env.get("NTRACER_STRICT_REFERENCE") != "1" and len(flat["solid_types"]) == 0
    return _batches(name, env.get("NTRACER_CLEAN_NORMALS") == "1", prune)
