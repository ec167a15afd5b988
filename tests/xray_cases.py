"""The reference of the X-ray tests (tests/test_xray_host.py, tests/test_xray_gpu.py): nothing here comes from the code under test.

crossings32 is the rule of include/ntracer_hip.h restated in numpy, fp32 operation by operation -- every np.float32 operation its
own step, every sum left to right in an explicit loop, as primary_hit_cases.aabb_distance is written -- over ALL primitives of
the scene, no tree.  Solids go through solid_cases._cube64 / _sphere64 on their local rays, with those functions' margins.  B,
the colour of a ray that hits nothing, is the oracle's colour of the same rays with the same scene parameters and an empty tree.
The expected colour is float64 arithmetic on the fp32 transmittances and the fp32 B.  test_xray_host.py pins the restatement to
the oracle: its nearest accepted t is nto_kd_intersects' dist bit for bit.  Everything is computed once per process and never
modified afterwards."""
import functools

import numpy as np

import fixtures as fx
import oracle_binding as ob
import primary_hit_cases as ph
import ray_query_cases as rq
import solid_cases as sd

f32 = np.float32
FLT_MAX = rq.FLT_MAX
FUZZ = f32(f32(1.1920928955078125e-07) * f32(10.0))        # NT_FUZZ
ONE_FUZZ = f32(f32(1.0) + FUZZ)                            # (1.0f + NT_FUZZ)
BUILT = "simplex_built_n4"                                 # the 4-D simplex made by the native builder: 5 facets, a padded batch

# (scene, sizes) of the packet route, and of the general route; the forced cases run the packet scenes under NTRACER_FORCE_VAR=1
PACKET = [("cell600_n4", [(1, 1), (8, 8), (9, 7), (37, 21), (64, 48)]), ("cell120_n4", [(37, 21)]), ("simplex7_n7", [(9, 7), (37, 21)]),
          ("simplex10_n10", [(9, 7), (37, 21)]), ("feature5_n5", [(37, 21)]), (BUILT, [(17, 17)])]
GENERAL = [("feature11_n11", [(9, 7), (37, 21)]), ("feature16_n16", [(9, 7), (37, 21)]), ("lit12_n12", [(9, 7), (37, 21)])]
FORCED = [("cell120_n4", [(37, 21)]), ("simplex10_n10", [(37, 21)])]
COLOURED = ["cell120_n4", "feature5_n5", "feature16_n16"]
ALL_VIEWS = [(name, w, h) for name, sizes in PACKET + GENERAL for w, h in sizes]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(dimension, flat arrays, scene parameters or None, fov, (origin, axes) of camera k -> callable)"""
    if name == BUILT:
        from ntracer_amd import polytope
        nt, sc, dist = polytope.build_scene(["3", "3", "3"])
        flat = {k: np.array(v) for k, v in sc._flat.items()}
        flat["batch_size"] = 4
        n = 4
        o = np.array([0.05, -0.03, dist, 1e-4], f32)
        return n, flat, None, 0.8, lambda k: (o, np.eye(n, dtype=f32))
    g, n, flat = rq.scene(name)
    return n, flat, fx.params_of(g), ph.fov_of(name), lambda k: ph.camera(name, k)


def live_masks(flat, n):
    """bit l of byte b: lane l of batch b is no bytewise copy of an earlier lane of the batch"""
    recs = np.ascontiguousarray(flat["batch_recs"], f32).reshape(-1, 4, n * n + n + 1)
    out = np.zeros(len(recs), np.uint8)
    for b in range(len(recs)):
        for l in range(4):
            if not any(recs[b, l].tobytes() == recs[b, e].tobytes() for e in range(l)):
                out[b] |= 1 << l
    return out


def _simplices32(n, recs, o, D, scalar):
    """the batch rule (scalar False) or the scalar rule of every record [S] on every ray [R] from the origin o: accepted [S][R],
    t [S][R], fuzzed [S][R] -- accepted only thanks to NT_FUZZ"""
    S, R = len(recs), len(D)
    acc = np.zeros((S, R), bool)
    fuz = np.zeros((S, R), bool)
    tt = np.zeros((S, R), f32)
    with np.errstate(all="ignore"):
        for s0 in range(0, S, 1024):
            r = recs[s0:s0 + 1024]
            dd, N, p1 = r[:, 0], r[:, 1:1 + n], r[:, 1 + n:1 + 2 * n]
            E = r[:, 1 + 2 * n:].reshape(len(r), n - 1, n)
            denom = (N[:, 0, None] * D[None, :, 0]).astype(f32)
            no = (N[:, 0] * o[0]).astype(f32)
            for k in range(1, n):
                prod = (N[:, k, None] * D[None, :, k]).astype(f32)
                denom = (denom + prod).astype(f32)
                po = (N[:, k] * o[k]).astype(f32)
                no = (no + po).astype(f32)
            num = (-((no + dd).astype(f32))).astype(f32)
            t = (num[:, None] / denom).astype(f32)
            if scalar:
                ok = (denom != 0) & ~((t <= 0) | (t >= FLT_MAX))
            else:
                ok = (denom != 0) & (t >= 0) & (t != 0)
            pside = []
            for k in range(n):
                td = (t * D[None, :, k]).astype(f32)
                at = (o[k] + td).astype(f32)
                pside.append((p1[:, k, None] - at).astype(f32))
            tot = np.zeros(t.shape, f32)
            thanks = np.zeros(t.shape, bool)
            for e in range(n - 1):
                area = (E[:, e, 0, None] * pside[0]).astype(f32)
                for k in range(1, n):
                    prod = (E[:, e, k, None] * pside[k]).astype(f32)
                    area = (area + prod).astype(f32)
                if scalar:
                    ok &= ~((area < -FUZZ) | (area > ONE_FUZZ))
                else:
                    ok &= area >= -FUZZ
                thanks |= area < 0
                tot = (tot + area).astype(f32)
            ok &= tot <= ONE_FUZZ
            thanks |= tot > 1
            acc[s0:s0 + 1024] = ok
            fuz[s0:s0 + 1024] = ok & thanks
            tt[s0:s0 + 1024] = t
    return acc, tt, fuz


def crossings32(flat, o, D, live=None):
    """The crossing set of every ray D [R][n] from the origin o, by the rule's fp32 operations on the batches (the batch rule, the
    live mask `live` or live_masks applied) and the unbatched triangles (the scalar rule); rays with aabb_distance < 0 cross
    nothing.  A dict: count [R]; materials [R][n_materials], how many crossings of each material; nearest [R], the nearest
    accepted t (FLT_MAX: none); fuzzed [R], how many of the ray's accepted simplices were accepted only thanks to NT_FUZZ."""
    n = len(o)
    o, D = np.asarray(o, f32), np.ascontiguousarray(D, f32)
    R = len(D)
    n_mats = len(np.asarray(flat["materials"]).reshape(-1, 10))
    lo, hi = np.asarray(flat["aabb_start"], f32), np.asarray(flat["aabb_end"], f32)
    enter = ph.aabb_distance(lo, hi, o, D) >= 0
    count = np.zeros(R, np.int32)
    fuzzed = np.zeros(R, np.int32)
    mats = np.zeros((R, n_mats), np.int32)
    nearest = np.full(R, FLT_MAX, f32)
    rec_len = n * n + n + 1
    brecs = np.ascontiguousarray(flat["batch_recs"], f32).reshape(-1, rec_len)
    trecs = np.ascontiguousarray(flat["tri_recs"], f32).reshape(-1, rec_len)
    if live is None:
        live = live_masks(flat, n)
    lanes = ((np.asarray(live)[:, None] >> np.arange(4)[None]) & 1).astype(bool).reshape(-1)
    for recs, matids, alive, scalar in ((brecs, np.asarray(flat["batch_mats"]).reshape(-1), lanes, False),
                                        (trecs, np.asarray(flat["tri_mats"]).reshape(-1), np.ones(len(trecs), bool), True)):
        if not len(recs):
            continue
        acc, t, fuz = _simplices32(n, recs, o, D, scalar)
        acc &= alive[:, None] & enter[None]
        fuz &= acc
        count += acc.sum(axis=0).astype(np.int32)
        fuzzed += fuz.sum(axis=0).astype(np.int32)
        for m in range(n_mats):
            mats[:, m] += acc[matids == m].sum(axis=0).astype(np.int32)
        nearest = np.minimum(nearest, np.where(acc, t, FLT_MAX).min(axis=0)).astype(f32)
    return dict(count=count, materials=mats, nearest=nearest, fuzzed=fuzzed, enter=enter)


def solid_crossings(flat, o, D, enter):
    """The Solids by solid_cases' float64 rules on the local rays: (count [R], materials [R][n_materials], unsafe [R] -- how many of
    the ray's Solids decide within solid_cases.MARGIN)"""
    R = len(D)
    n_mats = len(np.asarray(flat["materials"]).reshape(-1, 10))
    count, unsafe, mats = np.zeros(R, np.int32), np.zeros(R, np.int32), np.zeros((R, n_mats), np.int32)
    types = np.asarray(flat["solid_types"]).reshape(-1)
    if not len(types):
        return count, mats, unsafe
    n, orient, inv, pos = sd._solid_parts(flat)
    o64, D64 = np.asarray(o, np.float64), np.asarray(D, np.float64)
    smats = np.asarray(flat["solid_mats"]).reshape(-1)
    for k, typ in enumerate(types):
        lo = np.repeat((inv[k] @ o64 - pos[k])[None], R, axis=0)
        ld = D64 @ inv[k].T
        dist, _, _, margin = sd._cube64(lo, ld) if typ == 1 else sd._sphere64(lo, ld)
        hit = (dist > 0) & enter
        count += hit
        mats[:, smats[k]] += hit
        unsafe += (margin < sd.MARGIN) & enter
    return count, mats, unsafe


@functools.lru_cache(maxsize=None)
def reference(name, width, height, k=0):
    """Of the view from golden camera k: count, materials, nearest, fuzzed (crossings32 plus the Solids), unsafe, odd = fuzzed +
    unsafe (primitives a ray, the slack of its count), ordinary = odd == 0, and B [H * W][3], the oracle's colour with an empty
    tree.  Rays in row-major order."""
    n, flat, params, fov, cam = scene(name)
    o, axes = cam(k)
    osc = ob.OracleScene(n, o, axes, fov)
    D = np.zeros((height * width, n), f32)
    for y in range(height):
        for x in range(width):
            D[y * width + x] = osc.primary_dir(x, y, width, height)
    r = crossings32(flat, o, D)
    sc, sm, unsafe = solid_crossings(flat, o, D, r["enter"])
    r["simplices"] = r["count"].copy()
    r["count"] = r["count"] + sc
    r["materials"] = r["materials"] + sm
    r["unsafe"] = unsafe
    r["odd"] = r["fuzzed"] + unsafe
    r["ordinary"] = r["odd"] == 0
    empty = dict(flat)
    empty["root"] = -1
    bsc = ob.OracleScene(n, o, axes, fov, flat=empty, params=params)
    ys, xs = np.divmod(np.arange(width * height), width)
    r["B"] = np.asarray(bsc.colors_at(xs, ys, width, height), f32)
    r["D"] = D
    for v in r.values():
        v.setflags(write=False)
    return r


def transmittance(flat, absorbance, tint):
    """T [n_materials][3] in np.float32, in the order of the rule: clamp01(1 - absorbance * (1 - tint * color))"""
    color = np.asarray(flat["materials"], f32).reshape(-1, 10)[:, :3]
    a, ti = f32(absorbance), f32(tint)
    tc = (ti * color).astype(f32)
    inner = (f32(1.0) - tc).astype(f32)
    ab = (a * inner).astype(f32)
    t = (f32(1.0) - ab).astype(f32)
    return np.minimum(np.maximum(t, f32(0.0)), f32(1.0)).astype(f32)


def expected_colour(name, width, height, absorbance, tint, k=0):
    """float64 [H * W][3]: B times the product of the fp32 transmittances of the ray's crossings"""
    n, flat, _, _, _ = scene(name)
    r = reference(name, width, height, k)
    T = transmittance(flat, absorbance, tint).astype(np.float64)
    out = r["B"].astype(np.float64)
    for m in range(len(T)):
        out = out * T[m][None, :] ** r["materials"][:, m, None]
    return out


def colour_bound(name, width, height, k=0):
    """(k + 2) * 2^-23 * max(1, max B) a ray: k fp32 multiplications of relative error <= 2^-24 each, doubled for the order"""
    r = reference(name, width, height, k)
    return (r["count"] + 2) * 2.0 ** -23 * max(1.0, float(r["B"].max()))
