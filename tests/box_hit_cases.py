"""Expected BoxScene hit records and face-line masks, shared by tests/test_box_hits_*.py and tests/test_box_lines_*.py, from the
oracle alone.

For every pixel (x, y) of a width x height view of the hypercube, nothing left out: the primary ray's direction d from the
oracle's own primary_dir, and the rule of include/ntracer_hip.h ("BoxScene hit buffers and face lines") restated in sequential
fp32 numpy, every operation rounded to fp32 on its own --
    for i = 0 .. n - 1 in ascending order, skipping d_i == 0:
        s = d_i < 0 ? 1 : -1;  dist = (s - o_i) / d_i
        if dist > 0 and for every j != i: not (|(d_j * dist) + o_j| > 1 + ROUNDING_FUZZ):
            dist >= FLT_MAX: no hit;  else: face (i, s) at dist;  stop
-- the colour that record stands for (|d_i| * (1, .5, .5) on a hit, the background rule on d_0 without one), which
test_box_hits_host.py holds against the oracle's nto_colors_at bit for bit, and the mask: a pixel with a hit gets, for each of its
four neighbours q inside the image, SILHOUETTE if q has no hit, nothing if q shows the same (item, lane) or is nearer, CREASE
otherwise.  Everything is computed once per process and never modified afterwards."""
import functools

import numpy as np

import fixtures as fx
import oracle_binding as ob

f32 = np.float32

SILHOUETTE, CREASE = 1, 2
FLT_MAX = f32(np.finfo(np.float32).max)
FUZZ = f32(f32(1.1920928955078125e-07) * f32(10.0))       # ROUNDING_FUZZ (src/tracer.hpp:25)
LIMIT = f32(f32(1.0) + FUZZ)

# compile-time-N kernels: the smallest, the bench's, the last with CompositeScene kernels beside it, the first without, the
# largest; run-time n: the first and the largest
DIMS = (3, 6, 10, 11, 24, 25, 64)
# fixtures.stress_cameras(n, default_rng(n)): every pixel on one face; the origin on a face's plane; three to seven faces,
# silhouette and edges; nothing hit -- and, as camera 4, fixtures.diagonal_camera just outside the circumsphere
STRESS = (7, 14, 58, 2)
CAMERAS = tuple(range(len(STRESS) + 1))
CAMERA_NAMES = ("one-face", "on-plane", "faces", "nothing", "diagonal")
# 1 x 1: no neighbour at all; one column, one row; a partial tile; more than one wave's rows; and one view wider and taller than
# the fused kernel's 64 x 32 tile both ways, so that halo records of neighbouring blocks are read in both directions
SIZES = [(1, 1), (1, 7), (7, 1), (9, 7), (37, 21)]
BIG = (70, 37)
ALL_SIZES = SIZES + [BIG]
FOV = 0.8


def diagonal_distance(n):
    """outside the circumsphere (radius sqrt(n)), near enough that the cube still fills a good part of the view"""
    return float(np.sqrt(n)) + 0.75


@functools.lru_cache(maxsize=None)
def camera(n, k):
    """(origin [n], axes [n][n]) of camera k of dimension n"""
    if k < len(STRESS):
        o, a = fx.stress_cameras(n, np.random.default_rng(n))[STRESS[k]]
    else:
        o, a = fx.diagonal_camera(n, diagonal_distance(n), np.random.default_rng(n))
    o, a = np.ascontiguousarray(o, f32), np.ascontiguousarray(a, f32)
    o.setflags(write=False)
    a.setflags(write=False)
    return o, a


def oracle_scene(n, k):
    o, a = camera(n, k)
    return ob.OracleScene(n, o, a, fov=FOV)


def records_of(o, D):
    """the rule on origin o [n] and unit directions D [P][n]: (dist, item, lane) [P]"""
    o, D = np.asarray(o, f32), np.asarray(D, f32)
    P, n = D.shape
    dist_out = np.full(P, FLT_MAX, f32)
    item = np.full(P, -1, np.int32)
    lane = np.full(P, -1, np.int32)
    done = np.zeros(P, bool)
    with np.errstate(all="ignore"):
        for i in range(n):
            di = D[:, i]
            s = np.where(di < 0, f32(1.0), f32(-1.0)).astype(f32)
            dist = ((s - o[i]).astype(f32) / di).astype(f32)
            p = ((D * dist[:, None]).astype(f32) + o[None, :]).astype(f32)
            inside = ~(np.abs(p) > LIMIT)
            inside[:, i] = True
            ok = ~done & (di != 0) & (dist > 0) & inside.all(axis=1)
            hit = ok & ~(dist >= FLT_MAX)
            dist_out[hit] = dist[hit]
            item[hit] = i
            lane[hit] = (s[hit] > 0).astype(np.int32)
            done |= ok
    return dist_out, item, lane


def colors_of(D, item):
    """the colours the records stand for: box_scene::calculate_color (tracer.hpp:101-113) on d and the face"""
    D = np.asarray(D, f32)
    P = len(D)
    out = np.zeros((P, 3), f32)
    hit = item >= 0
    shade = np.abs(D[np.arange(P), np.where(hit, item, 0)]).astype(f32)
    out[hit, 0] = (shade[hit] * f32(1.0)).astype(f32)
    out[hit, 1] = (shade[hit] * f32(0.5)).astype(f32)
    out[hit, 2] = out[hit, 1]
    d0 = D[:, 0]
    pos = ~hit & (d0 > 0)
    neg = ~hit & ~(d0 > 0)
    out[pos] = d0[pos, None]
    out[neg, 0] = f32(0.0)
    out[neg, 1] = -d0[neg]
    out[neg, 2] = -d0[neg]
    return out


def mask_of(dist, item, lane):
    """(mask [H][W] uint8 with every kind, counts of the pairs): the rule written out on records [H][W]"""
    height, width = item.shape
    mask = np.zeros((height, width), np.uint8)
    counts = dict(silhouette=0, edge=0, farther=0, same=0, equal_dist=0)
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
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
        edge = hit & (iq >= 0) & ~same & ~farther
        mask[ys, xs] |= (np.where(sil, SILHOUETTE, 0) | np.where(edge, CREASE, 0)).astype(np.uint8)
        counts["silhouette"] += int(sil.sum())
        counts["edge"] += int(edge.sum())
        counts["farther"] += int(farther.sum())
        counts["same"] += int(same.sum())
        counts["equal_dist"] += int((edge & (dp == dq)).sum())
    return mask, counts


def normals_of(n, item, lane):
    """the outward normals s * e_i as rows [H][W][n] (zero without a hit)"""
    out = np.zeros(item.shape + (n,), f32)
    ys, xs = np.nonzero(item >= 0)
    out[ys, xs, item[ys, xs]] = np.where(lane[ys, xs] > 0, f32(1.0), f32(-1.0))
    return out


@functools.lru_cache(maxsize=None)
def expected(n, k, width, height):
    """dict of the view of camera k at dimension n: dirs [H][W][n], dist / item / lane [H][W], colors [H][W][3], mask [H][W] (every
    kind; AND it with the setting's), counts, faces (the distinct (item, lane) seen)"""
    osc = oracle_scene(n, k)
    D = np.stack([osc.primary_dir(x, y, width, height) for y in range(height) for x in range(width)]).astype(f32)
    o, _ = camera(n, k)
    dist, item, lane = records_of(o, D)
    colors = colors_of(D, item).reshape(height, width, 3)
    dist, item, lane = dist.reshape(height, width), item.reshape(height, width), lane.reshape(height, width)
    mask, counts = mask_of(dist, item, lane)
    e = dict(dirs=D.reshape(height, width, n), dist=dist, item=item, lane=lane, colors=colors, mask=mask)
    for a in e.values():
        a.setflags(write=False)
    e["counts"] = counts
    e["faces"] = tuple(sorted({(int(i), int(l)) for i, l in zip(item.ravel(), lane.ravel()) if i >= 0}))
    return e


def records(n, k, width, height):
    """the expected records as the library lays them out: [H * W][4] int32 (dist's bits, item, lane, 0)"""
    e = expected(n, k, width, height)
    out = np.zeros((height * width, 4), np.int32)
    out[:, 0] = e["dist"].reshape(-1).view(np.int32)
    out[:, 1] = e["item"].reshape(-1)
    out[:, 2] = e["lane"].reshape(-1)
    return out


def view_id(v):
    n, k, (w, h) = v
    return "n%d-%s-%dx%d" % (n, CAMERA_NAMES[k], w, h)


def views(n):
    return [(n, k, size) for k in CAMERAS for size in ALL_SIZES]
