"""The reference of the hit-layer tests (tests/test_hit_layers_host.py, tests/test_hit_layers_gpu.py): nothing here comes from the
code under test.

The crossing set of every ray is xray_cases' restatement of the rule of include/ntracer_hip.h: xc._simplices32 gives the accepted
simplices and their fp32 t (the batch rule under xc.live_masks, the scalar rule for unbatched triangles), and the Solids go through
solid_cases' float64 rules on their local rays, as xc.solid_crossings sends them.  The set is ordered by the rule's key -- t, then
the leaf-item code, then the lane -- and cut at `layers`.

A ray is compared only if it is `ordinary` in xc.reference and no Solid crossing among its first layers + 1 lies within
1e-4 * max(1, t) of a neighbour in the list: the kernel's Solid t is fp32 and this one float64, so their order is not decidable
closer than that.  Solid layers compare dist within 1e-5 * max(1, t), the project's composite tolerance; everything else compares
bit for bit.  test_hit_layers_host.py holds the left-out share of every view to 1 %.  Computed once per process, never modified."""
import functools

import numpy as np

import solid_cases as sd
import xray_cases as xc

f32 = np.float32
FLT_MAX = xc.FLT_MAX
LAYERS_MAX = 8
KEPT = LAYERS_MAX + 2                  # the entries of a ray's list that are kept: layers + 1 and the neighbour behind them
SOLID_ORDER = 1e-4                     # a Solid's place in the order is not decidable closer than this, relative to max(1, t)
SOLID_DIST = 1e-5                      # the project's composite tolerance, relative to max(1, t)

# (scene, width, height, layers) of the packet route and of the general one, golden camera 0 throughout; FORCED runs under
# NTRACER_FORCE_VAR=1
PACKET = [("cell600_n4", 1, 1, 4), ("cell600_n4", 9, 7, 4), ("cell600_n4", 37, 21, 4),
          ("cell120_n4", 37, 21, 1), ("cell120_n4", 37, 21, 2), ("cell120_n4", 37, 21, 3), ("cell120_n4", 37, 21, 8),
          ("simplex10_n10", 37, 21, 4), ("feature5_n5", 37, 21, 4), (xc.BUILT, 17, 17, 4)]
GENERAL = [(name, w, h, layers) for name in ("feature11_n11", "feature16_n16") for w, h in ((9, 7), (37, 21)) for layers in (2, 8)]
FORCED = [("cell120_n4", 37, 21, 8), ("simplex10_n10", 37, 21, 2)]
VIEWS = sorted(set((name, w, h) for name, w, h, _ in PACKET + GENERAL))


@functools.lru_cache(maxsize=None)
def lists(name, width, height):
    """Of the view from golden camera 0: the first KEPT entries of every ray's ordered crossing list -- t [R][KEPT] in
    float64 (an fp32 t exactly, or a Solid's float64 distance; inf: no such entry), item, lane [R][KEPT] (-1: none), solid
    [R][KEPT] -- and count [R], the length of the whole list.  Rays in row-major order."""
    n, flat, _, _, cam = xc.scene(name)
    o = np.asarray(cam(0)[0], f32)
    r = xc.reference(name, width, height)
    D, enter = r["D"], r["enter"]
    R = len(D)
    rec_len = n * n + n + 1
    ts, items, lanes, accs, solids = [], [], [], [], []
    brecs = np.ascontiguousarray(flat["batch_recs"], f32).reshape(-1, rec_len)
    if len(brecs):
        live = ((np.asarray(xc.live_masks(flat, n))[:, None] >> np.arange(4)[None]) & 1).astype(bool).reshape(-1)
        acc, t, _ = xc._simplices32(n, brecs, o, D, False)
        s = np.arange(len(brecs))
        ts.append(t.astype(np.float64)); accs.append(acc & live[:, None] & enter[None])
        items.append((s // 4) << 2); lanes.append(s % 4); solids.append(np.zeros(len(s), bool))
    trecs = np.ascontiguousarray(flat["tri_recs"], f32).reshape(-1, rec_len)
    if len(trecs):
        acc, t, _ = xc._simplices32(n, trecs, o, D, True)
        s = np.arange(len(trecs))
        ts.append(t.astype(np.float64)); accs.append(acc & enter[None])
        items.append((s << 2) | 1); lanes.append(np.full(len(s), -1)); solids.append(np.zeros(len(s), bool))
    types = np.asarray(flat["solid_types"]).reshape(-1)
    if len(types):
        # xc.solid_crossings' loop, keeping the distances it decides by
        _, _, inv, pos = sd._solid_parts(flat)
        o64, D64 = np.asarray(o, np.float64), np.asarray(D, np.float64)
        for j, typ in enumerate(types):
            lo = np.repeat((inv[j] @ o64 - pos[j])[None], R, axis=0)
            ld = D64 @ inv[j].T
            dist, _, _, _ = sd._cube64(lo, ld) if typ == 1 else sd._sphere64(lo, ld)
            ts.append(np.asarray(dist, np.float64)[None]); accs.append(((dist > 0) & enter)[None])
            items.append(np.array([(j << 2) | 2])); lanes.append(np.array([-1])); solids.append(np.array([True]))
    out_t = np.full((R, KEPT), np.inf)
    out_item = np.full((R, KEPT), -1, np.int32)
    out_lane = np.full((R, KEPT), -1, np.int32)
    out_solid = np.zeros((R, KEPT), bool)
    count = np.zeros(R, np.int32)
    if ts:
        t, acc = np.concatenate(ts), np.concatenate(accs)
        item, lane, solid = np.concatenate(items), np.concatenate(lanes), np.concatenate(solids)
        count = acc.sum(axis=0).astype(np.int32)
        for ray in np.nonzero(count)[0]:
            p = np.nonzero(acc[:, ray])[0]
            p = p[np.lexsort((lane[p], item[p], t[p, ray]))][:KEPT]
            out_t[ray, :len(p)], out_item[ray, :len(p)], out_lane[ray, :len(p)], out_solid[ray, :len(p)] = t[p, ray], item[p], lane[p], solid[p]
    out = dict(t=out_t, item=out_item, lane=out_lane, solid=out_solid, count=count, ordinary=r["ordinary"])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, width, height, layers):
    """The records of the view, [layers][R]: dist (fp32; FLT_MAX: no such layer), item, lane, solid, and per ray count and
    compared -- the rays that are held to the records"""
    ls = lists(name, width, height)
    t, solid = ls["t"], ls["solid"]
    # a Solid among the first layers + 1 within SOLID_ORDER of a neighbour in the list
    with np.errstate(invalid="ignore"):
        gap = np.abs(t[:, 1:] - t[:, :-1]) <= SOLID_ORDER * np.maximum(1.0, np.minimum(t[:, 1:], t[:, :-1]))
    gap &= np.isfinite(t[:, 1:])
    near = np.zeros(t.shape, bool)
    near[:, 1:] |= gap
    near[:, :-1] |= gap
    undecided = (near & solid)[:, :layers + 1].any(axis=1)
    there = np.isfinite(t[:, :layers])
    with np.errstate(over="ignore"):
        dist = np.where(there, t[:, :layers], FLT_MAX).astype(f32)
    out = dict(dist=dist.T.copy(), item=ls["item"][:, :layers].T.copy(), lane=ls["lane"][:, :layers].T.copy(),
               solid=solid[:, :layers].T.copy(), count=ls["count"], compared=ls["ordinary"] & ~undecided)
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_records(records, name, width, height, layers, label):
    """int32 [layers][height][width][4] against expected(); prints what it holds the records to before it asserts"""
    e = expected(name, width, height, layers)
    rec = np.asarray(records)
    assert rec.dtype == np.int32 and rec.shape == (layers, height, width, 4), (label, rec.dtype, rec.shape)
    rec = rec.reshape(layers, height * width, 4)
    dist, item, lane, count = rec[..., 0].view(f32), rec[..., 1], rec[..., 2], rec[..., 3]
    cmp = e["compared"]
    print("%s %dx%d layers %d: %d of %d rays compared, counts up to %d, %d rays cut" % (
        label, width, height, layers, int(cmp.sum()), len(cmp), int(e["count"].max(initial=0)), int((e["count"] > layers).sum())))
    assert (count == count[0][None]).all(), "%s: the count differs between the layers of a pixel" % label
    bad = np.nonzero(cmp & (count[0] != e["count"]))[0]
    assert len(bad) == 0, "%s: %d compared rays with another count, first ray %d: got %d, expected %d" % (
        label, len(bad), bad[0], count[0][bad[0]], e["count"][bad[0]])
    for l in range(layers):
        for what, got, want in (("item", item[l], e["item"][l]), ("lane", lane[l], e["lane"][l])):
            bad = np.nonzero(cmp & (got != want))[0]
            assert len(bad) == 0, "%s layer %d: %d rays with another %s, first ray %d: got %d, expected %d" % (
                label, l, len(bad), what, bad[0], got[bad[0]], want[bad[0]])
        exact = cmp & ~e["solid"][l]
        bad = np.nonzero(exact & (dist[l].view(np.int32) != e["dist"][l].view(np.int32)))[0]
        assert len(bad) == 0, "%s layer %d: %d rays with other bits of dist, first ray %d: got %r, expected %r" % (
            label, l, len(bad), bad[0], dist[l][bad[0]], e["dist"][l][bad[0]])
        sol = cmp & e["solid"][l]
        if sol.any():
            want = e["dist"][l][sol].astype(np.float64)
            err = np.abs(dist[l][sol].astype(np.float64) - want) / np.maximum(1.0, want)
            print("  layer %d: %d Solid records, largest relative error %.3g" % (l, int(sol.sum()), err.max()))
            assert (err <= SOLID_DIST).all(), "%s layer %d: a Solid's dist is off by %g of max(1, t)" % (label, l, err.max())
