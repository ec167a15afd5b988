"""Batched ray queries (nt_intersect_rays / nt_occludes_rays and their _device forms, KDNode.intersects / occludes) against
the oracle's nto_kd_intersects / nto_kd_occludes: every ray of every set is compared, none is left out.

The oracle runs in the GPU's mode (ray_query_cases.batches).  item, lane, n_transparent and blocked must be equal for every
ray; dist within 1e-5 (1 + |dist|) and normals within 1e-5, the project's composite tolerance -- by the arithmetic contract
there is no pow on this path, so the observed difference is 0.  The ray sets, per scene: (A) the golden
cameras' golden pixels, (B) second legs from the oracle's hit points towards seeded random points of the scene's box, with
the leg's length as `distance` and the hit as the skip, run as occlusion and as closest-hit queries, (C) 500 seeded edge
cases from inside the box with zero direction components, origins exactly on the root's split plane and t_near / t_far
windows at 0.5x and 1.5x of the unwindowed distance.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C
import threading

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.wrapper import NTracer

pytestmark = pytest.mark.gpu

TOL = 1e-5
FLT_MAX = rq.FLT_MAX
LAUNCHES = (1, 63, 64, 65, 257)         # a partial wave, a wave, a partial block, more than one block
QUERY_SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR")     # what a query routes on

# floors by the oracle alone, so that no case can pass on all misses: opaque hits on (A), rays of (A) with a transparent
# hit, blocked second legs
MIN_OPAQUE = 25
MIN_TRANSPARENT = {"feature5_n5": 20, "feature11_n11": 20}
MIN_BLOCKED = {"cell600_n4": 10, "feature5_n5": 10, "lit12_n12": 10}


def _scene(case, mp):
    name, env = case
    sup.set_switches(mp, QUERY_SWITCHES, env)
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat)


def _check_intersect(got, ref, sl, label, normals=True):
    item = np.where(got["kind"] < 0, -1, (got["index"] << 2) | got["kind"])
    for k, g in (("item", item), ("lane", got["lane"]), ("n_transparent", got["n_transparent"])):
        bad = np.nonzero(g != ref[k][sl])[0]
        assert len(bad) == 0, "%s: %s differs on %d rays, first %d: got %r, oracle %r" % (label, k, len(bad), bad[0], g[bad[0]], ref[k][sl][bad[0]])
    hit = item >= 0
    rd = ref["dist"][sl]
    assert np.array_equal(got["dist"][~hit], rd[~hit]), label               # FLT_MAX where nothing was hit
    err = np.abs(got["dist"][hit].astype(np.float64) - rd[hit]) / (1.0 + np.abs(rd[hit].astype(np.float64)))
    worst = float(err.max()) if hit.any() else 0.0
    assert worst <= TOL, "%s: dist off by %g" % (label, worst)
    nworst = 0.0
    if normals:
        for k in ("normal_origin", "normal"):
            e = np.abs(got[k][hit].astype(np.float64) - ref[k][sl][hit])
            nworst = max(nworst, float(e.max()) if hit.any() else 0.0)
            assert nworst <= TOL, "%s: %s off by %g" % (label, k, nworst)
            assert not got[k][~hit].any(), "%s: %s written for a ray without an opaque hit" % (label, k)
    return worst, nworst


def _check_occludes(got, ref, sl, label):
    for k in ("blocked", "n_transparent"):
        bad = np.nonzero(np.asarray(got[k]) != ref[k][sl])[0]
        assert len(bad) == 0, "%s: %s differs on %d rays, first %d" % (label, k, len(bad), bad[0])


def _single_item_oracle(name, item):
    """a one-leaf scene holding only `item`, every material opaque"""
    g, n, flat = rq.scene(name)
    f = dict(flat)
    f.update(root=0, node_axis=np.array([-1], np.int32), node_split=np.zeros(1, np.float32), node_left=np.zeros(1, np.int32),
             node_right=np.ones(1, np.int32), items=np.array([item], np.int32))
    m = np.array(flat["materials"], np.float32).copy()
    m[:, 6] = 1.0
    f["materials"] = m
    return rq.Oracle(n, f, True, False)


def _check_lists(b, name, got, ref_n, label):
    """the transparent list is the prefix the walk kept, and each listed hit is that primitive's own answer"""
    tl = got["transparent"]
    cap = tl.shape[1]
    kept = np.minimum(ref_n, cap)
    used = np.arange(cap)[None, :] < kept[:, None]
    assert (tl[~used][:, 1] == -1).all(), label
    rays, slots = np.nonzero(used)
    oracles = {}
    for r, s in zip(rays, slots):
        dist = float(tl[r, s, 0:1].view(np.float32)[0])
        item, lane = int(tl[r, s, 1]), int(tl[r, s, 2])
        if item not in oracles:
            oracles[item] = _single_item_oracle(name, item)
        one = oracles[item].intersects(b.i_origins[r:r + 1], b.i_directions[r:r + 1], [-FLT_MAX], [FLT_MAX], b.i_skip_item[r:r + 1],
                                       b.i_skip_lane[r:r + 1])
        assert one["item"][0] == item and one["lane"][0] == lane, (label, r, s, item, lane, one["item"][0], one["lane"][0])
        assert abs(one["dist"][0] - dist) <= TOL * (1 + abs(dist)), (label, r, s, dist, one["dist"][0])
    return len(rays)


@pytest.mark.parametrize("case", rq.CASES, ids=rq.case_id)
def test_queries_equal_the_oracle(case):
    name, env = case
    b = rq.batches(case)
    ref, oref = b.i_ref, b.o_ref
    count = len(b.i_origins)
    A = b.i_slices["A"]
    # ---- floors, by the oracle alone
    first = slice(0, b.per_frame)
    assert (ref["item"][first] >= 0).sum() >= MIN_OPAQUE, name
    if name in MIN_TRANSPARENT:
        per_frame = (ref["n_transparent"][A] > 0).reshape(-1, b.per_frame).sum(axis=1)
        frame9 = list(rq.scene(name)[0]["frames"]).index(9)
        assert per_frame[frame9] >= MIN_TRANSPARENT[name], (name, per_frame)
        if name == "feature5_n5":
            assert (ref["n_transparent"][A] > 1).any()                   # frame 9: some rays with two
    if name in MIN_BLOCKED:
        assert oref["blocked"][b.o_slices["B"]].sum() >= MIN_BLOCKED[name], name
    if name == "feature16_n16":
        assert (oref["n_transparent"][b.o_slices["B"]] > 0).sum() >= 10
    if name == "cell600_n4":
        # the far-child quirk of _occludes (tracer.hpp:1298): with distance = FLT_MAX a blocker beyond the first split the ray
        # crosses inside its window is never looked at.  From the first golden camera not one of the 1 686 primary rays that
        # hit something is "blocked"; over the five cameras 617 of 8 423 are (those whose first leaf already holds the blocker)
        assert (ref["item"][first] >= 0).sum() == 1686
        assert oref["blocked"][first].sum() == 0
        assert oref["blocked"][b.o_slices["A"]].sum() < (ref["item"][A] >= 0).sum() // 2

    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        args = (b.i_origins, b.i_directions, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)
        # ---- closest hits: the whole batch (normals and the transparent lists with it), then the same rays in small launches
        full = sc.intersect_rays(*args, normals=True, max_transparent=4)
        worst = _check_intersect(full, ref, slice(0, count), rq.case_id(case) + " all")
        print("%s: %d rays, dist error %g, normal error %g" % (rq.case_id(case), count, worst[0], worst[1]))
        for k in LAUNCHES:
            part = sc.intersect_rays(*(a[:k] for a in args), normals=True)
            _check_intersect(part, ref, slice(0, k), "%s first %d" % (rq.case_id(case), k))
        # max_transparent 0, 1, 4: no list, and lists that are prefixes of each other and of the walk's
        listed = _check_lists(b, name, full, ref["n_transparent"], rq.case_id(case))
        one = sc.intersect_rays(*args, max_transparent=1)
        assert "transparent" not in sc.intersect_rays(*(a[:65] for a in args))
        assert np.array_equal(one["transparent"][:, 0], full["transparent"][:, 0])
        _check_intersect(one, ref, slice(0, count), rq.case_id(case) + " max_transparent=1", normals=False)
        if name in MIN_TRANSPARENT:
            assert listed >= MIN_TRANSPARENT[name]
        # ---- occlusion: the whole batch and one small launch
        oargs = (b.o_origins, b.o_directions, b.o_distance, b.o_t_near, b.o_t_far, b.o_skip_item, b.o_skip_lane)
        ofull = sc.occludes_rays(*oargs, max_transparent=4)
        _check_occludes(ofull, oref, slice(0, len(b.o_origins)), rq.case_id(case) + " occlusion")
        kept = np.minimum(oref["n_transparent"], 4)
        assert ((ofull["transparent"][:, :, 1] >= 0).sum(axis=1) == kept).all()
        for k in LAUNCHES:
            _check_occludes(sc.occludes_rays(*(a[:k] for a in oargs)), oref, slice(0, k), "%s occlusion, first %d" % (rq.case_id(case), k))

        # ---- the _device forms agree with the host forms bit for bit
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        t = [torch.from_numpy(np.array(a)).to(dev) for a in args]
        dfull = sc.intersect_rays(*t, normals=True, max_transparent=4)
        ot = [torch.from_numpy(np.array(a)).to(dev) for a in oargs]
        dofull = sc.occludes_rays(*ot, max_transparent=4)
        torch.cuda.synchronize()
        bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
        for k in full:
            assert np.array_equal(bits(dfull[k].cpu().numpy()), bits(full[k])), (rq.case_id(case), k)
        for k in ofull:
            assert np.array_equal(bits(dofull[k].cpu().numpy()), bits(ofull[k])), (rq.case_id(case), k)


@pytest.mark.parametrize("env", [{}, {"NTRACER_FORCE_VAR": "1"}], ids=["fixed_n", "run_time_n"])
def test_capped_grid_strides_and_the_scene_is_held(env):
    """feature5_n5's closest-hit walk keeps a `checked` column per resident lane, so its grid is capped (1024 blocks of 256
    lanes, 4096 of 64 at run-time n) and the blocks stride: the same rays, tiled to eight times 262 144 and a ragged end.
    The host query holds the scene while it runs (Scene.locked, LockedError from a setter) and lets go of it afterwards.
    The query has no hook to look out from, so the window is watched from a second thread; it is made wide for that --
    some 300 MB cross PCIe inside it, tens of milliseconds against a microsecond a look."""
    case = ("feature5_n5", env)
    b = rq.batches(case)
    count = 8 * 262144 + 300
    reps = count // len(b.i_origins) + 1
    tile = lambda a: np.ascontiguousarray(np.concatenate([a] * reps)[:count])
    args = [tile(a) for a in (b.i_origins, b.i_directions, b.i_t_near, b.i_t_far, b.i_skip_item, b.i_skip_lane)]
    ref = {k: tile(v) for k, v in b.i_ref.items()}
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        assert not sc.locked
        sc.intersect_rays(*(a[:1] for a in args))                # (the scene is on the device before the window opens)
        out, looks, held, refused = {}, 0, 0, 0
        fov = sc.fov
        worker = threading.Thread(target=lambda: out.update(sc.intersect_rays(*args, normals=True, max_transparent=4)))
        worker.start()
        while worker.is_alive():
            looks += 1
            if sc.locked:
                held += 1
                try:
                    sc.set_fov(fov)
                except _lib.LockedError:
                    refused += 1
        worker.join()
        assert held > 0 and refused > 0, "the scene was never seen held during the query (%d looks)" % looks
        assert not sc.locked
        sc.set_fov(fov)
        _check_intersect(out, ref, slice(0, count), "feature5_n5 tiled")


def _tri(nt, t, mat):
    return nt.Triangle(t["p1"], t["face_normal"], t["edge_normals"], mat)


def test_known_answer_through_the_python_objects():
    """lib/ntracer/tests/test.py:303-363 as the reference's script has it: one hit, the very object put in the leaf"""
    ka = fx.known_answer()
    nt = NTracer(3)
    from ntracer_amd import Material
    mat = Material((1, 1, 1))
    primitives = [_tri(nt, t, mat) for t in ka["triangles"]]

    def node(d):
        if d is None:
            return None
        if "leaf" in d:
            return nt.KDLeaf([primitives[i] for i in d["leaf"]])
        return nt.KDBranch(d["branch"]["axis"], d["branch"]["split"], node(d["branch"]["left"]), node(d["branch"]["right"]))

    scene = nt.CompositeScene(nt.AABB(ka["aabb"]["start"], ka["aabb"]["end"]), node(ka["tree"]))
    scene.set_fov(float(ka["fov"]))
    hits = scene.root.intersects(tuple(ka["ray"]["origin"]), tuple(ka["ray"]["direction"]))
    assert len(hits) == 1
    assert hits[0].primitive is primitives[4]
    assert hits[0].batch_index == -1
    ref = ob.OracleScene(3, [0, 0, 0], np.eye(3), flat=fx.known_answer_flat(ka)).kd_intersects(ka["ray"]["origin"], ka["ray"]["direction"])
    assert abs(hits[0].dist - ref["dist"]) <= TOL * (1 + abs(ref["dist"]))
    assert np.abs(np.asarray(list(hits[0].origin)) - ref["origin"]).max() <= TOL
    assert np.abs(np.asarray(list(hits[0].normal)) - ref["normal"]).max() <= TOL
    # the skip: the ray leaves from what it hit and finds nothing else in front
    again = scene.root.intersects(tuple(ka["ray"]["origin"]), tuple(ka["ray"]["direction"]), source=primitives[4])
    assert all(h.primitive is not primitives[4] for h in again)
    # a scene from flat arrays answers with the objects its `root` exposes
    flat_scene = tracern.CompositeScene.from_flat(3, fx.known_answer_flat(ka))
    h2 = flat_scene.root.intersects(ka["ray"]["origin"], ka["ray"]["direction"])
    assert len(h2) == 1 and h2[0].primitive is flat_scene.root.right[0]
    # ... on its own handle: a root that `root` materialised is the scene's root like one the scene was made from
    assert flat_scene.root._owner() is flat_scene and flat_scene.root._private is None
    assert scene.root._owner() is scene and scene.root._private is None


def test_transparent_hits_through_the_python_objects():
    """KDNode.intersects / occludes on feature5_n5 (transparent batches, triangles and Solids): the RayIntersection objects
    of the transparent hits -- whose normal rays the binding works out on the host, in fp32 in the reference's order --
    against the oracle's answer for a one-leaf scene holding only that item with an opaque material: dist, origin and
    normal within the composite tolerance, `primitive` the object `root` exposes for the item, batch_index its lane."""
    name = "feature5_n5"
    b = rq.batches((name, {}))
    g, n, flat = rq.scene(name)
    ref, oref = b.i_ref, b.o_ref
    # rays with transparent hits, a few for every opaque-hit item they end on (so that every listed kind comes up)
    rays, per_item = [], {}
    for r in np.nonzero(ref["n_transparent"] > 0)[0]:
        key = (int(ref["item"][r]), int(ref["n_transparent"][r]))
        if per_item.get(key, 0) < 3:
            per_item[key] = per_item.get(key, 0) + 1
            rays.append(int(r))
    occl = [int(r) for r in np.nonzero((oref["n_transparent"] > 0) & ~oref["blocked"])[0][:12]]
    assert len(rays) >= 10 and len(occl) >= 5
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp)
        root = sc.root
        oracles, kinds = {}, set()

        def check(h, o, d, skip_item, skip_lane):
            item = sc._item_of(h.primitive)
            assert item >= 0 and h.primitive is sc._object_of(item & 3, item >> 2)
            if item not in oracles:
                oracles[item] = _single_item_oracle(name, item)
            one = oracles[item].intersects(o[None], d[None], [-FLT_MAX], [FLT_MAX], [skip_item], [skip_lane])
            assert one["item"][0] == item and one["lane"][0] == h.batch_index, (item, h.batch_index, one["lane"][0])
            assert abs(one["dist"][0] - h.dist) <= TOL * (1 + abs(h.dist))
            assert np.abs(np.asarray(list(h.origin), np.float32) - one["normal_origin"][0]).max() <= TOL, (item, list(h.origin), one["normal_origin"][0])
            assert np.abs(np.asarray(list(h.normal), np.float32) - one["normal"][0]).max() <= TOL, (item, list(h.normal), one["normal"][0])
            kinds.add(item & 3)

        for r in rays:
            o, d = b.i_origins[r], b.i_directions[r]
            source = sc._object_of(int(b.i_skip_item[r]) & 3, int(b.i_skip_item[r]) >> 2) if b.i_skip_item[r] >= 0 else None
            hits = root.intersects(o, d, float(b.i_t_near[r]), float(b.i_t_far[r]), source, int(b.i_skip_lane[r]))
            opaque = ref["item"][r] >= 0
            assert len(hits) == ref["n_transparent"][r] + (1 if opaque else 0)
            if opaque:
                assert sc._item_of(hits[-1].primitive) == ref["item"][r] and hits[-1].batch_index == ref["lane"][r]
            for h in hits[:ref["n_transparent"][r]]:
                check(h, o, d, int(b.i_skip_item[r]), int(b.i_skip_lane[r]))
        for r in occl:
            o, d = b.o_origins[r], b.o_directions[r]
            source = sc._object_of(int(b.o_skip_item[r]) & 3, int(b.o_skip_item[r]) >> 2) if b.o_skip_item[r] >= 0 else None
            blocked, hits = root.occludes(o, d, float(b.o_distance[r]), float(b.o_t_near[r]), float(b.o_t_far[r]), source, int(b.o_skip_lane[r]))
            assert blocked is False and len(hits) == oref["n_transparent"][r]
            for h in hits:
                check(h, o, d, int(b.o_skip_item[r]), int(b.o_skip_lane[r]))
        assert root._private is None
        print("transparent hits checked on items of kinds", sorted(kinds))


def test_far_child_quirk_through_the_python_objects():
    """SURVEY appendix A / tests/test_oracle_golden.py: occludes is False from one side although B blocks the ray at t = 3
    (tracer.hpp:1298) and True from the other, while intersects finds B at 3.0.  The branch is no scene's root: it answers
    from a handle of its own."""
    nt = NTracer(3)
    from ntracer_amd import Material
    mat = Material((1, 1, 1))
    B = nt.Triangle((1, -1, -1), (1, 0, 0), [(0, -0.25, 0), (0, 0, -0.25)], mat)
    A = nt.Triangle((-1, 5, -1), (1, 0, 0), [(0, -0.25, 0), (0, 0, -0.25)], mat)
    root = nt.KDBranch(0, 0, nt.KDLeaf([A]), nt.KDLeaf([B]))
    hits = root.intersects((-2, 0, -.2), (1, 0, 0))
    assert len(hits) == 1 and hits[0].primitive is B and abs(hits[0].dist - 3.0) < 1e-6
    for dist in (10.0, 1.5, 3.4e38, None):
        assert root.occludes((-2, 0, -.2), (1, 0, 0), dist) == (False, [])
    assert root.occludes((2, 0, -.2), (-1, 0, 0), 10.0) == (True, None)
    assert root._private is not None and root._owner is None


def test_abort_word_raised_before_the_call_nothing_is_written():
    import torch
    case = ("cell600_n4", {})
    b = rq.batches(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        dev = torch.device("cuda", torch.cuda.current_device())
        count = 1000
        o = torch.from_numpy(np.array(b.i_origins[:count])).to(dev)
        d = torch.from_numpy(np.array(b.i_directions[:count])).to(dev)
        hits = torch.full((count, 4), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        normals = torch.full((count, 4), 7.0, dtype=torch.float32, device=dev)
        word = torch.ones(1, dtype=torch.int32, device=dev)
        rays = _lib.NtRayBatch()
        rays.count, rays.origins, rays.directions = count, o.data_ptr(), d.data_ptr()
        res = _lib.NtRayResults()
        res.hits, res.normal_origin = hits.data_ptr(), normals.data_ptr()
        opts = _lib.NtRenderOpts()
        opts.device = dev.index
        opts.abort_device = word.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream
        for fn in (_lib.lib().nt_intersect_rays_device, _lib.lib().nt_occludes_rays_device):
            assert fn(sc._handle, C.byref(rays), C.byref(res), C.byref(opts), stream) == _lib.NT_OK
        torch.cuda.synchronize()
        assert bool((hits == 0x5a5a5a5a).all()) and bool((normals == 7.0).all())
        # every other field of the options must be 0
        opts.collect_stats = 1
        assert _lib.lib().nt_intersect_rays_device(sc._handle, C.byref(rays), C.byref(res), C.byref(opts), stream) == _lib.NT_E_INVALID


def test_an_empty_scene_answers_no_hit_and_not_blocked():
    g, n, flat = rq.scene("cell600_n4")
    f = dict(flat)
    f["root"] = -1
    b = rq.batches(("cell600_n4", {}))
    sc = tracern.CompositeScene.from_flat(n, f)
    r = sc.intersect_rays(b.i_origins[:300], b.i_directions[:300], normals=True, max_transparent=2)
    assert (r["kind"] == -1).all() and (r["index"] == -1).all() and (r["lane"] == -1).all() and (r["dist"] == FLT_MAX).all()
    assert not r["n_transparent"].any() and not r["normal"].any() and (r["transparent"][:, :, 1] == -1).all()
    o = sc.occludes_rays(b.i_origins[:300], b.i_directions[:300])
    assert not o["blocked"].any() and not o["n_transparent"].any()


def test_a_box_scene_is_refused():
    box = tracern.BoxScene(4)
    o = np.zeros((2, 4), np.float32)
    hits = np.zeros((2, 4), np.int32)
    rays = _lib.NtRayBatch()
    rays.count, rays.origins, rays.directions = 2, o.ctypes.data, o.ctypes.data
    res = _lib.NtRayResults()
    res.hits = hits.ctypes.data
    for fn in (_lib.lib().nt_intersect_rays, _lib.lib().nt_occludes_rays):
        assert fn(box._handle, C.byref(rays), C.byref(res), -1) == _lib.NT_E_INVALID
        assert "not a composite scene" in _lib.last_error()
