"""The Solid family without a GPU: the oracle pinned to a float64 brute force on the torture scenes of tests/solid_cases.py,
builder.solid_bounds and the native builder's placement of Solids against float64 surface points, the structure the scenes
promise, and the route table of tests/test_solids_gpu.py held against the sources."""
import collections
import os
import re

import numpy as np
import pytest

import solid_cases as sc
import support as sup
from ntracer_amd import _lib, builder, tracern

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntracer_amd", "csrc")


def _id(case):
    return "%s-n%d" % case


# ------------------------------------------------------------------ 1. the oracle against float64
@pytest.mark.parametrize("case", sc.scene_dims(), ids=_id)
def test_the_oracle_agrees_with_float64_on_every_batch(case):
    """which primitive is hit, on every ray outside the margin; dist within TOLERANCE[n]; the hit point and the normal O n_local
    (not normalised) to a part in 10^4 -- the bound of an fp32 matrix product of 64 terms, not a measured one; the cap on what
    the margin leaves out, by float64 alone; and the floors that keep a batch from passing on misses"""
    name, n = case
    for variant in sc.variants(name, n):
        b = sc.batches(name, n, variant)
        bf = b.brute
        label = "%s n=%d %s" % (name, n, variant)
        for key, sl in b.slices.items():
            count, out = sl.stop - sl.start, int((~bf.safe[sl]).sum())
            if sc.capped(b, key):
                assert out <= sc.CAP * count, "%s %s: %d of %d rays inside the margin" % (label, key, out, count)
            else:
                assert out >= 1, (label, key)               # (the exempt batches are where they were aimed)
        for clean in (False, True):
            ref = b.i_ref[clean]
            worst = sc.compare_with_float64(b, ref, label)
            both = bf.safe & (bf.item >= 0)
            for got, want in ((ref["normal_origin"], bf.normal_origin), (ref["normal"], bf.normal)):
                if clean:           # (in the default mode a later cube test leaves its marks in the normal ray: the reference's aliasing)
                    # (... plus what the ray's own deviation in dist moves the hit point by, and a sphere's normal with it)
                    scale = np.maximum(np.abs(want[both]).max(axis=1, keepdims=True), 1.0)
                    moved = 2 * np.abs(ref["dist"][both].astype(np.float64) - bf.dist[both])[:, None]
                    assert (np.abs(got[both] - want[both]) <= 1e-4 * scale + moved).all(), label
        # both normal modes find the same hits
        for k in ("dist", "item", "lane", "n_transparent"):
            assert np.array_equal(b.i_ref[False][k], b.i_ref[True][k]), (label, k)
        # ---- floors
        r = b.i_ref[False]
        hits = {key: int((r["item"][sl] >= 0).sum()) for key, sl in b.slices.items()}
        assert hits["A0"] >= 90, (label, hits)
        for key in ("C", "D"):
            if key in b.slices:
                sl = b.slices[key]
                assert hits[key] > 0 and (name != "field" or hits[key] < sl.stop - sl.start), (label, key, hits)
        if "B" in b.slices:
            sl = b.slices["B"]
            d = b.i_directions[sl]
            assert ((d != 0).sum(axis=1) == 1).all()                                  # exact zeros in every other component
            assert 0.2 * (sl.stop - sl.start) < hits["B"] < sl.stop - sl.start, (label, hits)
        en = slice(b.slices["ENO"].start, b.slices["ENI"].stop)
        assert en.stop - en.start == b.slices["ES"].stop - b.slices["ES"].start
        assert hits["ENO"] + hits["ENI"] >= hits["ES"] and b.o_ref["blocked"][en].sum() >= b.o_ref["blocked"][b.slices["ES"]].sum(), (label, hits)
        # both kinds of leg without the skip are there, and the float64 check of those that leave cannot go empty: the cap above
        assert b.slices["ENO"].stop - b.slices["ENO"].start >= 15 and b.slices["ENI"].stop - b.slices["ENI"].start >= 15, label
    print("%s n=%d: oracle within %g relative of float64, nearer than %g within %g ulps" % (name, n, worst[0], sc.NEAR, worst[1]))


def test_axis_rays_on_a_face_plane_and_along_a_face():
    """batch B by hand, field at n = 3: an origin exactly on the entry face's plane gives dist == 0, which is no hit of that cube
    -- the ray goes through it unseen -- and a line with p_j == 1 exactly still counts as within the face (<= 1 + fuzz)"""
    b = sc.batches("field", 3)
    flat = sc.scene("field", 3)
    sl = b.slices["B"]
    o, d, r = b.i_origins[sl], b.i_directions[sl], b.i_ref[False]
    n_plane = n_edge = 0                                    # rays on a plane; lines along a face that meet their own cube
    for k in range(len(flat["solid_types"])):
        rec = np.asarray(flat["solid_recs"], np.float64)[k]
        if int(flat["solid_types"][k]) != sc.CUBE or rec[0] != 0.25 or not np.array_equal(rec[:9].reshape(3, 3), 0.25 * np.eye(3)):
            continue
        if int(flat["solid_mats"][k]) == 2:
            continue                                        # (a transparent cube is no ray's closest opaque hit)
        item = (k << 2) | _lib.KIND_SOLID
        u = (o.astype(np.float64) - sc.solid_centre(flat, k)) * 4                    # local coordinates, exact
        a = np.argmax(d != 0, axis=1)
        ua = u[np.arange(len(u)), a] * d[np.arange(len(u)), a]                       # along the ray, in front: negative
        rest = np.abs(np.where(np.arange(3)[None] == a[:, None], 0.0, u))
        on_plane = (ua == -1.0) & (rest < 1).all(axis=1) & (np.abs(u) <= 2).all(axis=1)
        along = (ua == -2.0) & (rest.max(axis=1) == 1.0)
        assert (r["item"][sl][on_plane] != item).all(), k
        # (... unless a neighbour that overlaps the cube is met first)
        own = r["item"][sl][along] == item
        # (... or the line lies in a split plane of the tree and the walk takes the side that does not hold the cube)
        assert (r["dist"][sl][along][own] == f32(0.25)).all(), k
        n_plane, n_edge = n_plane + int(on_plane.sum()), n_edge + int(own.sum())
    assert n_plane >= 4 and n_edge >= 2, (n_plane, n_edge)


# ------------------------------------------------------------------ 2. solid_bounds
@pytest.mark.parametrize("n", (3, 7, 17))
def test_solid_bounds_cover_and_are_tight(n):
    """2000 float64 surface points of each kind and type lie inside the box; the box is the closed form -- centre O p, extent
    sum_j |O_kj| of a cube and |O_k.| of a sphere -- to one fp32 ulp outward"""
    rng = np.random.default_rng(sc.SEED + n)
    for kind in range(4):
        for typ in (sc.CUBE, sc.SPHERE):
            centre = sc._centre(n, rng.uniform(-1, 1, 3), 0.01)
            flat = dict(solid_recs=sc.solid_record(n, typ, centre, sc.orientation(n, kind, 0.3, rng))[None], solid_types=np.array([typ]),
                        aabb_start=np.zeros(n))
            rec = np.asarray(flat["solid_recs"], np.float64)[0]
            o, p = rec[:n * n].reshape(n, n), rec[2 * n * n:]
            lo, hi = builder.solid_bounds(typ == sc.CUBE, p, o)
            assert lo.dtype == f32 and hi.dtype == f32
            pts = sc.surface_points(flat, 0, 2000, rng)
            label = (n, sc.KIND_NAMES[kind], typ)
            ext = np.abs(o).sum(axis=1) if typ == sc.CUBE else np.sqrt((o * o).sum(axis=1))
            c = o @ p
            # every point is inside the fp32 box, and the box is the closed form or at most one fp32 ulp beyond it, outward
            ulp = np.spacing(np.maximum(np.abs(c - ext), np.abs(c + ext)).astype(f32)).astype(np.float64)
            assert (pts >= lo).all() and (pts <= hi).all(), label
            assert (lo <= c - ext).all() and (lo >= c - ext - ulp).all() and (hi >= c + ext).all() and (hi <= c + ext + ulp).all(), label
            # the points reach the closed form: the test would see a box that is too tight
            assert (pts.max(axis=0) >= c + ext - 1e-9).all() and (pts.min(axis=0) <= c - ext + 1e-9).all(), label


# ------------------------------------------------------------------ 3. and 4. the tree
@pytest.mark.parametrize("n", sc.dims("field"))
def test_field_tree_lists_every_solid_in_every_leaf_it_reaches(n):
    """the structure field promises -- 40 Solids and no simplex, at least 8 leaves, a Solid in 3 or more of them, more than 32
    Solids so that the `checked` lists pass a word -- and membership: where one of 2000 float64 surface points of a Solid lies
    more than 1e-5 inside a leaf's cell, the leaf lists the Solid"""
    flat = sc.scene("field", n)
    assert len(flat["solid_types"]) == 40 and len(flat["batch_recs"]) == 0 and len(flat["tri_recs"]) == 0
    assert (np.asarray(flat["solid_types"]) == sc.CUBE).sum() == 20
    leaves = sc.leaves(flat)
    refs = collections.Counter(i for _, _, items in leaves for i in items)
    assert len(leaves) >= 8 and max(refs.values()) >= 3 and len(refs) == 40, (len(leaves), max(refs.values()), len(refs))
    assert max(len(items) for _, _, items in leaves) >= 2
    rng = np.random.default_rng(sc.SEED + 50 + n)
    reached = 0
    for k in range(40):
        pts = sc.surface_points(flat, k, 2000, rng)
        item = (k << 2) | _lib.KIND_SOLID
        for lo, hi, items in leaves:
            inside = ((pts > lo + 1e-5) & (pts < hi - 1e-5)).all(axis=1)
            if inside.any():
                reached += 1
                assert item in items, "n=%d: Solid %d reaches the cell %r .. %r of a leaf that does not list it" % (n, k, lo[:3], hi[:3])
    assert reached >= sum(refs.values()) * 0.6, (reached, sum(refs.values()))      # (the points find most of the references)


@pytest.mark.parametrize("case", sc.scene_dims(), ids=_id)
def test_scene_structure(case):
    name, n = case
    flat = sc.scene(name, n)
    import high_dimension_cases as hd
    assert hd.stack_depth_of(flat) <= 32, case                 # (route() takes the packet walk's limit as met)
    kinds = set(int(i) & 3 for i in flat["items"])
    if name == "pierced":
        assert kinds == {_lib.KIND_BATCH, _lib.KIND_SOLID}
        # a leaf that holds batches and a Solid: the nearest hit alternates between a lane and a Solid there
        assert any(len(set(i & 3 for i in items)) == 2 for _, _, items in sc.leaves(flat)), case
    else:
        assert kinds == {_lib.KIND_SOLID} and len(flat["batch_recs"]) == 0 and len(flat["tri_recs"]) == 0
    # the three cameras: outside everything; inside the sphere; inside the cube -- by float64's local coordinates
    n_, orient, inv, pos = sc._solid_parts(flat)
    cams = sc.cameras(name, n)
    local = lambda cam, k: inv[k] @ cams[cam][0].astype(np.float64) - pos[k]
    for k in range(len(orient)):
        u = local(0, k)
        assert (np.abs(u).max() if int(flat["solid_types"][k]) == sc.CUBE else np.linalg.norm(u)) > 1.5, (case, k)
    # the stored inverse, which the float64 reference takes the local ray from, is the inverse of the stored orientation
    for k in range(len(orient)):
        assert np.abs(inv[k] @ orient[k] - np.eye(n)).max() < 1e-5 and np.abs(orient[k] @ inv[k] - np.eye(n)).max() < 1e-5, (case, k)
    assert int(flat["solid_types"][sc.INSIDE_SPHERE[name]]) == sc.SPHERE and np.linalg.norm(local(1, sc.INSIDE_SPHERE[name])) < 0.5
    assert int(flat["solid_types"][sc.INSIDE_CUBE[name]]) == sc.CUBE and np.abs(local(2, sc.INSIDE_CUBE[name])).max() < 0.5
    # from inside, the enclosing Solid is not there for the oracle: no ray of A1 names the sphere, none of A2 the cube
    b = sc.batches(name, n)
    for key, k in (("A1", sc.INSIDE_SPHERE[name]), ("A2", sc.INSIDE_CUBE[name])):
        assert (b.i_ref[False]["item"][b.slices[key]] != ((k << 2) | _lib.KIND_SOLID)).all(), (case, key)
    if name == "field":
        assert (b.i_ref[False]["item"][b.slices["A1"]] >= 0).sum() >= 100, case       # ... and what stands behind it is seen
    if name == "nest":
        rec = np.asarray(flat["solid_recs"])
        assert np.array_equal(rec[sc.COINCIDENT[0]], rec[sc.COINCIDENT[1]]) and flat["solid_mats"][sc.COINCIDENT[0]] != flat["solid_mats"][sc.COINCIDENT[1]]


def test_orientations_are_what_their_names_say():
    for n in (3, 10, 64):
        rng = np.random.default_rng(n)
        eye = np.eye(n)
        o = [sc.orientation(n, k, 0.3, rng) for k in range(4)]
        assert np.array_equal(o[0], 0.3 * eye)
        assert np.allclose(o[1] @ o[1].T, 0.09 * eye, atol=1e-12) and not np.allclose(o[1], 0.3 * eye)
        d = np.diag(o[2])
        assert np.array_equal(o[2], np.diag(d)) and d.max() / d.min() == 4.0
        inv = np.linalg.inv(o[3])
        assert not np.allclose(inv * (np.linalg.norm(o[3]) / np.linalg.norm(inv)), o[3].T, atol=1e-3)   # no multiple of the transpose
        assert np.linalg.cond(o[3]) < 20


# ------------------------------------------------------------------ 5. the route table
CALL = re.compile(r"\b(solid_intersects_marks|solid_intersects|solid_marks_var|solid_var)\s*(<[^<>]*>)?\s*\(")
HEAD = re.compile(r"^(?:__device__|__global__).*?\b(?:void|float|bool|int|Color3)\s+([A-Za-z_]\w*)\s*\(", re.M)


def _sites():
    """{enclosing function: file} of every call of the four functions in csrc (their own definitions left out)"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        src = sup.source(name)
        heads = [(m.start(), m.group(1)) for m in HEAD.finditer(src)]
        for m in CALL.finditer(src):
            line_start = src.rfind("\n", 0, m.start()) + 1
            if src[line_start:m.start()].lstrip().startswith(("__device__", "//")):
                continue                                    # the definition itself, or a comment
            inside = [h for h in heads if h[0] < m.start()]
            assert inside, (name, m.group(0))
            out[inside[-1][1]] = name
    return out


def test_every_call_site_of_the_solid_functions_is_in_a_family_the_route_table_reaches():
    sites = _sites()
    assert len(sites) >= 13, sites
    assert set(sites) == set(sc.SITES), "call sites no family accounts for: %s; families without a call site: %s" % (
        sorted(set(sites) - set(sc.SITES)), sorted(set(sc.SITES) - set(sites)))
    rows = [k for k, _ in sc.ROUTES]
    assert len(rows) == len(set(rows))
    families = {sc.family(k) for k in rows} - {None}
    assert families == set(sc.SITES.values()), (sorted(families), sorted(set(sc.SITES.values())))


def test_every_row_is_a_kernel_the_sources_launch_and_every_solid_capable_launch_has_a_row():
    launched = set()
    for name in sorted(os.listdir(CSRC)):
        for k in re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*(?:\s*<[^<>]*>)?)", sup.source(name)):
            launched.add(re.sub(r"\s+", "", k))
    rows = {k for k, _ in sc.ROUTES}
    assert rows <= launched, sorted(rows - launched)
    # a kernel of the stems the table knows, in an instantiation a scene with Solids takes, is a row: all of the _t and run-time-n
    # forms, and of the fixed ones those whose last flag (SCAL / SCALP: unbatched primitives in the leaf loops) is true
    stems = {k.split("<")[0] for k in rows}
    for k in sorted(launched):
        stem = k.split("<")[0]
        if stem not in stems or k in rows:
            continue
        args = k[k.index("<") + 1:-1].split(",") if "<" in k else []
        if stem == "composite_packet":
            capable = len(args) >= 4 and args[3] == "true" and len(args) <= 6       # (seven arguments: the clip-plane form)
        elif stem == "composite_kernel":
            # <N, FEAT, STATS, SCAL = true>: a scene with Solids is FEAT; the statistics launch is test_composite_matrix's row
            capable = args[1] == "true" and not (len(args) == 4 and args[3] == "false") and k not in sc.OTHER_ROWS
        else:
            capable = args[-1] == "true" and len(args) > 1
        assert not capable, "%s is launched, can walk a scene with Solids and has no row" % k
    for stem in sc.OTHER_SUITES:
        assert any(k.split("<")[0] == stem for k in launched), stem


def test_every_row_is_reached_by_a_case_of_the_gpu_test_and_nothing_else_is():
    reached = sc.reached()
    rows = dict(sc.ROUTES)
    assert set(reached) == set(rows), (sorted(set(reached) - set(rows)), sorted(set(rows) - set(reached)))
    for kernel, (name, n, kind, env, call) in sc.ROUTES:
        assert kernel in sc.route(name, n, kind, env, call), kernel
        assert (name, n, kind, tuple(sorted(env.items())), call) in reached[kernel], kernel
        assert call in sc.CALLS and all(k in sc.SWITCHES for k in env)


def test_clip_planes_are_refused_for_every_scene_before_a_device_is_touched():
    """a scene with Solids under clip planes: NT_E_UNSUPPORTED from the render and from primary_hits alike"""
    import ctypes as C
    import ntracer_amd
    import test_composite_matrix as tcm
    for name in sc.SCENES:
        for n in (3, 17):
            s = tracern.CompositeScene.from_flat(n, sc.scene_flat(name, n, "transparent"))
            s.set_clip_planes([([1.0] + [0.0] * (n - 1), 0.25)])
            fmt = tcm._fmt(9, 7)
            buf = bytearray([tcm.SENTINEL]) * (fmt.pitch * 7)
            with pytest.raises(NotImplementedError, match="Solids"):
                ntracer_amd.BlockingRenderer().render(buf, fmt, s)
            assert buf == bytearray([tcm.SENTINEL]) * (fmt.pitch * 7) and not s.locked
            hits = np.zeros((63, 4), np.int32)
            hb = _lib.NtHitBuffers()
            hb.hits = hits.ctypes.data
            assert _lib.lib().nt_primary_hits(s._handle, 9, 7, C.byref(hb), -1) == _lib.NT_E_UNSUPPORTED and "Solids" in _lib.last_error()
            assert not hits.any()
