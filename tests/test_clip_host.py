"""Clip planes without a GPU: the ABI and the Python surface, every refusal before a device is touched, what the header says, and
the pins and floors of tests/clip_cases.py -- the references of tests/test_clip_gpu.py -- by the oracle alone.

Floors, as the code below asserts them.  Under the median plane and under the eight planes every view of every scene shows >= 5
pixels that moved to another surface and >= 5 that stayed.  Under the slab every view shows >= 5 that stayed and >= 5 that lost
their surface, and on cell120_n4 >= 5 that moved.  The one exception: under the slab the views of cell600_n4, orthoplex5_n5,
simplex7_n7 and simplex10_n10 are NOT asked for moved pixels.  Those shells are convex, and the slab lies between the 0.2 and
0.5 quantiles of the points SEEN: behind the nearer plane a ray meets only the shell's far side, well beyond the slab (0 .. 4
moved pixels measured).  Moved pixels under a finite t1 at N = 5, 7 and 10 come from clip_cases.two_shells instead -- the twin
of each scene, both halves, under a slab that takes the near shell away and keeps the front of the far one -- with >= 5 moved,
>= 5 unchanged and >= 5 lost pixels each."""
import ctypes as C
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import clip_cases as cc
import ntracer_amd
import primary_hit_cases as ph
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")
W, H = cc.W, cc.H


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", cc.PINNED)
def test_the_brute_force_without_planes_is_the_oracle_bit_for_bit(name):
    for k in cc.CAMERAS:
        e = ph.expected((name, {}), W, H, k)
        b = cc.brute(name, W, H, k, cc.NO_PLANES)
        bad = int((b["dist"].view(np.uint32) != e["dist"].view(np.uint32)).sum())
        print("%s camera %d: %d mismatches of %d" % (name, k, bad, W * H))
        assert bad == 0
        sure = b["unique"]
        assert np.array_equal(b["item"][sure], e["item"][sure]) and np.array_equal(b["lane"][sure], e["lane"][sure])
        assert not b["near"].any()                           # (no planes: t0 = 0 and no t1, and no candidate lies at 0)


@pytest.mark.parametrize("name", cc.SCENES_A)
def test_the_plane_sets_meet_their_floors_and_the_near_cap(name):
    for k in cc.CAMERAS:
        for kind in cc.KINDS:
            moved, unchanged, lost, near = cc.census(name, kind, k)
            print("%s camera %d %s: moved %d, unchanged %d, lost %d, near %d of %d" % (name, k, kind, moved, unchanged, lost, near, W * H))
            assert near <= cc.NEAR_CAP * W * H, (name, k, kind, near)
            normals, offsets = cc.planes(name, kind, k)
            assert len(offsets) == {"median": 1, "slab": 2, "eight": 8}[kind] <= cc.CLIP_MAX
            assert unchanged >= cc.MIN_UNCHANGED, (name, k, kind, unchanged)
            if kind != "slab" or name == "cell120_n4":
                assert moved >= cc.MIN_MOVED, (name, k, kind, moved)
            if kind == "slab":
                assert lost >= cc.MIN_LOST, (name, k, kind, lost)
                t0, t1, empty = cc.window((normals, offsets), ph.camera(name, k)[0], ph.rays(name, W, H, k)[0].reshape(W * H, -1))
                assert (t1 < cc.FLT_MAX).all() and not empty.all()       # the slab exercises t1 on every ray
    # at the other sizes of the GPU test (which takes cell120_n4 at 37 x 21 alone) the cap is a pixel at least
    for w, h in cc.SIZES[1:3] if name != "cell120_n4" else []:
        for kind in cc.KINDS:
            assert int(cc.brute(name, w, h, 0, cc.planes(name, kind, 0))["near"].sum()) <= max(1, int(cc.NEAR_CAP * w * h)), (name, kind, w, h)


def test_the_window_rule_on_rays_worked_by_hand():
    a = np.asarray([[2.0, 0.0, 0.0]], np.float32)
    o = np.asarray([1.0, 0.0, 0.0], np.float32)
    d = np.asarray([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    # 2 x <= 6: leaving at t = 2, entering never (t0 stays 0), parallel inside
    t0, t1, empty = cc.window((a, np.asarray([6.0], np.float32)), o, d)
    assert list(t0) == [0, 0, 0] and list(t1) == [2.0, cc.FLT_MAX, cc.FLT_MAX] and not empty.any()
    # 2 x <= -4 from outside: the ray towards it enters at t = 3, the others never do
    t0, t1, empty = cc.window((a, np.asarray([-4.0], np.float32)), o, d)
    assert list(empty) == [True, False, True] and t0[1] == 3.0 and t1[0] == -3.0
    # keep-regions that do not meet
    t0, t1, empty = cc.window(cc.keep_nothing("cell600_n4"), ph.camera("cell600_n4", 0)[0], ph.rays("cell600_n4", 8, 8, 0)[0].reshape(64, -1))
    assert empty.all()
    t0, t1, empty = cc.window(cc.keep_all("cell600_n4"), ph.camera("cell600_n4", 0)[0], ph.rays("cell600_n4", 8, 8, 0)[0].reshape(64, -1))
    assert not empty.any()


@pytest.mark.parametrize("high", cc.HIGH, ids=lambda v: "n%d" % v[0])
def test_the_wide_combs_are_cut_through_their_primitives(high):
    s, d, aabb, plane, plain, cut = cc.high(*high)
    was, now = plain["item"] >= 0, cut["item"] >= 0
    moved = was & now & (plain["dist"] != cut["dist"])
    print("n = %d: %d hit, %d moved, %d lost, %d near" % (high[0], int(was.sum()), int(moved.sum()), int((was & ~now).sum()), int(cut["near"].sum())))
    assert moved.sum() >= cc.MIN_MOVED and (was & ~now).sum() >= cc.MIN_LOST and (was & now & ~moved).sum() >= cc.MIN_UNCHANGED
    assert cut["near"].sum() <= cc.NEAR_CAP * aabb.size and high[0] > 10


@pytest.mark.parametrize("name", cc.TWO_SHELLS)
def test_the_slab_over_two_shells_moves_pixels_under_a_finite_t1(name):
    n, both, params, (o, axes), d, aabb, planes, plain, cut = cc.two_shells(name)
    was, now = plain["item"] >= 0, cut["item"] >= 0
    same = was & now & (plain["dist"].view(np.uint32) == cut["dist"].view(np.uint32))
    moved, lost = was & now & ~same, was & ~now
    print("%s: %d hit, %d moved, %d unchanged, %d lost, %d near" % (name, int(was.sum()), int(moved.sum()), int(same.sum()), int(lost.sum()),
                                                                    int(cut["near"].sum())))
    assert moved.sum() >= cc.MIN_MOVED and same.sum() >= cc.MIN_UNCHANGED and lost.sum() >= cc.MIN_LOST
    assert cut["near"].sum() <= cc.NEAR_CAP * aabb.size and n > 4
    t0, t1, empty = cc.window(planes, o, d.reshape(-1, n))
    assert (t1 < cc.FLT_MAX).all()                                  # a finite t1 on every ray
    # the pixels that moved show the far shell: a simplex of the copy
    nb, nt = len(both["batch_recs"]) // 2, len(both["tri_recs"]) // 2
    item = cut["item"][moved]
    assert (np.where((item & 3) == 0, (item >> 2) >= nb, (item >> 2) >= nt)).all()
    if name == "simplex10_n10":
        # loose triangles, the walk's scalar accept site: the scene has three a shell; >= 5 pixels show one of the near shell's,
        # which the slab rejects there, and some pixel shows one of the far shell's under it, which it accepts there
        loose_near = was & ((plain["item"] & 3) == 1) & ((plain["item"] >> 2) < nt)
        assert nt == 3 and loose_near.sum() >= cc.MIN_MOVED and not (now & ((cut["item"] & 3) == 1) & ((cut["item"] >> 2) < nt)).any()
        assert (now & ((cut["item"] & 3) == 1) & ((cut["item"] >> 2) >= nt)).sum() >= 1


@pytest.mark.parametrize("t", cc.TWINS, ids=cc.twin_id)
def test_the_twin_is_changed_by_its_second_half(t):
    name, variant = t
    n, both, emptied, params, plane, cams = cc.twin(name, variant)
    # B's leaves alone are emptied: same nodes, same splits, same box
    for key in both:
        same = np.array_equal(np.asarray(both[key]), np.asarray(emptied[key]))
        assert same == (key not in (("batch_recs", "node_right") if variant == "glass-split" else ("node_right",))), key
    if variant == "glass-split":
        # the plane passes between the simplices of every batch: lanes 0 and 1 on A's side, 2 and 3 beyond it, and the
        # expected scene has exactly those two removed
        p1 = np.asarray(both["batch_recs"])[:, :, 1 + n]
        assert (p1[:, :2] < plane[1][0]).all() and (p1[:, 2:] > plane[1][0]).all()
        assert not np.asarray(emptied["batch_recs"])[:, 2:].any() and np.array_equal(emptied["batch_recs"][:, :2], both["batch_recs"][:, :2])
    nn = (len(both["node_axis"]) - 1) // 2
    root = int(both["root"])
    assert both["node_axis"][root] == 0 and both["node_split"][root] == plane[1][0] and root == 2 * nn
    lo, hi = np.asarray(rq.scene(name)[2]["aabb_start"]), np.asarray(rq.scene(name)[2]["aabb_end"])
    assert hi[0] < plane[1][0] < hi[0] + 0.5 * (hi[0] - lo[0])
    if variant in ("lit", "reflective", "glass", "glass-split"):
        assert (np.asarray(params["point_light_pos"]).reshape(-1, n)[:, 0] < plane[1][0]).all()         # the lights are on A's side
    if variant in ("glass", "glass-split"):
        m = np.asarray(both["materials"])
        assert (m[:, 6] < 1).any() and (m[np.asarray(both["batch_mats"]).ravel()][:, 6] < 1).sum() * 2 < both["batch_mats"].size
    assert cams[0][0][0] < plane[1][0] < cams[1][0][0]         # camera 1 stands in the half-space that is cut away
    for k in cc.TWIN_CAMERAS:
        rec, col, seen = cc.twin_census(name, variant, k)
        a, b = cc.twin_expected(name, variant, k), cc.twin_unclipped(name, variant, k)
        second = int(((a["item"] == b["item"]) & (a["item"] >= 0) & (np.abs(a["frame"] - b["frame"]) > 1e-4).any(axis=2)).sum())
        print("%s camera %d: B changes %d records and %d colours (%d through secondary rays alone), A shows on %d pixels"
              % (cc.twin_id(t), k, rec, col, second, seen))
        assert rec >= cc.MIN_TWIN_DIFF and col >= cc.MIN_TWIN_DIFF and seen >= cc.MIN_TWIN_DIFF
        if variant in ("glass", "glass-split"):
            assert (a["n_transparent"] > 0).sum() >= cc.MIN_TWIN_DIFF
        if variant == "glass-split":
            # the simplices beyond the plane change the transparent lists of rays that meet them in A's own leaves
            assert (a["n_transparent"] != b["n_transparent"]).sum() >= cc.MIN_TWIN_DIFF
    if name == "cell600_n4" and variant in ("lit", "reflective", "glass"):
        a, b = cc.twin_expected(name, variant, 0), cc.twin_unclipped(name, variant, 0)
        assert ((a["item"] == b["item"]) & (a["item"] >= 0) & (np.abs(a["frame"] - b["frame"]) > 1e-4).any(axis=2)).sum() >= 1


def test_the_one_leaf_scene_reaches_the_last_test_rule_of_the_transparent_leaf():
    n, flat, removed, params, plane, (o, axes) = cc.one_leaf()
    whole, want = cc.one_leaf_views("whole"), cc.one_leaf_views("removed")
    # as it stands every pixel shows P's opaque simplex in front of the plane; without it Q, behind two transparent simplices
    # that the leaf's last test -- the miss of M -- trims away (tracer.hpp:977-1086): n_transparent is 0, where a leaf whose
    # last test were P's would keep the one at z = 1.5
    assert (whole["item"] == (2 << 2)).all() and (whole["lane"] == 1).all() and (whole["dist"] < 1.0).all()
    assert (want["item"] == 0).all() and (want["lane"] == 0).all() and (want["dist"] >= 3.0).all() and (want["n_transparent"] == 0).all()
    assert list(flat["items"]) == [0, 4, 8, 12] and flat["node_right"][0] == 4 and (np.asarray(flat["materials"])[:, 6] < 1).any()
    d = np.asarray([[0.0, 0.0, 1.0]], np.float32)
    t0, t1, empty = cc.window(plane, o, d)
    assert t0[0] == 1.0 and t1[0] == cc.FLT_MAX and not empty[0]                # z = 0.5 is cut away, z = 1.5, 2 and 3 are kept
    assert not np.asarray(removed["batch_recs"])[2, 1].any() and np.array_equal(removed["batch_recs"][2, 0], flat["batch_recs"][2, 0])


# ------------------------------------------------------------------ the ABI and the Python surface
NAMES = ("nt_scene_set_clip_planes", "nt_scene_get_clip_planes")


def test_the_exported_symbols_the_header_and_the_python_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "int nt_scene_set_clip_planes(nt_scene_t *s, int count, const float *normals, const float *offsets);" in code
    assert "int nt_scene_get_clip_planes(const nt_scene_t *s, int *count, float *normals, float *offsets);" in code
    assert re.search(r"#define NT_CLIP_MAX 8\b", code) and _lib.NT_CLIP_MAX == 8 == cc.CLIP_MAX
    assert re.search(r"#define NT_DEV_CLIP_MAX 8\b", sup.source("nt_device.hpp"))
    # the header carries the rule ...
    for phrase in ("t0 = 0, t1 = FLT_MAX, empty = false", "p = a_k0 * o_0, then p = p + a_kj * o_j", "s = p - b_k",
                   "r = a_k0 * d_0, then r = r + a_kj * d_j", "q = (-s) / r, and if q < t1 then t1 = q", "q = (-s) / r, and if q > t0 then t0 = q",
                   "r == 0 and s > 0:  empty = true", "empty = empty or t0 > t1", "!empty && t0 <= t <= t1", "a_k . x <= b_k",
                   "max(aabb entry, t0)", "no caps", "casts no shadow and shows in no mirror", "never been tested"):
        assert phrase in header, phrase
    # ... and the refusals
    for phrase in ("supersampling factor above 1", "row bands", "collect_stats", "a lens", "the parallel projection", "ambient occlusion",
                   "outlines", "depth cues", "a scene with Solids", "nt_colors_at / nt_calculate_color", "nt_ray_colors*", "nt_render_rays*",
                   "nt_adaptive_mask*", "nt_ambient_occlusion*", "nt_outline_mask*", "nt_depth_cue_factors*", "ignore the setting",
                   "Not part of a pickled scene"):
        assert phrase in header[header.index("Clip planes (the reference has none)"):header.index("#define NT_CLIP_MAX")], phrase
    for cls in (tracern.CompositeScene, tracern.BoxScene):
        params = [(p.name, p.default) for p in list(inspect.signature(cls.set_clip_planes).parameters.values())[1:]]
        assert params == [("planes", inspect.Parameter.empty)]
        assert isinstance(inspect.getattr_static(cls, "clip_planes"), property) and inspect.getattr_static(cls, "clip_planes").fset is None
    assert ntracer_amd.clip_plane_through is tracern.clip_plane_through and "clip_plane_through" in ntracer_amd.__all__


def test_clip_plane_through_rounds_the_float64_dot_product_once():
    point = (0.1, 0.2, 0.3, 1.0 / 3.0)
    normal = (1.0 / 7.0, -2.5, 1e-3, 3.0)
    a, b = ntracer_amd.clip_plane_through(point, normal)
    a32 = np.asarray(normal, np.float32)
    assert a == tuple(float(v) for v in a32)
    assert b == float(np.float32(np.dot(a32.astype(np.float64), np.asarray(point, np.float64))))
    a, b = ntracer_amd.clip_plane_through(tracern.Vector(3, (1, 2, 3)), tracern.Vector(3, (0, 0, 1)))
    assert (a, b) == ((0.0, 0.0, 1.0), 3.0)
    with pytest.raises(ValueError):
        ntracer_amd.clip_plane_through((1, 2, 3), (1, 2))


def _scene(name="cell600_n4"):
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat), n


def _raw(n, planes):
    normals = np.ascontiguousarray([p[0] for p in planes], np.float32).reshape(-1, n)
    offsets = np.ascontiguousarray([p[1] for p in planes], np.float32)
    return len(planes), normals.ctypes.data_as(_lib.f32p), offsets.ctypes.data_as(_lib.f32p), (normals, offsets)


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    sc, n = _scene()
    assert sc.clip_planes == ()
    two = [((0.5, -0.25, 0.75, 1.0), 1.5), ((0.0, 0.0, 0.0, -3.0), -0.125)]
    sc.set_clip_planes(two)
    assert sc.clip_planes == tuple(two)
    sc.set_clip_planes([(tracern.Vector(4, (1, 0, 0, 0)), 2)])
    assert sc.clip_planes == (((1.0, 0.0, 0.0, 0.0), 2.0),)
    eight = [(tuple(float(j == k % 4) * (k + 1) for j in range(4)), float(k)) for k in range(8)]
    sc.set_clip_planes(eight)
    assert sc.clip_planes == tuple(eight)
    # the ABI's getter through whichever pointers are given
    count, normals, offsets = C.c_int(-1), np.full((8, n), -1, np.float32), np.full(8, -1, np.float32)
    assert L.nt_scene_get_clip_planes(sc._handle, C.byref(count), None, None) == 0 and count.value == 8
    assert L.nt_scene_get_clip_planes(sc._handle, None, normals.ctypes.data_as(_lib.f32p), None) == 0 and normals[7].tolist() == [0, 0, 0, 8.0]
    assert L.nt_scene_get_clip_planes(sc._handle, None, None, offsets.ctypes.data_as(_lib.f32p)) == 0 and offsets.tolist() == [float(k) for k in range(8)]
    assert L.nt_scene_get_clip_planes(sc._handle, None, None, None) == 0
    assert L.nt_scene_get_clip_planes(None, C.byref(count), None, None) == _lib.NT_E_INVALID
    # every refusal leaves it as it was
    keep = sc.clip_planes
    nan, inf = float("nan"), float("inf")
    ok = ((1.0, 0.0, 0.0, 0.0), 1.0)
    refused = [[ok] * 9, [((0.0, 0.0, 0.0, 0.0), 1.0)], [ok, ((0.0, 0.0, 0.0, 0.0), 0.0)], [((1.0, 0.0, 0.0, 0.0), nan)], [((1.0, 0.0, 0.0, 0.0), inf)]]
    refused += [[ok, (tuple(v if j == k else 1.0 for j in range(n)), 0.0)] for k in (0, n - 1) for v in (nan, inf, -inf)]
    for planes in refused:
        cnt, pn, po, hold = _raw(n, planes)
        assert L.nt_scene_set_clip_planes(sc._handle, cnt, pn, po) == _lib.NT_E_INVALID, planes
        assert "clip plane" in _lib.last_error()
        assert sc.clip_planes == keep
        with pytest.raises(ValueError):
            sc.set_clip_planes(planes)
        assert sc.clip_planes == keep
    cnt, pn, po, hold = _raw(n, [ok])
    assert L.nt_scene_set_clip_planes(sc._handle, -1, pn, po) == _lib.NT_E_INVALID and sc.clip_planes == keep
    assert L.nt_scene_set_clip_planes(None, 1, pn, po) == _lib.NT_E_INVALID
    for bad in ([((1, 0, 0), 0.0)], [((1, 0, 0, 0, 0), 0.0)], [(1, 0, 0, 0)], [((1, 0, 0, 0), "1")], [((1, 0, 0, 0), True)], [((1, 0, 0, 0),)], 5):
        with pytest.raises((ValueError, TypeError)):
            sc.set_clip_planes(bad)
        assert sc.clip_planes == keep
    # locked while a render holds the scene, as nt_scene_set_camera
    assert L.nt_scene_lock(sc._handle) == 0
    assert L.nt_scene_set_clip_planes(sc._handle, cnt, pn, po) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_clip_planes(sc._handle, 0, None, None) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        sc.set_clip_planes(None)
    assert sc.clip_planes == keep
    assert L.nt_scene_unlock(sc._handle) == 0
    # off: a count of 0, NULL pointers, None, an empty sequence
    assert L.nt_scene_set_clip_planes(sc._handle, 0, pn, po) == 0 and sc.clip_planes == ()
    sc.set_clip_planes([ok])
    assert L.nt_scene_set_clip_planes(sc._handle, 1, None, po) == 0 and sc.clip_planes == ()
    sc.set_clip_planes([ok])
    assert L.nt_scene_set_clip_planes(sc._handle, 1, pn, None) == 0 and sc.clip_planes == ()
    sc.set_clip_planes([ok])
    sc.set_clip_planes(None)
    assert sc.clip_planes == ()
    sc.set_clip_planes([ok])
    sc.set_clip_planes([])
    assert sc.clip_planes == ()
    assert L.nt_scene_get_clip_planes(sc._handle, C.byref(count), normals.ctypes.data_as(_lib.f32p), offsets.ctypes.data_as(_lib.f32p)) == 0 and count.value == 0
    # a view setting like fov, kept in the native handle: no part of what is pickled, and not carried over to another scene
    before = pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2)
    sc.set_clip_planes([ok])
    assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before
    assert not any("clip" in k for k in sc.__dict__)
    assert sc.with_rebuilt_tree().clip_planes == () and sc.clip_planes == (ok,)
    assert _scene()[0].clip_planes == ()
    # a BoxScene has none
    box = tracern.BoxScene(4)
    assert L.nt_scene_set_clip_planes(box._handle, cnt, pn, po) == _lib.NT_E_INVALID
    assert L.nt_scene_set_clip_planes(box._handle, 0, None, None) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_clip_planes([ok])
    assert box.clip_planes == ()


def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device: NT_E_UNSUPPORTED with a message that starts "clip planes", the
    destination as it was (the table form needs a device to make its table).  There is no device here: a refusal that reached
    one would show as another error."""
    L = _lib.lib()
    sc, n = _scene()
    ok = ((1.0, 0.0, 0.0, 0.0), 1.0)
    sc.set_clip_planes([ok])
    w, h = 8, 4
    fmt = sup.fmt_of(w, h)
    fst = fmt._as_struct()
    size = fmt.pitch * h
    dest = (C.c_char * size)(*([0x4E] * size))
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def forms(scene, opts):
        po = None if opts is None else C.byref(opts)
        return [L.nt_render(scene._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_device(scene._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_frames_device(scene._handle, dest, size, 1, origins.ctypes.data_as(_lib.f32p), axes.ctypes.data_as(_lib.f32p),
                                          C.byref(fst), po, None)]

    def refused(opts, word, scene=sc):
        for status in forms(scene, opts):
            assert status == _lib.NT_E_UNSUPPORTED, (word, status, _lib.last_error())
            assert _lib.last_error().startswith("clip planes") and word in _lib.last_error(), _lib.last_error()
        assert bytes(dest) == b"\x4e" * size

    sc.set_supersampling(2)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(None)
    sc.set_supersampling(1)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "band")
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    sc.set_lens(None)
    sc.set_parallel_projection(2.0)
    refused(None, "parallel")
    sc.set_parallel_projection(None)
    sc.set_ambient_occlusion(4, 1.0)
    refused(None, "ambient occlusion")
    sc.set_ambient_occlusion(None)
    sc.set_outlines()
    refused(None, "outlines")
    sc.set_outlines(None)
    sc.set_depth_cue(1.0, 2.0)
    refused(None, "depth cues")
    with pytest.raises(NotImplementedError, match="clip planes"):
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, sc)
    sc.set_depth_cue(None)
    # a scene with Solids: renders and primary hits alike
    g, n5, flat = rq.scene("feature5_n5")
    solids = tracern.CompositeScene.from_flat(n5, flat)
    solids.set_clip_planes([((1.0, 0.0, 0.0, 0.0, 0.0), 1.0)])
    origins, axes = np.zeros((1, n5), np.float32), np.eye(n5, dtype=np.float32)[None].copy()
    refused(None, "Solids", solids)
    hits = np.zeros((w * h, 4), np.int32)
    hb = _lib.NtHitBuffers()
    hb.hits = hits.ctypes.data
    assert L.nt_primary_hits(solids._handle, w, h, C.byref(hb), -1) == _lib.NT_E_UNSUPPORTED and "Solids" in _lib.last_error()
    assert L.nt_primary_hits_device(solids._handle, w, h, C.byref(hb), None, None) == _lib.NT_E_UNSUPPORTED
    assert not hits.any()
    # with the setting off again the other settings' own refusals are back, in their own words
    sc.set_clip_planes(None)
    sc.set_depth_cue(1.0, 2.0)
    sc.set_outlines()
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()
    for status in forms(sc, None):
        assert status == _lib.NT_E_UNSUPPORTED and _lib.last_error().startswith("depth cue")
    # each of them in the setting's own words, which tests/view_setting_refusals.py has byte for byte and
    # tests/test_view_setting_refusals.py holds every render form to; the tenth, the row range, is a guard for callers inside
    # nt_api.cpp, which the same test reads
    import view_setting_refusals as vr
    words = [m for (setting, _), m in vr.RENDER_REFUSALS.items() if setting == "clip"]
    assert len(words) == 9 and all(m.startswith("clip planes are not available") for m in words)
    # render_checks asks the planes first -- of the planes and the cue the planes refuse --, and enqueue sends the scene to
    # enqueue_clip before any other setting's route
    assert vr.RENDER_REFUSALS["clip", "cue"] == "clip planes are not available while depth cues are on"
    assert ("cue", "clip") not in vr.RENDER_REFUSALS and "kViewSettings" in sup.function_body(sup.source("nt_api.cpp"), "int render_checks(")
    enq = sup.function_body(sup.source("nt_api.cpp"), "int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in) {")
    assert enq.index("enqueue_clip(") < enq.index("enqueue_cue(")


def test_what_does_not_honour_the_setting_is_refused_while_it_is_on():
    L = _lib.lib()
    sc, n = _scene()
    sc.set_clip_planes([((1.0, 0.0, 0.0, 0.0), 1.0)])
    w, h = 8, 4
    out = np.full(w * h * 3, 77, np.float32)
    xs, ys = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rays = _lib.NtRays()
    o, d = np.zeros((2, n), np.float32), np.ones((2, n), np.float32)
    rays.count, rays.origins, rays.directions = 2, o.ctypes.data, d.ctypes.data
    fmt = sup.fmt_of(2, 1)
    fst = fmt._as_struct()
    sc.set_supersampling(2)
    sc.set_adaptive_supersampling(0.1)
    sc.set_ambient_occlusion(4, 1.0)
    sc.set_outlines()
    sc.set_depth_cue(1.0, 2.0)
    calls = [
        lambda: L.nt_colors_at(sc._handle, w, h, 1, xs.ctypes.data_as(_lib.i32p), ys.ctypes.data_as(_lib.i32p), out.ctypes.data_as(_lib.f32p), -1),
        lambda: L.nt_calculate_color(sc._handle, 0, 0, w, h, out.ctypes.data_as(_lib.f32p)),
        lambda: L.nt_ray_colors(sc._handle, C.byref(rays), out.ctypes.data_as(_lib.f32p), -1),
        lambda: L.nt_ray_colors_device(sc._handle, C.byref(rays), out.ctypes.data_as(_lib.f32p), None, None),
        lambda: L.nt_render_rays(sc._handle, out.ctypes.data, 64, C.byref(fst), C.byref(rays), -1),
        lambda: L.nt_render_rays_device(sc._handle, out.ctypes.data, 64, C.byref(fst), C.byref(rays), None, None),
        lambda: L.nt_adaptive_mask(sc._handle, w, h, out.ctypes.data, None, None),
        lambda: L.nt_adaptive_mask_device(sc._handle, w, h, out.ctypes.data, None, None),
        lambda: L.nt_ambient_occlusion(sc._handle, w, h, out.ctypes.data, None),
        lambda: L.nt_ambient_occlusion_device(sc._handle, w, h, out.ctypes.data, None, None),
        lambda: L.nt_outline_mask(sc._handle, w, h, out.ctypes.data, None, None),
        lambda: L.nt_outline_mask_device(sc._handle, w, h, out.ctypes.data, None, None),
        lambda: L.nt_depth_cue_factors(sc._handle, w, h, out.ctypes.data, None),
        lambda: L.nt_depth_cue_factors_device(sc._handle, w, h, out.ctypes.data, None, None),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.NT_E_UNSUPPORTED, (k, _lib.last_error())
        assert _lib.last_error().startswith("clip planes"), (k, _lib.last_error())
    assert (out == 77).all()
    with pytest.raises(NotImplementedError, match="clip planes"):
        sc.calculate_color(0, 0, w, h)
    # a BoxScene is not concerned, and the ray queries ignore the setting: they get as far as the device
    q = _lib.NtRayBatch()
    q.count, q.origins, q.directions = 2, o.ctypes.data, d.ctypes.data
    res = _lib.NtRayResults()
    hits = np.zeros((2, 4), np.int32)
    res.hits = hits.ctypes.data
    status = L.nt_intersect_rays(sc._handle, C.byref(q), C.byref(res), -1)
    assert status != _lib.NT_E_UNSUPPORTED and "clip" not in _lib.last_error()


# ------------------------------------------------------------------ the kernels' source
def test_the_clip_launches_are_kept_apart_from_the_existing_launchers():
    comp, var = sup.source("nt_composite.hpp"), sup.source("nt_var.hip")
    for src, head in ((comp, "int launch_composite_fixed("), (var, "int nt_launch_composite("), (var, "int nt_launch_hits("),
                      (sup.source("nt_hits.hpp"), "int launch_hits_fixed("), (sup.source("nt_cue.hpp"), "int launch_cue_fixed(")):
        body = sup.function_body(src, head)
        assert "clip" not in body.lower().replace("nt_clipplanes{nullptr,0}", "").replace("ntclipplanes{nullptr, 0}", ""), head
    fixed = sorted(sup.launches_through(sup.source("nt_clip.hpp"), "int launch_clip_fixed("))
    assert fixed == sorted(["packet_numerators<N>", "composite_packet<N,32,false,true,true,false,true>", "composite_packet<N,32,false,false,true,false,true>",
                            "clip_shade<N,false,false>", "clip_shade<N,true,true>", "clip_shade<N,true,false>", "hits_normals<N,true>",
                            "hits_normals<N,false>"])
    general = sorted(sup.launches(sup.function_body(var, "int clip_var_launch(")))
    assert general == sorted(["composite_kernel_var", "composite_kernel_var_t<true>", "composite_kernel_var_t<false>", "hits_closest_var",
                              "hits_closest_var_t<true>", "hits_closest_var_t<false>"])
    assert not sup.launches(sup.function_body(var, "int nt_launch_clip("))
    # composite_packet's CLIP is a trailing parameter with a default, and the walks' a trailing type with one
    assert "template <int N, int DEPTH, bool FEAT, bool SCAL, bool HITS = false, bool LENS = false, bool CLIP = false>" in comp
    assert comp.count("typename CLIP = ClipOff>") == 3 and comp.count("typename WIN = ClipOff::Win>") == 2
    # the new translation unit is in the build's list, once a dimension
    from ntracer_amd import build
    units = [u for u in build.units() if u[1] == "nt_inst_clip.hip"]
    assert sorted(int(u[2][0].split("=")[1]) for u in units) == list(range(3, 11))
    assert os.path.join(CSRC, "nt_clip.hpp") in [os.path.normpath(p) for p in build.HDR]
    assert '#ifndef NT_INST_N\n#error' in sup.source("nt_inst_clip.hip")
    out = os.popen("nm -D -C --defined-only %s" % _lib.LIB_PATH).read()
    assert sorted(int(v) for v in re.findall(r"\bnt_clip_packet<(\d+)>\(", out)) == list(range(3, 11))
