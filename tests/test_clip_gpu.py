"""Clip planes (scene.set_clip_planes, nt_scene_set_clip_planes, and the renders and primary-hit passes that honour them) on the
GPU against tests/clip_cases.py, whose references come from the oracle alone.

Reference A, planes that cut through primitives: on every pixel that is not `near` a bound (clip_cases.brute; capped at 2 % of a
view by test_clip_host.py) dist must equal the brute force bit for bit and item / lane must be equal where one simplex alone
reaches that dist; an unlit pixel's colour must be the oracle's colour of its ray in a scene of its own simplex alone, within
the project's 1e-5 (1 byte in RGBX8).  Reference B, the twin scene: dist, item, lane and n_transparent must equal the oracle's
on the tree with B's leaves emptied, and frames must lie within 1e-5 of its frames -- unlit, lit with shadows, reflective, and
the glass variant on the general route.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import clip_cases as cc
import fixtures as fx
import primary_hit_cases as ph
import ray_color_cases as rc
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

W, H = cc.W, cc.H
TOL = 1e-5
SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL", "NTRACER_CHUNK_FRAMES")


def _env(mp, env):
    sup.set_switches(mp, SWITCHES, env)


def _golden(name, mp, k=0, variant="", env=None):
    _env(mp, env or {})
    n, flat, params = rc.case_scene((name, {}, variant))
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(params)
    sc.set_fov(ph.fov_of(name))
    sc._set_camera_arrays(*ph.camera(name, k))
    return sc


def _pairs(planes):
    normals, offsets = planes
    return [(tuple(float(v) for v in a), float(b)) for a, b in zip(normals, offsets)]


def frame_f32(sc, w, h):
    return sup.render_host(sc, sup.fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h, w, 3)


def _records(sc, w, h, normals=False):
    r = sc.primary_hits(w, h, normals=normals)
    return r


def _assert_brute(got, want, label, w, h):
    """dist bit for bit off the `near` pixels, item / lane where the minimiser is unique"""
    keep = ~want["near"]
    assert int(want["near"].sum()) <= max(1, int(cc.NEAR_CAP * w * h)), (label, int(want["near"].sum()))
    gd, wd = np.asarray(got.dist, np.float32).reshape(h, w), want["dist"]
    bad = np.argwhere((gd.view(np.uint32) != wd.view(np.uint32)) & keep)
    assert len(bad) == 0, "%s: dist differs on %d pixels, first (y, x) = %r: got %r, reference %r" % (
        label, len(bad), tuple(bad[0]), gd[tuple(bad[0])], wd[tuple(bad[0])])
    sure = keep & (want["unique"] | (want["item"] < 0))
    gi, gl = np.asarray(got.item).reshape(h, w), np.asarray(got.lane).reshape(h, w)
    assert np.array_equal(gi[sure], want["item"][sure]) and np.array_equal(gl[sure], want["lane"][sure]), label
    assert (np.asarray(got.n_transparent) == 0).all(), label
    return sure


# ------------------------------------------------------------------ Reference A
@pytest.mark.parametrize("name", cc.SCENES_A)
def test_cuts_through_primitives_equal_the_brute_force(name):
    cameras = cc.CAMERAS if name != "cell120_n4" else (0,)        # (14 400 simplices: one camera keeps the reference quick)
    sizes = cc.SIZES if name != "cell120_n4" else [(W, H)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _golden(name, mp)
        n = sc.dimension
        for k in cameras:
            sc._set_camera_arrays(*ph.camera(name, k))
            o = ph.camera(name, k)[0]
            for kind in cc.KINDS:
                planes = cc.planes(name, kind, k)
                sc.set_clip_planes(_pairs(planes))
                assert len(sc.clip_planes) == {"median": 1, "slab": 2, "eight": 8}[kind]
                for w, h in sizes:
                    label = "%s camera %d %s %dx%d" % (name, k, kind, w, h)
                    want = cc.brute(name, w, h, k, planes)
                    got = _records(sc, w, h, normals=(w, h) == (W, H))
                    sure = _assert_brute(got, want, label, w, h)
                    print("%s: %d hit, %d near, %d not unique" % (label, int((want["item"] >= 0).sum()), int(want["near"].sum()),
                                                                int(((want["item"] >= 0) & ~want["unique"]).sum())))
                    if (w, h) != (W, H):
                        continue
                    # the normal rows of the pixels that hit: the point o + t d, and a unit vector against the ray
                    hit = sure & (want["item"] >= 0)
                    d = ph.rays(name, w, h, k)[0]
                    point = o[None].astype(np.float64) + want["dist"][hit].astype(np.float64)[:, None] * d[hit].astype(np.float64)
                    no = np.asarray(got.normal_origin, np.float32).reshape(h, w, n)[hit]
                    nd = np.asarray(got.normal_dir, np.float32).reshape(h, w, n)[hit]
                    assert np.allclose(no, point, rtol=1e-5, atol=1e-5), label
                    assert np.allclose((nd.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-5) and ((nd * d[hit]).sum(axis=1) <= 1e-6).all(), label
                    if kind == "eight":
                        continue
                    # colours: the oracle's colour of each pixel's own simplex, the background where nothing is left
                    ref = cc.simplex_colors(name, w, h, k, want)
                    img = frame_f32(sc, w, h)
                    clamped = np.clip(ref, 0.0, 1.0)
                    err = np.abs(img - clamped).max(axis=2)
                    assert (err[sure] <= TOL).all(), (label, float(err[sure].max()), int((err[sure] > TOL).sum()))
                    bytes_ = sup.render_host(sc, sup.fmt_of(w, h, fx.RGBX8)).reshape(h, w, 4)
                    wantb = sx.pack(clamped, fx.RGBX8, False).reshape(h, w, 4)
                    assert (np.abs(bytes_.astype(int) - wantb.astype(int))[sure] <= 1).all(), label


@pytest.mark.parametrize("high", cc.HIGH, ids=lambda v: "n%d" % v[0])
def test_the_run_time_n_kernels_cut_a_wide_comb(high):
    n, depth = high
    s, d, aabb, plane, plain, cut = cc.high(n, depth)
    h, w = aabb.shape
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, {})
        sc = tracern.CompositeScene.from_flat(n, s.flat)
        sc.set_params_flat(s.params)
        sc.set_fov(float(s.fov))
        sc._set_camera_arrays(s.origin, s.axes)
        _assert_brute(_records(sc, w, h), plain, "wide comb n = %d without planes" % n, w, h)
        sc.set_clip_planes(_pairs(plane))
        _assert_brute(_records(sc, w, h), cut, "wide comb n = %d under one plane" % n, w, h)
        moved = (plain["item"] >= 0) & (cut["item"] >= 0) & (plain["dist"] != cut["dist"])
        assert moved.sum() >= cc.MIN_MOVED
        # the render shows the cut: a pixel that lost its surface is background, as the plain render has it where nothing is hit
        img = frame_f32(sc, w, h)
        sc.set_clip_planes(None)
        base = frame_f32(sc, w, h)
        lost = (plain["item"] >= 0) & (cut["item"] < 0) & ~cut["near"]
        same = (plain["item"] == cut["item"]) & (plain["lane"] == cut["lane"]) & ~cut["near"] & cut["unique"]
        assert lost.sum() >= cc.MIN_LOST and np.abs(img - base)[same].max() <= TOL
        assert (np.abs(img - base)[moved & ~cut["near"]].max(axis=1) > TOL).sum() >= cc.MIN_MOVED


@pytest.mark.parametrize("name", cc.TWO_SHELLS)
def test_a_slab_over_two_shells_moves_pixels_to_the_far_shell(name):
    """N = 5, 7 and 10 (loose triangles) under a finite t1 with something behind the cut: the brute force on both shells"""
    n, both, params, (o, axes), d, aabb, planes, plain, cut = cc.two_shells(name)
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, {})
        sc = tracern.CompositeScene.from_flat(n, both)
        sc.set_params_flat(params)
        sc.set_fov(ph.fov_of(name))
        sc._set_camera_arrays(o, axes)
        _assert_brute(_records(sc, W, H), plain, "%s two shells without planes" % name, W, H)
        base = frame_f32(sc, W, H)
        sc.set_clip_planes(_pairs(planes))
        sure = _assert_brute(_records(sc, W, H), cut, "%s two shells under the slab" % name, W, H)
        img = frame_f32(sc, W, H)
        moved = sure & (plain["item"] >= 0) & (cut["item"] >= 0) & (plain["dist"] != cut["dist"])
        same = sure & (plain["item"] == cut["item"]) & (plain["lane"] == cut["lane"])
        assert moved.sum() >= cc.MIN_MOVED and np.abs(img - base)[same].max() <= TOL
        assert (np.abs(img - base)[moved].max(axis=1) > TOL).sum() >= cc.MIN_MOVED


# ------------------------------------------------------------------ Reference B
def _twin_scene(t, mp, env=None):
    _env(mp, env or {})
    n, both, emptied, params, plane, cams = cc.twin(*t)
    sc = tracern.CompositeScene.from_flat(n, both)
    sc.set_params_flat(params)
    sc.set_fov(ph.fov_of(t[0]))
    sc.set_clip_planes(_pairs(plane))
    return sc, cams


def _assert_twin(sc, t, k, label):
    want = cc.twin_expected(t[0], t[1], k)
    got = sc.primary_hits(W, H)
    gd = np.asarray(got.dist, np.float32).reshape(H, W)
    assert np.array_equal(gd.view(np.uint32), want["dist"].view(np.uint32)), (label, int((gd != want["dist"]).sum()))
    for key in ("item", "lane", "n_transparent"):
        assert np.array_equal(np.asarray(getattr(got, key)).reshape(H, W), want[key]), (label, key)
    img = frame_f32(sc, W, H)
    err = np.abs(img - np.clip(want["frame"], 0.0, 1.0)).max(axis=2)
    assert err.max() <= TOL, (label, float(err.max()), int((err > TOL).sum()))


TWIN_RUNS = [(t, {}) for t in cc.TWINS] + [(("cell600_n4", "lit"), {"NTRACER_FORCE_VAR": "1"}), (("cell600_n4", "glass"), {"NTRACER_FORCE_VAR": "1"}),
                                          (("cell600_n4", "glass-split"), {"NTRACER_FORCE_VAR": "1"}),
                                          (("cell600_n4", "reflective"), {"NTRACER_COMPOSITE_KERNEL": "2"})]


@pytest.mark.parametrize("run", TWIN_RUNS, ids=lambda r: cc.twin_id(r[0]) + "".join("," + k[len("NTRACER_"):] for k in r[1]))
def test_the_cut_away_twin_does_not_exist(run):
    t, env = run
    with pytest.MonkeyPatch.context() as mp:
        sc, cams = _twin_scene(t, mp, env)
        for k in cc.TWIN_CAMERAS:
            sc._set_camera_arrays(*cams[k])
            _assert_twin(sc, t, k, "%s camera %d %r" % (cc.twin_id(t), k, env))


@pytest.mark.parametrize("t", [("cell600_n4", "lit"), ("cell600_n4", "glass")], ids=cc.twin_id)
def test_a_camera_table_in_chunks_of_two_frames(t):
    import torch
    with pytest.MonkeyPatch.context() as mp:
        sc, cams = _twin_scene(t, mp, {"NTRACER_CHUNK_FRAMES": "2"})
        order = (0, 1, 0)
        table = CameraTable(sc.dimension, np.asarray([cams[k][0] for k in order]), np.asarray([cams[k][1] for k in order]))
        fmt = sup.fmt_of(W, H, fx.RGBF32)
        size = fmt.pitch * H
        buf = torch.full((3 * size + 16,), 0x3D, dtype=torch.uint8, device="cuda")
        fst = fmt._as_struct()
        _lib.check(_lib.lib().nt_render_table_device(sc._handle, C.c_void_p(buf.data_ptr()), size, table._h, 0, 3, C.byref(fst), None,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[3 * size:] == 0x3D).all()
        hits = sc.primary_hits(W, H, table=table, device="cuda")
        for f, k in enumerate(order):
            want = cc.twin_expected(t[0], t[1], k)
            img = got[f * size:(f + 1) * size].view(">f4").astype(np.float32).reshape(H, W, 3)
            assert np.abs(img - np.clip(want["frame"], 0.0, 1.0)).max() <= TOL, (cc.twin_id(t), f)
            assert np.array_equal(hits.item[f].cpu().numpy().reshape(H, W), want["item"]), (cc.twin_id(t), f)
            assert np.array_equal(hits.dist[f].cpu().numpy().reshape(H, W).view(np.uint32), want["dist"].view(np.uint32)), (cc.twin_id(t), f)
            assert np.array_equal(hits.n_transparent[f].cpu().numpy().reshape(H, W), want["n_transparent"]), (cc.twin_id(t), f)


@pytest.mark.parametrize("env", [{}, {"NTRACER_CLEAN_NORMALS": "1"}], ids=["", "CLEAN_NORMALS"])
def test_a_batch_cut_between_its_simplices_is_still_tested_for_what_it_keeps(env):
    """the transparent leaf's last-test rule (clip_cases.one_leaf): a miss behind a batch that lost ONE simplex to the plane is
    today's miss, and the transparent hits of the leaf are trimmed by it as the oracle trims them without that simplex"""
    n, flat, removed, params, plane, (o, axes) = cc.one_leaf()
    w, h = 9, 7
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, env)
        sc = tracern.CompositeScene.from_flat(n, flat)
        sc.set_params_flat(params)
        sc.set_fov(0.8)
        sc._set_camera_arrays(o, axes)
        for which, planes in (("whole", None), ("removed", _pairs(plane))):
            sc.set_clip_planes(planes)
            want = cc.one_leaf_views(which, w, h)
            got = sc.primary_hits(w, h)
            assert np.array_equal(np.asarray(got.dist, np.float32).reshape(h, w).view(np.uint32), want["dist"].view(np.uint32)), which
            for key in ("item", "lane", "n_transparent"):
                assert np.array_equal(np.asarray(getattr(got, key)).reshape(h, w), want[key]), (which, key)
            assert np.abs(frame_f32(sc, w, h) - np.clip(want["frame"], 0.0, 1.0)).max() <= TOL, which


# ------------------------------------------------------------------ further checks
@pytest.mark.parametrize("scene", [("cell600_n4", "lit", {}), ("simplex10_n10", "", {}), ("cell600_n4", "glass", {}),
                                   ("cell600_n4", "lit", {"NTRACER_FORCE_VAR": "1"})],
                         ids=lambda s: s[0] + "," + s[1] + "".join("," + k[len("NTRACER_"):] for k in s[2]))
def test_planes_that_keep_the_whole_box_change_nothing(scene):
    name, variant, env = scene
    with pytest.MonkeyPatch.context() as mp:
        if variant == "glass":
            # transparent materials on the general route: the twin as it stands, both halves kept
            _env(mp, env)
            n, both, emptied, params, plane, cams = cc.twin(name, "glass")
            sc = tracern.CompositeScene.from_flat(n, both)
            sc.set_params_flat(params)
            sc.set_fov(ph.fov_of(name))
            sc._set_camera_arrays(*cams[0])
            lo, hi = np.asarray(both["aabb_start"], np.float64), np.asarray(both["aabb_end"], np.float64)
            keep = (np.concatenate([np.eye(n)[:4], -np.eye(n)[:4]]).astype(np.float32),
                    np.concatenate([hi[:4] + 2 * (hi - lo)[:4], -lo[:4] + 2 * (hi - lo)[:4]]).astype(np.float32))
            assert (np.asarray(both["materials"])[:, 6] < 1).any()
        else:
            sc = _golden(name, mp, variant=variant, env=env)
            keep = cc.keep_all(name)
        for fmt in (sup.fmt_of(W, H, fx.RGBF32), sup.fmt_of(W, H, fx.RGBX8)):
            sc.set_clip_planes(None)
            plain = sup.render_host(sc, fmt)
            r0 = sc.primary_hits(W, H, normals=True)
            sc.set_clip_planes(_pairs(keep))
            assert np.array_equal(sup.render_host(sc, fmt), plain), (name, variant)
            r1 = sc.primary_hits(W, H, normals=True)
            for key in ("dist", "item", "lane", "n_transparent", "normal_origin", "normal_dir"):
                a, b = np.asarray(getattr(r0, key)), np.asarray(getattr(r1, key))
                assert a.tobytes() == b.tobytes(), (name, variant, key)
        assert (np.asarray(r0.item) >= 0).sum() >= 5
        if variant == "glass":
            assert (np.asarray(r0.n_transparent) > 0).sum() >= 5


@pytest.mark.parametrize("scene", [("cell600_n4", "lit", {}), ("cell600_n4", "lit", {"NTRACER_FORCE_VAR": "1"})],
                         ids=lambda s: s[0] + "".join("," + k[len("NTRACER_"):] for k in s[2]))
def test_an_empty_keep_region_gives_the_background(scene):
    name, variant, env = scene
    with pytest.MonkeyPatch.context() as mp:
        sc = _golden(name, mp, variant=variant, env=env)
        sc.set_clip_planes(_pairs(cc.keep_nothing(name)))
        r = sc.primary_hits(W, H)
        assert (np.asarray(r.item) == -1).all() and (np.asarray(r.lane) == -1).all() and (np.asarray(r.n_transparent) == 0).all()
        assert (np.asarray(r.dist, np.float32) == np.float32(cc.FLT_MAX)).all()
        nothing = dict(item=np.full((H, W), -1, np.int32), lane=np.full((H, W), -1, np.int32))
        ref = np.clip(cc.simplex_colors(name, W, H, 0, nothing), 0.0, 1.0)
        assert np.abs(frame_f32(sc, W, H) - ref).max() <= TOL


def test_the_two_routes_agree_on_a_lit_scene_cut_through_its_primitives():
    """a consistency check only: neither side is a reference (Reference A and B are the checks against the oracle)"""
    w, h = 64, 48
    frames, records = [], []
    for env in ({}, {"NTRACER_FORCE_VAR": "1"}):
        with pytest.MonkeyPatch.context() as mp:
            sc = _golden("cell600_n4", mp, k=1, variant="lit", env=env)
            sc.set_clip_planes(_pairs(cc.planes("cell600_n4", "median", 1)))
            frames.append(frame_f32(sc, w, h))
            records.append(sc.primary_hits(w, h))
    for key in ("dist", "item", "lane", "n_transparent"):
        assert np.asarray(getattr(records[0], key)).tobytes() == np.asarray(getattr(records[1], key)).tobytes(), key
    assert (np.asarray(records[0].item) >= 0).sum() >= 300
    assert np.abs(frames[0] - frames[1]).max() <= TOL
