"""View stacks without a GPU: nt_view_stack_cameras and Scene.view_stack_cameras against the numpy restatement of the rule
(tests/view_stack_cases.py) bit for bit, the setter and getter, every NT_E_INVALID, the three helpers, and the refusals of a
render with the setting on as literal strings -- every one of them comes before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import box_hit_cases as bc
import fixtures as fx
import ntracer_amd
import ray_query_cases as rq
import view_stack_cases as vc
from ntracer_amd import _lib, tracern

W, H = 8, 4
f32 = np.float32


def _box(n=6):
    return tracern.BoxScene(n)


def _composite(name="cell120_n4"):
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat)


def _table(n, K, seed):
    """offsets with every component set, the hidden ones included"""
    return np.random.default_rng(seed).uniform(-0.3, 0.3, (K, n)).astype(f32)


# ------------------------------------------------------------------ 1. the cameras
@pytest.mark.parametrize("n", (3, 6, 25, 64))
@pytest.mark.parametrize("focus", (None, 2.75), ids=("translations", "focus"))
def test_the_sample_cameras_equal_the_rule_bit_for_bit(n, focus):
    rng = np.random.default_rng(7 * n)
    q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    cams = {"orthonormal": (rng.uniform(-3, 3, n).astype(f32), q.astype(f32)), "stress-3": fx.stress_cameras(n, np.random.default_rng(n))[3],
            "diagonal": bc.camera(n, 4)}
    a = cams["orthonormal"][1].astype(np.float64)
    assert np.allclose(a @ a.T, np.eye(n), atol=1e-5)
    s = np.asarray(cams["diagonal"][1], np.float64)
    assert not np.allclose(s @ s.T, np.eye(n), atol=1e-3)          # (raw, non-orthonormal axes)
    for K in (1, 5, 64):
        e = _table(n, K, 100 * n + K)
        sc = _box(n)
        sc.set_view_stack(e, focus)
        for name, (o, ax) in cams.items():
            o, ax = np.ascontiguousarray(o, f32), np.ascontiguousarray(ax, f32).reshape(n, n)
            want_o, want_a = vc.rule_cameras(o, ax, e, focus)
            # the C entry point with a camera of the caller's
            got_o, got_a = np.full((K, n), 7, f32), np.full((K, n, n), 7, f32)
            _lib.check(_lib.lib().nt_view_stack_cameras(sc._handle, o.ctypes.data_as(_lib.f32p), ax.ctypes.data_as(_lib.f32p),
                                                        got_o.ctypes.data_as(_lib.f32p), got_a.ctypes.data_as(_lib.f32p)))
            assert np.array_equal(got_o.view(np.uint32), want_o.view(np.uint32)), (n, K, name)
            assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), (n, K, name)
            # the method, with the scene's own camera (NULL origin and axes)
            sc._set_camera_arrays(o, ax)
            got_o, got_a = sc.view_stack_cameras()
            assert np.array_equal(got_o.view(np.uint32), want_o.view(np.uint32)) and np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))
            # only the origin and the forward row move
            keep = [r for r in range(n) if r != 2]
            assert np.array_equal(got_a[:, keep], np.broadcast_to(ax[keep], (K, n - 1, n)))
            if focus is None:
                assert np.array_equal(got_a[:, 2], np.broadcast_to(ax[2], (K, n)))
            else:
                assert not np.array_equal(got_a[:, 2], np.broadcast_to(ax[2], (K, n)))


def test_with_a_focus_the_rays_of_a_pixel_meet_on_the_focal_plane():
    """on the cameras the library hands out"""
    n, focus = 6, 3.0
    o, ax = bc.camera(n, 4)
    e = _table(n, 7, 3)
    e[:, 2:] = 0                                                    # a lens: offsets in the right/up plane
    sc = _box(n)
    sc._set_camera_arrays(o, ax)
    sc.set_view_stack(e, focus)
    origins, axes = sc.view_stack_cameras()
    for cx, cy in ((0.0, 0.0), (0.3, -0.2)):
        target = o + focus * (ax[2] + cx * ax[0] - cy * ax[1])
        for k in range(len(e)):
            p = origins[k] + focus * (axes[k, 2] + cx * axes[k, 0] - cy * axes[k, 1])
            assert np.allclose(p, target, atol=1e-5)


# ------------------------------------------------------------------ 2. the setter and the getter
@pytest.mark.parametrize("make", (_box, _composite), ids=("box", "composite"))
def test_the_setting_round_trips_on_both_scene_kinds(make):
    sc = make()
    n = sc.dimension
    assert sc.view_stack is None
    e = _table(n, 9, 1)
    w = np.random.default_rng(2).uniform(0, 0.4, (9, 3)).astype(f32)
    sc.set_view_stack(e, 2.5, w)
    vs = sc.view_stack
    assert np.array_equal(vs["offsets"], e) and np.array_equal(vs["weights"], w) and vs["focus"] == 2.5
    sc.set_view_stack(e[:4])
    vs = sc.view_stack
    assert vs["focus"] is None and np.array_equal(vs["offsets"], e[:4])
    assert np.array_equal(vs["weights"].view(np.uint32), np.full((4, 3), f32(1) / f32(4), f32).view(np.uint32))
    # the C getter with NULL pointers, and the count alone
    count = C.c_int(-1)
    _lib.check(_lib.lib().nt_scene_get_view_stack(sc._handle, C.byref(count), None, None, None))
    assert count.value == 4
    sc.set_view_stack(None)
    assert sc.view_stack is None
    with pytest.raises(ValueError, match="no view stack is set"):
        sc.view_stack_cameras()
    out = np.zeros((1, n * n), f32)
    assert _lib.lib().nt_view_stack_cameras(sc._handle, None, None, out.ctypes.data_as(_lib.f32p), out.ctypes.data_as(_lib.f32p)) == _lib.NT_E_INVALID
    assert _lib.last_error() == "the view stack is off (nt_scene_set_view_stack)"


def test_the_route_setting_round_trips_and_refuses_other_values():
    for sc in (_box(5), _composite()):
        assert sc.view_stack_route is None
        sc.set_view_stack_route("frames")
        assert sc.view_stack_route == "frames" and _lib.lib().nt_scene_get_view_stack_route(sc._handle) == _lib.NT_STACK_ROUTE_FRAMES
        for bad in (2, -1):
            assert _lib.lib().nt_scene_set_view_stack_route(sc._handle, bad) == _lib.NT_E_INVALID and sc.view_stack_route == "frames"
        with pytest.raises(ValueError):
            sc.set_view_stack_route("fused")
        _lib.check(_lib.lib().nt_scene_lock(sc._handle))
        try:
            assert _lib.lib().nt_scene_set_view_stack_route(sc._handle, 0) == _lib.NT_E_LOCKED
        finally:
            _lib.check(_lib.lib().nt_scene_unlock(sc._handle))
        sc.set_view_stack_route(None)
        assert sc.view_stack_route is None
    assert _lib.lib().nt_scene_set_view_stack_route(None, 0) == _lib.NT_E_INVALID


def test_the_setting_is_not_pickled():
    """a view setting like fov, kept in the native handle: no part of what is pickled"""
    import pickle
    for sc in (_box(5), _composite()):
        before = pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2)
        sc.set_view_stack(_table(sc.dimension, 3, 1), 2.0)
        assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before


def test_a_locked_scene_keeps_its_setting():
    sc = _box(5)
    e = _table(5, 3, 1)
    sc.set_view_stack(e)
    _lib.check(_lib.lib().nt_scene_lock(sc._handle))
    try:
        assert _lib.lib().nt_scene_set_view_stack(sc._handle, 0, None, 0.0, None) == _lib.NT_E_LOCKED
    finally:
        _lib.check(_lib.lib().nt_scene_unlock(sc._handle))
    assert np.array_equal(sc.view_stack["offsets"], e)


# ------------------------------------------------------------------ 3. NT_E_INVALID
def test_every_invalid_value_is_refused_and_the_setting_stays():
    L = _lib.lib()
    sc = _box(6)
    n = 6
    good = _table(n, 3, 5)
    sc.set_view_stack(good, 2.0)
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.f32p)
    bad_off = [good.copy() for _ in range(3)]
    bad_off[0][1, 4] = np.nan
    bad_off[1][2, 0] = np.inf
    bad_off[2][0, 5] = -np.inf
    w = np.full((3, 3), 0.25, f32)
    bad_w = [w.copy(), w.copy()]
    bad_w[0][2, 1] = np.nan
    bad_w[1][0, 0] = np.inf
    many = np.zeros((65, n), f32)
    calls = [(-1, good, 0.0, None), (65, many, 0.0, None), (3, None, 0.0, None), (3, good, -1.0, None), (3, good, float("nan"), None),
             (3, good, float("inf"), None), (3, good, 1e-45, None),
             (0, None, -1.0, None), (0, None, float("nan"), None), (0, good, float("inf"), None)]       # a bad focus, also when taking it off
    calls += [(3, b, 0.0, None) for b in bad_off] + [(3, good, 0.0, b) for b in bad_w]
    for count, off, focus, wt in calls:
        assert L.nt_scene_set_view_stack(sc._handle, count, p(off), focus, p(wt)) == _lib.NT_E_INVALID, (count, focus)
        assert _lib.last_error()
        vs = sc.view_stack
        assert np.array_equal(vs["offsets"], good) and vs["focus"] == 2.0
    assert L.nt_scene_set_view_stack(None, 0, None, 0.0, None) == _lib.NT_E_INVALID
    # 64 samples are accepted, and the method checks the shapes
    L_ok = L.nt_scene_set_view_stack(sc._handle, 64, p(many[:64]), 0.0, None)
    assert L_ok == 0 and len(sc.view_stack["offsets"]) == 64
    for off, focus, wt in ((np.zeros((3, 5), f32), None, None), (np.zeros(6, f32), None, None), (good, 0.0, None), (good, -2.0, None),
                           (good, True, None), (good, None, np.zeros((2, 3), f32))):
        with pytest.raises(ValueError):
            sc.set_view_stack(off, focus, wt)


# ------------------------------------------------------------------ 4. the helpers
def test_the_helpers_make_the_usual_tables():
    off, w = ntracer_amd.aperture_disc(6, 9, 0.25)
    assert off.shape == (9, 6) and off.dtype == f32 and w.shape == (9, 3) and w.dtype == f32
    assert not off[0].any() and not off[:, 2:].any()
    rad = np.sqrt((off.astype(np.float64) ** 2).sum(axis=1))
    assert (rad <= 0.25 + 1e-6).all() and abs(rad[-1] - 0.25) < 1e-6 and len({tuple(r) for r in off}) == 9
    assert np.allclose(w.sum(axis=0), 1.0, atol=1e-6)
    assert np.array_equal(ntracer_amd.aperture_disc(6, 9, 0.25)[0], off)                      # the same table every time
    off, w = ntracer_amd.slab(5, 4, 0.5, 7)
    assert off.shape == (7, 5) and w.shape == (7, 3) and not off[:, :4].any()
    assert np.allclose(off[:, 4], np.linspace(-0.5, 0.5, 7), atol=1e-7) and np.allclose(w.sum(axis=0), 1.0, atol=1e-6)
    lo, mid, hi = (0.2, 0.3, 1.0), (1.0, 1.0, 1.0), (1.0, 0.3, 0.2)
    off, w = ntracer_amd.slab(5, 3, 0.5, 5, colors=(lo, mid, hi))
    assert np.allclose(w * 5, [lo, np.add(lo, mid) / 2, mid, np.add(mid, hi) / 2, hi], atol=1e-6)
    off, w = ntracer_amd.stereo_pair(4, 0.5)
    assert np.array_equal(off, np.asarray([[-0.25, 0, 0, 0], [0.25, 0, 0, 0]], f32)) and np.array_equal(w, np.asarray([[1, 0, 0], [0, 1, 1]], f32))
    for bad in (lambda: ntracer_amd.slab(5, 2, 0.5, 3), lambda: ntracer_amd.slab(3, 3, 0.5, 3), lambda: ntracer_amd.aperture_disc(6, 65, 0.1),
                lambda: ntracer_amd.aperture_disc(6, 0, 0.1), lambda: ntracer_amd.slab(5, 3, 0.5, 65), lambda: ntracer_amd.stereo_pair(2, 0.1)):
        with pytest.raises(ValueError):
            bad()
    # what a helper returns is what the setter takes
    sc = _box(6)
    off, w = ntracer_amd.slab(6, 3, 0.2, 5)
    sc.set_view_stack(off, None, w)
    assert np.array_equal(sc.view_stack["weights"], w)


# ------------------------------------------------------------------ 5. the refusals
REFUSALS = {
    "supersampling": "a view stack is not available with a supersampling factor above 1 (2)",
    "bands": "a view stack is not available with row bands (band_world 2)",
    "collect_stats": "a view stack is not available with collect_stats",
    "lens": "a view stack is not available while a lens is set",
    "parallel": "a view stack is not available while the parallel projection is set",
    "clip": "a view stack is not available while clip planes are set",
    "cue": "a view stack is not available while depth cues are on",
    "outlines": "a view stack is not available while outlines are on",
    "ao": "a view stack is not available while ambient occlusion is on",
    "face lines": "a view stack is not available while face lines are set",
    "face shading": "a view stack is not available while face shading is set",
}
# cause -> (what sets it up on the scene, the options of the call)
CAUSES = {
    "supersampling": (lambda s: s.set_supersampling(2), None),
    "bands": (None, dict(band_world=2)),
    "collect_stats": (None, dict(collect_stats=1)),
    "lens": (lambda s: s.set_lens(tracern.Lens.pinhole(W, H, 0.8)), None),
    "parallel": (lambda s: s.set_parallel_projection(2.0), None),
    "clip": (lambda s: s.set_clip_planes([((1.0,) + (0.0,) * (s.dimension - 1), 1.0)]), None),
    "cue": (lambda s: s.set_depth_cue(1.0, 2.0), None),
    "outlines": (lambda s: s.set_outlines(), None),
    "ao": (lambda s: s.set_ambient_occlusion(4, 1.0), None),
    "face lines": (lambda s: s.set_face_lines(), None),
    "face shading": (lambda s: s.set_face_shading(near=1.0, far=2.0), None),
}
BOX_ONLY = ("face lines", "face shading")
COMPOSITE_ONLY = ("clip", "cue", "outlines", "ao")


def _answers(scene, fields):
    """[(status, message)] of nt_render and nt_render_device into one marked destination, and whether it is as it was"""
    L = _lib.lib()
    fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in fx.RGBX8])
    fst = fmt._as_struct()
    size = fmt.pitch * H
    dest = (C.c_char * size)(*([0x4E] * size))
    opts = None
    if fields is not None:
        opts = _lib.NtRenderOpts()
        opts.device = -1
        for k, v in fields.items():
            setattr(opts, k, v)
    po = None if opts is None else C.byref(opts)
    out = []
    for call in (lambda: L.nt_render(scene._handle, dest, size, C.byref(fst), po, None),
                 lambda: L.nt_render_device(scene._handle, dest, size, C.byref(fst), po, None)):
        status = call()
        out.append((status, _lib.last_error()))
    return out, bytes(dest) == b"\x4e" * size


@pytest.mark.parametrize("cause", sorted(REFUSALS))
def test_a_render_with_the_stack_on_is_refused_in_these_words(cause):
    kinds = [_box] if cause in BOX_ONLY else [_composite] if cause in COMPOSITE_ONLY else [_box, _composite]
    for make in kinds:
        sc = make()
        sc.set_view_stack(np.zeros((2, sc.dimension), f32))
        setup, fields = CAUSES[cause]
        if setup:
            setup(sc)
        answers, untouched = _answers(sc, fields)
        for status, message in answers:
            assert status == _lib.NT_E_UNSUPPORTED, (status, message)
            assert message == REFUSALS[cause]
        assert untouched


def test_the_stack_refuses_first_and_with_it_off_the_checks_answer_as_before():
    import view_setting_refusals as vr
    sc = _composite()
    sc.set_depth_cue(1.0, 2.0)
    sc.set_supersampling(2)
    before, _ = _answers(sc, None)
    assert [m for _, m in before] == [vr.RENDER_REFUSALS["cue", "supersampling"]] * 2
    sc.set_view_stack(np.zeros((1, sc.dimension), f32))
    during, untouched = _answers(sc, None)
    assert [m for _, m in during] == [REFUSALS["supersampling"]] * 2 and untouched
    sc.set_view_stack(None)
    after, _ = _answers(sc, None)
    assert after == before
    # the queries of the other settings ignore the stack: they answer what they answered without it
    sc.set_supersampling(1)
    sc.set_view_stack(np.zeros((1, sc.dimension), f32))
    out = np.zeros(W * H * 8, np.uint8)
    opts = _lib.NtRenderOpts()
    opts.device = -1
    opts.band_world = 2
    assert _lib.lib().nt_depth_cue_factors_device(sc._handle, W, H, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID
    assert _lib.last_error() == vr.QUERY_REFUSALS["nt_depth_cue_factors", "options: band_world"][1]


def test_the_cases_of_the_gpu_tests_show():
    """from the oracle alone: every stack changes at least 50 of the 777 pixels of the 37 x 21 view, at every dimension and
    scene the GPU tests use -- and the sample cameras those expectations were made with are, bit for bit, the library's"""
    low = 777

    def same_cameras(sc, o, a, st, want):
        sc._set_camera_arrays(o, a)
        sc.set_view_stack(*st)
        got = sc.view_stack_cameras()
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for n in vc.BOX_FUSED_DIMS + vc.BOX_FRAMES_DIMS:
        for k in vc.BOX_CAMERAS:
            for name in vc.stacks_of(n):
                st = vc.box_stack(n, k, name)
                o, a = bc.camera(n, k)
                same_cameras(_box(n), o, a, st, vc.rule_cameras(o, a, st[0], st[1]))
                if name != "one":
                    low = min(low, vc.check_box_shows(n, k, name))
    for case in vc.COMPOSITE[:4]:
        for name in vc.STACKS:
            st = vc.composite_stack(case, name)
            same_cameras(_composite(case[0]), *vc.composite_camera(case), st, vc.composite_cameras(case, name))
            if name != "one":
                low = min(low, vc.check_composite_shows(case, name))
    assert low >= vc.MIN_SHOWN
    # and K = 1 with a zero offset is the plain frame
    w, h = vc.SHOW_SIZE
    assert np.array_equal(vc.box_expected(6, 2, "one", w, h).view(np.uint32), vc.box_plain(6, 2, w, h).view(np.uint32))
