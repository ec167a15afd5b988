"""Adaptive supersampling (nt_scene_set_adaptive_supersampling / scene.set_adaptive_supersampling), the part that needs no GPU:
the setting as a scene attribute -- default, round trips, refused values, the lock, pickling, with_rebuilt_tree() --, the
header's text, the refusals, which answer before a device is touched, the expected-image builder of tests/adaptive_cases.py at
the threshold's extremes, the conditions its cases were chosen by, and the launches of the new launchers pinned to those cases."""
import ctypes as C
import math
import os
import pickle
import re

import numpy as np
import pytest

import adaptive_cases as ac
import fixtures as fx
import oracle_binding as ob
import ss_expected as sx
import support as sup
from ntracer_amd import Channel, ImageFormat, _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def box():
    return tracern.BoxScene(5)


def composite():
    return tracern.CompositeScene.from_flat(4, fx.flat_of(fx.load("cell600_n4")))


SCENES = [box, composite]


def get(sc):
    on, t = C.c_int(-1), C.c_float(-1.0)
    assert _lib.lib().nt_scene_get_adaptive_supersampling(sc._handle, C.byref(on), C.byref(t)) == _lib.NT_OK
    return on.value, t.value


@pytest.mark.parametrize("make", SCENES)
def test_the_setting_is_off_by_default(make):
    sc = make()
    assert sc.adaptive_supersampling is None
    assert get(sc) == (0, 0.0)


@pytest.mark.parametrize("make", SCENES)
def test_round_trips_through_the_abi_and_python(make):
    sc = make()
    L = _lib.lib()
    for t in (0.1, 0.02, -1.0, 2.0, 0.0):
        assert L.nt_scene_set_adaptive_supersampling(sc._handle, 1, t) == _lib.NT_OK
        assert get(sc) == (1, float(f32(t))) and sc.adaptive_supersampling == float(f32(t))
    for t in (0.25, 1, np.float32(0.5), -3):
        sc.set_adaptive_supersampling(t)
        assert sc.adaptive_supersampling == float(t) and get(sc) == (1, float(t))
    sc.set_adaptive_supersampling(None)
    assert sc.adaptive_supersampling is None and get(sc) == (0, 0.0)
    assert L.nt_scene_set_adaptive_supersampling(sc._handle, 1, 0.3) == _lib.NT_OK
    assert L.nt_scene_set_adaptive_supersampling(sc._handle, 0, 0.7) == _lib.NT_OK          # off: the threshold is dropped
    assert get(sc) == (0, 0.0)
    with pytest.raises(AttributeError):
        sc.adaptive_supersampling = 0.1                       # read-only, like fov
    # either pointer of the getter may be NULL; the factor is another setting
    assert L.nt_scene_get_adaptive_supersampling(sc._handle, None, None) == _lib.NT_OK
    assert L.nt_scene_set_adaptive_supersampling(None, 1, 0.1) == _lib.NT_E_INVALID
    assert L.nt_scene_get_adaptive_supersampling(None, None, None) == _lib.NT_E_INVALID
    sc.set_adaptive_supersampling(0.1)
    assert sc.supersampling == 1
    sc.set_supersampling(3)
    assert sc.adaptive_supersampling == float(f32(0.1))


@pytest.mark.parametrize("make", SCENES)
def test_nan_and_infinite_thresholds_are_refused_and_change_nothing(make):
    sc = make()
    L = _lib.lib()
    sc.set_adaptive_supersampling(0.25)
    for bad in (math.nan, math.inf, -math.inf):
        assert L.nt_scene_set_adaptive_supersampling(sc._handle, 1, bad) == _lib.NT_E_INVALID
        assert "finite" in _lib.last_error()
        with pytest.raises(ValueError):
            sc.set_adaptive_supersampling(bad)
        assert sc.adaptive_supersampling == 0.25
    for bad in ("0.1", True, [0.1]):
        with pytest.raises(ValueError):
            sc.set_adaptive_supersampling(bad)
    assert sc.adaptive_supersampling == 0.25
    sc.set_adaptive_supersampling(None)
    assert L.nt_scene_set_adaptive_supersampling(sc._handle, 1, math.nan) == _lib.NT_E_INVALID
    assert sc.adaptive_supersampling is None


@pytest.mark.parametrize("make", SCENES)
def test_a_locked_scene_refuses(make):
    sc = make()
    L = _lib.lib()
    sc.set_adaptive_supersampling(0.25)
    assert L.nt_scene_lock(sc._handle) == _lib.NT_OK
    try:
        assert L.nt_scene_set_adaptive_supersampling(sc._handle, 1, 0.5) == _lib.NT_E_LOCKED
        assert L.nt_scene_set_adaptive_supersampling(sc._handle, 0, 0.0) == _lib.NT_E_LOCKED
        with pytest.raises(_lib.LockedError):
            sc.set_adaptive_supersampling(0.5)
        with pytest.raises(_lib.LockedError):
            sc.set_adaptive_supersampling(None)
        assert sc.adaptive_supersampling == 0.25
    finally:
        assert L.nt_scene_unlock(sc._handle) == _lib.NT_OK
    sc.set_adaptive_supersampling(0.5)
    assert sc.adaptive_supersampling == 0.5


def test_the_setting_is_no_part_of_what_is_pickled():
    """like the factor (tests/test_supersampling_host.py): it lives in the native handle"""
    for make in SCENES:
        sc = make()
        before = pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2)
        sc.set_adaptive_supersampling(0.1)
        assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before
        assert not any("adaptive" in k for k in sc.__dict__)
        assert make().adaptive_supersampling is None


def test_with_rebuilt_tree_carries_the_setting_over():
    sc = composite()
    sc.set_supersampling(3)
    sc.set_adaptive_supersampling(0.125)
    other = sc.with_rebuilt_tree()
    assert other.adaptive_supersampling == 0.125 and other.supersampling == 3
    assert sc.adaptive_supersampling == 0.125
    assert composite().with_rebuilt_tree().adaptive_supersampling is None


def test_the_header_names_the_definition_and_the_refusals():
    with open(os.path.join(ROOT, "include", "ntracer_hip.h")) as f:
        header = f.read()
    raw = C.CDLL(_lib.LIB_PATH)
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in ("nt_scene_set_adaptive_supersampling", "nt_scene_get_adaptive_supersampling", "nt_adaptive_mask", "nt_adaptive_mask_device"):
        assert re.search(r"\bint %s\((const )?nt_scene_t \*s," % name, header), name
        assert hasattr(raw, name) and name in declared, name
    text = re.sub(r"\s+", " ", header)
    for phrase in ("contrast > t", "four neighbours", "clamped to [0, 1]", "row-major order", "(float)(s*s)", "t < 0 flags every pixel",
                   "t >= 1 flags none", "s = 1 the setting changes nothing", "thinner than a pixel", "row bands (band_world > 1)",
                   "collect_stats", "NaN or infinite", "NT_E_LOCKED", "NT_E_INVALID when the threshold is off"):
        assert phrase in text, phrase


@pytest.mark.parametrize("kind", ["composite", "box"])
def test_what_the_setting_refuses_is_refused_before_a_device_is_touched(kind):
    """every refusal below answers on a machine without a GPU, where anything that reached for a device would say NT_E_DEVICE"""
    L = _lib.lib()
    if kind == "composite":
        n = 4
        sc = composite()
    else:
        n = 6
        sc = tracern.BoxScene(n)
    w, h = 8, 5
    fmt = ImageFormat(w, h, [Channel(*c) for c in fx.RGBX8])
    fst = fmt._as_struct()
    dest = np.full(w * h * 4, 0xab, np.uint8)
    mask = np.full(w * h, 0xab, np.uint8)

    def calls(opts=None):
        o = C.byref(opts) if opts is not None else None
        cams = np.zeros((1, n), f32), np.eye(n, dtype=f32)[None].copy()
        return [L.nt_render(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_device(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_frames_device(sc._handle, dest.ctypes.data, dest.nbytes, 1, cams[0].ctypes.data_as(_lib.f32p),
                                          cams[1].ctypes.data_as(_lib.f32p), C.byref(fst), o, None)]

    def mask_calls(opts=None):
        o = C.byref(opts) if opts is not None else None
        return [L.nt_adaptive_mask(sc._handle, w, h, mask.ctypes.data, None, o), L.nt_adaptive_mask_device(sc._handle, w, h, mask.ctypes.data, o, None)]
    bands = _lib.NtRenderOpts()
    bands.device, bands.band_world, bands.band_rank = -1, 2, 1
    stats = _lib.NtRenderOpts()
    stats.device, stats.collect_stats = -1, 1
    # the mask wants the threshold
    for r in mask_calls():
        assert r == _lib.NT_E_INVALID and "threshold is off" in _lib.last_error()
    with pytest.raises(ValueError, match="threshold is off"):
        sc.refinement_mask(w, h)
    sc.set_supersampling(2)
    sc.set_adaptive_supersampling(0.1)
    for opts, word in ((bands, "band"), (stats, "collect_stats")):
        for r in calls(opts) + mask_calls(opts):
            assert r == _lib.NT_E_UNSUPPORTED and "adaptive" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    assert (dest == 0xab).all() and (mask == 0xab).all()                # nothing was drawn
    whole = _lib.NtRenderOpts()
    whole.device, whole.band_world, whole.band_rows = -1, 1, 8           # one band: the whole image, as for every render call
    if L.nt_device_count() == 0:
        for r in calls(whole) + mask_calls(whole):
            assert r == _lib.NT_E_DEVICE
        # past the checks the same calls end at the device, not before; and bands and statistics are refused only while the
        # setting is in force: threshold on and a factor above 1
        for r in calls() + mask_calls():
            assert r == _lib.NT_E_DEVICE
        sc.set_supersampling(1)
        for opts in (bands, stats):
            for r in calls(opts):
                assert r == _lib.NT_E_DEVICE
        sc.set_supersampling(2)
        sc.set_adaptive_supersampling(None)
        for opts in (bands, stats):
            for r in calls(opts):
                assert r == _lib.NT_E_DEVICE
    # a lens and the projection go on refusing the factor, in their own words
    sc.set_supersampling(2)
    sc.set_adaptive_supersampling(0.1)
    sc.set_parallel_projection(1.5)
    for r in calls():
        assert r == _lib.NT_E_UNSUPPORTED and "supersampling" in _lib.last_error() and "parallel" in _lib.last_error()
    for r in mask_calls():
        assert r == _lib.NT_E_UNSUPPORTED and "parallel" in _lib.last_error()
    assert (dest == 0xab).all() and (mask == 0xab).all()


# ------------------------------------------------------------------ the expected-image builder
def test_the_builder_at_the_extremes_of_the_threshold():
    """t < 0 flags every pixel: the supersampled image of ss_expected; t = 2 flags none: the plain oracle frame"""
    n, s = 6, 3
    o, a = ac.box_cameras(n)[7]
    osc = ob.OracleScene(n, o, a)
    mean = sx.mean_colors(osc, ac.W, ac.H, s)
    plain = osc.render(ac.W, ac.H, fx.RGBF32, threads=sup.worker_threads())
    e = ac.expected(osc, ac.W, ac.H, s, -1.0)
    assert e.mask.all() and not e.undecided.any()
    assert np.array_equal(e.pick.view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(e.image(fx.RGBX8), sx.pack(mean, fx.RGBX8))
    e = ac.expected(osc, ac.W, ac.H, s, 2.0)
    assert not e.mask.any() and not e.undecided.any()
    assert np.array_equal(e.image(fx.RGBF32), plain)
    assert np.array_equal(e.image(fx.RGBX8), osc.render(ac.W, ac.H, fx.RGBX8, threads=sup.worker_threads()))
    # in between it mixes the two, and the two differ
    e = ac.expected(osc, ac.W, ac.H, s, ac.T)
    assert np.array_equal(e.pick[e.mask].view(np.uint32), mean[e.mask].view(np.uint32))
    assert np.array_equal(e.pick[~e.mask].view(np.uint32), e.P[~e.mask].view(np.uint32))
    assert not np.array_equal(e.image(fx.RGBX8), sx.pack(mean, fx.RGBX8)) and not np.array_equal(e.image(fx.RGBF32), plain)


def test_the_contrast_is_the_definition_pixel_by_pixel():
    """the vectorised mask against the definition spelt out, on a small frame: borders, corners, and a one-pixel image"""
    rng = np.random.default_rng(5)
    P = rng.random((7, 9, 3)).astype(f32)
    c = ac.contrast(P)
    for y in range(7):
        for x in range(9):
            want = f32(0)
            for xx, yy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if 0 <= xx < 9 and 0 <= yy < 7:
                    want = max(want, np.abs(P[y, x] - P[yy, xx]).astype(f32).max())
            assert c[y, x] == want
    assert ac.contrast(P[:1, :1]).shape == (1, 1) and ac.contrast(P[:1, :1])[0, 0] == 0 and not ac.mask_of(P[:1, :1], 0.0).any()
    assert ac.mask_of(P[:1, :1], -1.0).all()
    assert ac.contrast(P[:1]).shape == (1, 9) and ac.contrast(P[:, :1]).shape == (7, 1)


@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_the_composite_cases_meet_their_conditions(case):
    for s in case[3]:
        ac.check_case(ac.case_expected(case, s), "%s s=%d" % (ac.case_id(case), s))


@pytest.mark.parametrize("n,s", ac.BOX_CASES)
def test_the_box_cases_meet_their_conditions(n, s):
    for k in ac.BOX_CAMERAS:
        ac.check_case(ac.box_expected(n, s, k), "BoxScene(%d) s=%d camera %d" % (n, s, k))


def test_the_shares_the_cases_were_chosen_by():
    """flagged pixels of the 23 751 at t = 0.1, by the oracle: the table the cases were accepted with"""
    got = {ac.case_id(c): int(ac.case_expected(c, c[3][0]).mask.sum()) for c in ac.CASES if not c[1]}
    assert got == {"cell600_n4": 2018, "cell600_n4,lit": 833, "simplex10_n10": 164, "feature5_n5": 946, "feature11_n11": 602, "lit12_n12": 639}, got
    assert [int(ac.box_expected(6, 2, k).mask.sum()) for k in ac.BOX_CAMERAS] == [234, 738, 50]
    assert not ac.mask_of(ac.plain_colors(ob.OracleScene(6, *ac.box_cameras(6)[0]), ac.W, ac.H), ac.T).any()     # stress camera 0 flags nothing


# ------------------------------------------------------------------ the launches
def test_every_launch_of_the_new_launchers_is_reached_by_a_case():
    hpp, var = sup.source("nt_adaptive.hpp"), sup.source("nt_var.hip")
    launched = (sup.launches(sup.function_body(hpp, "int launch_refine_fixed(")) | sup.launches(sup.function_body(hpp, "int launch_refine_box_fixed(")) |
                sup.launches(sup.function_body(hpp, "inline void launch_adaptive_flag(")) | sup.launches(sup.function_body(var, "int nt_launch_refine(")))
    assert len(launched) >= 12, sorted(launched)             # the scan still finds the launches
    assert launched == sup.launches(hpp) | sup.launches(sup.function_body(var, "int nt_launch_refine("))        # no launch of the header outside the launchers
    reached = {ac.route(case) for case in ac.CASES} | {ac.box_route(n) for n, _ in ac.BOX_CASES} | set(ac.FLAG_ROUTES)
    assert reached == launched, ("launched without a case: %s; routes nothing launches: %s"
                                 % (sorted(launched - reached), sorted(reached - launched)))
    for kernel in launched:
        assert kernel in ac.__doc__, kernel
    # the launches stay out of the render and ray launchers, and route on the switches read_switches already reads
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_var.hip", "int nt_launch_box("), ("nt_var.hip", "int nt_launch_rays(")):
        assert not any(k.startswith(("refine_", "adaptive_")) for k in sup.launches(sup.function_body(sup.source(src), head)))
    assert "getenv" not in hpp and "getenv" not in sup.function_body(var, "int nt_launch_refine(")
    api = sup.source("nt_api.cpp")
    assert "getenv" not in sup.function_body(api, "int enqueue_adaptive(")
