"""X-ray views, the part that needs no GPU: the numpy restatement of the rule (tests/xray_cases.py) pinned to the oracle, the
conditions that keep tests/test_xray_gpu.py from being vacuous, the live masks of a padded batch, the ABI and the setter, and
every answer the entry points give before a device is touched -- the messages written down here as literals."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import fixtures as fx
import ray_query_cases as rq
import primary_hit_cases as ph
import xray_cases as xc
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)

RENDER_REFUSALS = {
    "supersampling": "X-ray is not available with a supersampling factor above 1 (2)",
    "bands": "X-ray is not available with row bands (band_world 2)",
    "collect_stats": "X-ray is not available with collect_stats",
    "lens": "X-ray is not available while a lens is set",
    "parallel": "X-ray is not available while the parallel projection is set",
    "clip": "X-ray is not available while clip planes are set",
    "cue": "X-ray is not available while depth cues are on",
    "outlines": "X-ray is not available while outlines are on",
    "ao": "X-ray is not available while ambient occlusion is on",
    "stack": "X-ray is not available while a view stack is set",
}
COUNT_REFUSALS = {
    "null": "NULL argument",
    "size": "invalid view size",
    "box": "not a composite scene",
    "clip": "clip planes are set: the crossing count is not available under them",
    "projection": "the crossing counts are not available while a lens or the parallel projection is set",
    "pixels": "a view of 65536 x 65536 pixels is beyond 2^31 - 1 pixels",
    "options": "the crossing counts read device, strict_reference and abort_device of their options: every other field must be 0",
}
ABSORBANCE = "the X-ray's absorbance must lie in [0, 1]"
TINT = "the X-ray's tint must lie in [0, 1]"
UNDER_XRAY = {
    "nt_colors_at": "X-ray is on: the colour of single pixels (nt_colors_at / nt_calculate_color) is not available under it",
    "nt_outline_mask": "X-ray is on: the outline mask is not available under it",
    "nt_ambient_occlusion": "X-ray is on: the ambient occlusion count is not available under it",
    "nt_depth_cue_factors": "X-ray is on: the depth cue factors is not available under it",
    "nt_adaptive_mask": "X-ray is on: the adaptive mask is not available under it",
}


def _scene(name="cell120_n4"):
    n, flat, params, fov, cam = xc.scene(name)
    sc = tracern.CompositeScene.from_flat(n, flat)
    return sc, n, flat


# ------------------------------------------------------------------ the restatement, and the conditions on the inputs
@pytest.mark.parametrize("name", ["cell120_n4", "cell600_n4", "simplex10_n10"])
def test_the_nearest_crossing_is_the_oracles_hit_bit_for_bit(name):
    g, n, _ = rq.scene(name)
    flat = fx.flat_of(g, opaque=True)
    w, h = 37, 21
    r = xc.reference(name, w, h)
    o, _ = ph.camera(name, 0)
    D = r["D"]
    lo, hi = np.asarray(flat["aabb_start"], np.float32), np.asarray(flat["aabb_end"], np.float32)
    t0 = ph.aabb_distance(lo, hi, o, D)
    enter = np.nonzero(t0 >= 0)[0]
    assert np.array_equal(t0 >= 0, r["enter"]) and len(enter) > 100
    want = np.full(w * h, xc.FLT_MAX, np.float32)
    none = np.full(len(enter), -1, np.int32)
    got = rq.Oracle(n, flat, True, False).intersects(np.repeat(o[None], len(enter), axis=0), D[enter], t0[enter],
                                                     np.full(len(enter), xc.FLT_MAX), none, none)
    want[enter] = got["dist"]
    assert (want < xc.FLT_MAX).sum() >= 10                       # (the 10-D simplex is small in its golden view: 16 pixels)
    assert np.array_equal(bits(r["nearest"]), bits(want)), int((bits(r["nearest"]) != bits(want)).sum())
    if name == "simplex10_n10":
        assert len(np.asarray(flat["tri_recs"]).reshape(-1)) > 0          # unbatched triangles: the scalar rule is pinned too


@pytest.mark.parametrize("name", ["cell120_n4", "cell600_n4"])
def test_every_count_of_a_closed_shell_is_even(name):
    c = xc.reference(name, 37, 21)["count"]
    assert c.max() > 0 and not (c % 2).any()


def test_the_120_cell_crosses_more_than_the_transparent_cap_keeps():
    c = xc.reference("cell120_n4", 37, 21)["count"]
    assert c.max() >= 25
    # (measured: 138 at the most, 78 pixels above 24, a mean of 9.5)
    assert (int(c.max()), int((c > 24).sum())) == (138, 78) and abs(c.mean() - 9.5) < 0.05


@pytest.mark.parametrize("name,w,h", xc.ALL_VIEWS, ids=lambda v: str(v))
def test_at_most_one_ray_in_a_hundred_is_fuzzed_or_unsafe(name, w, h):
    r = xc.reference(name, w, h)
    assert (~r["ordinary"]).sum() <= 0.01 * w * h, (int(r["fuzzed"].sum()), int(r["unsafe"].sum()))
    if w * h > 64:
        assert r["count"].max() > 0                                      # the view sees the scene


def test_the_general_cases_are_of_the_general_route_and_the_packet_cases_of_the_packet():
    for name, _ in xc.PACKET:
        n, flat, _, _, _ = xc.scene(name)
        items = len(np.asarray(flat["batch_mats"]).reshape(-1)) // 4 + len(np.asarray(flat["tri_mats"]).reshape(-1)) + len(np.asarray(flat["solid_types"]).reshape(-1))
        assert n <= 10 and items <= 65536
    for name, _ in xc.GENERAL:
        assert xc.scene(name)[0] > 10
    n, flat, _, _, _ = xc.scene("cell600_n4")
    assert len(np.asarray(flat["batch_mats"]).reshape(-1)) // 4 == 150       # a bitset with a partial last word
    n, flat, _, _, _ = xc.scene("simplex10_n10")
    assert len(np.asarray(flat["tri_mats"]).reshape(-1)) > 0
    n, flat, _, _, _ = xc.scene("feature5_n5")
    assert len(np.asarray(flat["solid_types"]).reshape(-1)) > 0 and (np.asarray(flat["materials"]).reshape(-1, 10)[:, 6] < 1).any()


def test_the_padded_batch_of_a_built_simplex_counts_five_facets():
    n, flat, _, _, cam = xc.scene(xc.BUILT)
    live = xc.live_masks(flat, n)
    assert len(live) == 2 and sum(bin(int(m)).count("1") for m in live) == 5
    sc = tracern.CompositeScene.from_flat(n, flat)
    L = _lib.lib()
    got = np.zeros(len(live), np.uint8)
    assert L.nt_scene_batch_live_masks(sc._handle, got.ctypes.data) == len(live)
    assert L.nt_scene_batch_live_masks(sc._handle, None) == len(live)
    assert np.array_equal(got, live)
    assert L.nt_scene_batch_live_masks(tracern.BoxScene(4)._handle, None) == _lib.NT_E_INVALID
    r = xc.reference(xc.BUILT, 17, 17)
    assert r["count"].max() == 2 and not (r["count"] % 2).any()
    # without the mask the repeated facet counts again: the mask is what keeps the counts even
    o, _ = cam(0)
    c = xc.crossings32(flat, o, r["D"], live=np.full(len(live), 15, np.uint8))["count"]
    assert (c % 2).any() and c.max() > 2


# ------------------------------------------------------------------ the ABI and the setter
def test_the_exported_symbols_and_the_python_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_scene_set_xray", "nt_scene_get_xray", "nt_scene_batch_live_masks", "nt_crossing_counts", "nt_crossing_counts_device"):
        assert hasattr(raw, name), name
    L = _lib.lib()
    assert L.nt_scene_set_xray.argtypes == [C.c_void_p, C.c_int, C.c_float, C.c_float]
    assert L.nt_scene_get_xray.argtypes == [C.c_void_p, C.POINTER(C.c_int), _lib.f32p, _lib.f32p, _lib.f32p]
    assert L.nt_crossing_counts.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(_lib.NtRenderOpts)]
    assert L.nt_crossing_counts_device.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(_lib.NtRenderOpts), C.c_void_p]
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    for decl in ("int nt_scene_set_xray(nt_scene_t *s, int enabled, float absorbance, float tint);",
                 "int nt_scene_get_xray(const nt_scene_t *s, int *enabled, float *absorbance, float *tint, float *table);",
                 "int nt_crossing_counts(nt_scene_t *s, int width, int height, int32_t *counts, const nt_render_opts *opts);",
                 "int nt_crossing_counts_device(nt_scene_t *s, int width, int height, void *counts_dev, const nt_render_opts *opts, void *hip_stream);"):
        assert decl in header, decl
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.set_xray).parameters.values())[1:]]
    assert params == [("absorbance", 0.2), ("tint", 1.0)]
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.crossing_counts).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", None)]
    assert isinstance(inspect.getattr_static(tracern.CompositeScene, "xray"), property)
    assert inspect.getattr_static(tracern.CompositeScene, "xray").fset is None


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    sc, n, flat = _scene("feature5_n5")
    assert sc.xray is None
    sc.set_xray()
    x = sc.xray
    assert (x["absorbance"], x["tint"]) == (float(np.float32(0.2)), 1.0)
    # the table the library uploads is the numpy one, bit for bit
    for a, t in ((0.2, 1.0), (0.3, 0.0), (0.3, 1.0), (1.0, 1.0), (0.0, 0.5), (0.7, 0.35)):
        sc.set_xray(a, t)
        want = xc.transmittance(flat, a, t)
        assert want.shape[0] > 1 and np.array_equal(bits(sc.xray["transmittance"]), bits(want)), (a, t)
    assert np.array_equal(xc.transmittance(flat, 0.3, 0.0), np.full((len(want), 3), np.float32(1.0) - np.float32(0.3), np.float32))
    # the getter through whichever pointers are given
    on, ab = C.c_int(-1), C.c_float(-1)
    assert L.nt_scene_get_xray(sc._handle, C.byref(on), C.byref(ab), None, None) == 0 and (on.value, ab.value) == (1, float(np.float32(0.7)))
    assert L.nt_scene_get_xray(sc._handle, None, None, None, None) == 0
    assert L.nt_scene_get_xray(None, C.byref(on), None, None, None) == _lib.NT_E_INVALID
    # every refusal answers NT_E_INVALID word for word and leaves the setting as it was
    keep = sc.xray
    for a, t, words in [(v, 0.5, ABSORBANCE) for v in (-0.001, 1.001, np.nan, np.inf, -np.inf)] + \
                       [(0.5, v, TINT) for v in (-0.001, 1.001, np.nan, np.inf, -np.inf)]:
        assert L.nt_scene_set_xray(sc._handle, 1, a, t) == _lib.NT_E_INVALID, (a, t)
        assert _lib.last_error() == words
        now = sc.xray
        assert (now["absorbance"], now["tint"]) == (keep["absorbance"], keep["tint"]) and np.array_equal(now["transmittance"], keep["transmittance"])
    assert L.nt_scene_set_xray(None, 1, 0.5, 0.5) == _lib.NT_E_INVALID
    for bad in (dict(absorbance=True), dict(absorbance="0.2"), dict(tint=None), dict(absorbance=1.5), dict(tint=-0.5), dict(tint=float("nan"))):
        with pytest.raises((ValueError, TypeError)):
            sc.set_xray(**bad)
    # locked while a render holds the scene, as the other setters
    assert L.nt_scene_lock(sc._handle) == 0
    assert L.nt_scene_set_xray(sc._handle, 1, 0.5, 0.5) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_xray(sc._handle, 0, 0.0, 0.0) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        sc.set_xray()
    assert L.nt_scene_unlock(sc._handle) == 0
    assert sc.xray["absorbance"] == keep["absorbance"]
    sc.set_xray(None)
    assert sc.xray is None
    assert L.nt_scene_get_xray(sc._handle, C.byref(on), None, None, None) == 0 and on.value == 0
    # CompositeScene only
    box = tracern.BoxScene(4)
    assert L.nt_scene_set_xray(box._handle, 1, 0.5, 0.5) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_xray()
    assert box.xray is None


# ------------------------------------------------------------------ refusals, before a device is touched
def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    L = _lib.lib()
    sc, n, _ = _scene()
    sc.set_xray()
    w, h = 8, 4
    fmt = sup.fmt_of(w, h)
    fst = fmt._as_struct()
    size = fmt.pitch * h
    dest = (C.c_char * size)(*([0x4E] * size))
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def refused(opts, key):
        po = None if opts is None else C.byref(opts)
        for status in (L.nt_render(sc._handle, dest, size, C.byref(fst), po, None),
                       L.nt_render_device(sc._handle, dest, size, C.byref(fst), po, None),
                       L.nt_render_frames_device(sc._handle, dest, size, 1, origins.ctypes.data_as(_lib.f32p), axes.ctypes.data_as(_lib.f32p),
                                                 C.byref(fst), po, None)):
            assert status == _lib.NT_E_UNSUPPORTED, (key, status, _lib.last_error())
            assert _lib.last_error() == RENDER_REFUSALS[key]
        assert bytes(dest) == b"\x4e" * size

    sc.set_supersampling(2)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(None)
    sc.set_supersampling(1)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "bands")
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    sc.set_lens(None)
    sc.set_parallel_projection(2.0)
    refused(None, "parallel")
    sc.set_parallel_projection(None)
    sc.set_clip_planes([((1,) + (0,) * (n - 1), 0.5)])
    refused(None, "clip")
    sc.set_clip_planes(None)
    sc.set_depth_cue()
    refused(None, "cue")
    sc.set_depth_cue(None)
    sc.set_outlines()
    refused(None, "outlines")
    sc.set_outlines(None)
    sc.set_ambient_occlusion(4, 1.0)
    refused(None, "ao")
    sc.set_ambient_occlusion(None)
    sc.set_view_stack(np.zeros((1, n), np.float32))
    refused(None, "stack")
    sc.set_view_stack(None)
    assert len(RENDER_REFUSALS) == 10
    # what does not honour the setting is refused while it is on, as under clip planes
    xs = np.zeros(1, np.int32)
    rgb = np.full(3, 7, np.float32)
    assert L.nt_colors_at(sc._handle, w, h, 1, xs.ctypes.data_as(_lib.i32p), xs.ctypes.data_as(_lib.i32p), rgb.ctypes.data_as(_lib.f32p), -1) == _lib.NT_E_UNSUPPORTED
    assert _lib.last_error() == UNDER_XRAY["nt_colors_at"] and (rgb == 7).all()
    out = np.full(w * h * 8, 77, np.uint8)
    for entry, counted in (("nt_outline_mask", True), ("nt_adaptive_mask", True), ("nt_ambient_occlusion", False), ("nt_depth_cue_factors", False)):
        args = (sc._handle, w, h, out.ctypes.data) + ((None,) if counted else ()) + (None,)
        assert getattr(L, entry)(*args) == _lib.NT_E_UNSUPPORTED, entry
        assert _lib.last_error() == UNDER_XRAY[entry]
        assert getattr(L, entry + "_device")(sc._handle, w, h, out.ctypes.data, None, None) == _lib.NT_E_UNSUPPORTED, entry
    assert (out == 77).all()
    # off again: nothing of the setting is left in a refusal
    sc.set_xray(None)
    sc.set_supersampling(2)
    sc.set_outlines()
    assert L.nt_render(sc._handle, dest, size, C.byref(fst), None, None) == _lib.NT_E_UNSUPPORTED and _lib.last_error().startswith("outlines")


def test_the_count_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    sc, n, _ = _scene()
    box = tracern.BoxScene(4)
    out = np.full(8 * 4, 77, np.int32)
    host = lambda s, w, h, p, o=None: L.nt_crossing_counts(s, w, h, p, o)
    devf = lambda s, w, h, p, o=None: L.nt_crossing_counts_device(s, w, h, p, o, None)

    def refused(status, code, key):
        assert status == code, (key, status, _lib.last_error())
        assert _lib.last_error() == COUNT_REFUSALS[key]

    for on in (False, True):                 # whether or not the setting is on
        if on:
            sc.set_xray()
        for call in (host, devf):
            refused(call(None, 8, 4, out.ctypes.data), _lib.NT_E_INVALID, "null")
            refused(call(sc._handle, 8, 4, None), _lib.NT_E_INVALID, "null")
            for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
                refused(call(sc._handle, w, h, out.ctypes.data), _lib.NT_E_INVALID, "size")
            refused(call(box._handle, 8, 4, out.ctypes.data), _lib.NT_E_INVALID, "box")
            refused(call(sc._handle, 65536, 65536, out.ctypes.data), _lib.NT_E_INVALID, "pixels")
            sc.set_clip_planes([((1,) + (0,) * (n - 1), 0.5)])
            refused(call(sc._handle, 8, 4, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "clip")
            sc.set_clip_planes(None)
            sc.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
            refused(call(sc._handle, 8, 4, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "projection")
            sc.set_lens(None)
            sc.set_parallel_projection(2.0)
            refused(call(sc._handle, 8, 4, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "projection")
            sc.set_parallel_projection(None)
        for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
            opts = _lib.NtRenderOpts()
            opts.device = -1
            setattr(opts, field, 1)
            refused(devf(sc._handle, 8, 4, out.ctypes.data, C.byref(opts)), _lib.NT_E_INVALID, "options")
    assert (out == 77).all()
    with pytest.raises(ValueError):
        sc.crossing_counts(0, 4)
    with pytest.raises(ValueError, match="not a composite scene"):
        box.crossing_counts(8, 4)
