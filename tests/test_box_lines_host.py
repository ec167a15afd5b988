"""BoxScene face lines (BoxScene.set_face_lines, face_line_mask, nt_scene_set_box_lines, nt_box_line_mask*, and the renders that
honour the setting) without a GPU: that the expected masks of tests/box_hit_cases.py are the outline rule's with the crease test
always true, the setting's round trips and refusals, and what the mask forms and the renders refuse before they touch a device."""
import ctypes as C
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import box_hit_cases as bc
import ntracer_amd
import outline_cases as oc
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", bc.DIMS)
def test_the_expected_masks_are_the_outline_rule_with_the_crease_test_always_true(n):
    """outline_cases.mask_of fed with the normal rows s * e_i and crease_cos = 1.0 -- two different faces have c * c in {0, 1} --
    against the direct statement "different (item, lane) and not farther"; the two could differ only on a pair of opposite faces
    (c * c = 1), which no view of the cases has"""
    assert (bc.SILHOUETTE, bc.CREASE) == (oc.SILHOUETTE, oc.CREASE) == (_lib.NT_OUTLINE_SILHOUETTE, _lib.NT_OUTLINE_CREASE)
    marked = 0
    for _, k, (w, h) in bc.views(n):
        e = bc.expected(n, k, w, h)
        mask, counts = oc.mask_of(e["dist"], e["item"], e["lane"], bc.normals_of(n, e["item"], e["lane"]), 1.0, 0.0)
        assert np.array_equal(mask, e["mask"]), bc.view_id((n, k, (w, h)))
        assert (counts["silhouette"], counts["crease"], counts["depth"]) == (e["counts"]["silhouette"], e["counts"]["edge"], 0)
        assert not mask[e["item"] < 0].any() and not (mask & ~np.uint8(3)).any()
        # an edge is seen from both of its sides, one of which is the nearer: one-pixel lines
        assert e["counts"]["edge"] == e["counts"]["farther"] + e["counts"]["equal_dist"]
        marked += int((mask != 0).sum())
        if (w, h) == (1, 1):
            assert mask[0, 0] == 0
    assert marked > 300
    # each kind alone marks something, and differently
    e = bc.expected(n, 2, *bc.SIZES[-1])
    assert (e["mask"] & 1).any() and (e["mask"] & 2).any() and not np.array_equal(e["mask"] & 1, (e["mask"] & 2) >> 1)


def test_the_python_surface_and_the_abi_names():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_scene_set_box_lines", "nt_scene_get_box_lines", "nt_box_line_mask", "nt_box_line_mask_device"):
        assert hasattr(raw, name), name
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.BoxScene.set_face_lines).parameters.values())[1:]]
    assert params == [("color", (0, 0, 0)), ("strength", 1.0), ("silhouette", True), ("edges", True)]
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.BoxScene.face_line_mask).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", None)]
    assert isinstance(inspect.getattr_static(tracern.BoxScene, "face_lines"), property)
    assert inspect.getattr_static(tracern.BoxScene, "face_lines").fset is None
    for name in ("set_face_lines", "face_lines", "face_line_mask"):
        assert hasattr(ntracer_amd.NTracer(4).BoxScene, name) and not hasattr(tracern.CompositeScene, name)
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    sec = header[header.index("BoxScene hit buffers and face lines"):]
    for phrase in ("NT_OUTLINE_SILHOUETTE  if item(q) < 0;", "if item(q) == item(p) and lane(q) == lane(p);", "if dist(p) > dist(q)",
                   "NT_OUTLINE_CREASE      otherwise", "ANDed with `kinds`", "the nearer pixel carries the line",
                   "two different faces of a cube are\n   perpendicular or opposite", "(P.c * (1.0f - strength)) + (color.c * strength)",
                   "With strength = 0 the frame is the plain frame byte for byte, in every format", "lines never cross a frame boundary",
                   "The setting is not part of a pickled scene", "nt_scene_set_supersampling_scratch_mb"):
        assert phrase in sec, phrase
    for fn in ("nt_scene_set_box_lines", "nt_scene_get_box_lines", "nt_box_line_mask", "nt_box_line_mask_device"):
        assert re.search(r"\bint %s\(" % fn, sec), fn


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    box = tracern.BoxScene(5)
    assert box.face_lines is None
    box.set_face_lines()
    assert box.face_lines == dict(silhouette=True, edges=True, color=(0.0, 0.0, 0.0), strength=1.0)
    box.set_face_lines((1, 0.5, 0.25), 0.75, edges=False)
    assert box.face_lines == dict(silhouette=True, edges=False, color=(1.0, 0.5, 0.25), strength=0.75)
    box.set_face_lines(silhouette=False)
    assert box.face_lines == dict(silhouette=False, edges=True, color=(0.0, 0.0, 0.0), strength=1.0)
    # the ABI's getter through whichever pointers are given
    kinds, st, col = C.c_int(-1), C.c_float(-1), (C.c_float * 3)(-1, -1, -1)
    assert L.nt_scene_get_box_lines(box._handle, C.byref(kinds), None, C.byref(st)) == 0 and (kinds.value, st.value) == (2, 1.0)
    assert L.nt_scene_get_box_lines(box._handle, None, col, None) == 0 and list(col) == [0.0, 0.0, 0.0]
    assert L.nt_scene_get_box_lines(box._handle, None, None, None) == 0
    assert L.nt_scene_get_box_lines(None, C.byref(kinds), None, None) == _lib.NT_E_INVALID
    # every refusal leaves it as it was
    box.set_face_lines((0.25, 0.5, 1.0), 0.5)
    keep = box.face_lines
    black = (C.c_float * 3)(0, 0, 0)
    refused = [(k, black, 1.0) for k in (4, 5, 7, 8, -1)]                  # no depth bit for a convex body, nothing else either
    refused += [(3, black, v) for v in (-0.001, 1.001, np.nan, np.inf, -np.inf)]
    refused += [(3, None, 1.0)]
    for k in range(3):
        for v in (-0.001, 1.001, np.nan, np.inf):
            col = (C.c_float * 3)(0, 0, 0)
            col[k] = v
            refused.append((3, col, 1.0))
    for kinds, col, strength in refused:
        assert L.nt_scene_set_box_lines(box._handle, kinds, col, strength) == _lib.NT_E_INVALID, (kinds, strength)
        assert _lib.last_error()
        assert box.face_lines == keep
    assert L.nt_scene_set_box_lines(None, 3, black, 1.0) == _lib.NT_E_INVALID
    for bad in (dict(strength=True), dict(strength="1"), dict(color=(0, 0)), dict(color=(0, 0, 2)), dict(strength=1.5),
                dict(strength=float("nan")), dict(silhouette=False, edges=False)):
        with pytest.raises((ValueError, TypeError)):
            box.set_face_lines(**bad)
        assert box.face_lines == keep
    # the limits are in, each kind alone
    for kinds in (1, 2, 3):
        white = (C.c_float * 3)(1, 1, 1)
        assert L.nt_scene_set_box_lines(box._handle, kinds, white, 0.0) == 0
        assert box.face_lines == dict(silhouette=bool(kinds & 1), edges=bool(kinds & 2), color=(1.0, 1.0, 1.0), strength=0.0)
    # locked while a render holds the scene, as nt_scene_set_camera
    assert L.nt_scene_lock(box._handle) == 0
    keep = box.face_lines
    assert L.nt_scene_set_box_lines(box._handle, 3, black, 1.0) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_box_lines(box._handle, 0, None, 0.0) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        box.set_face_lines()
    assert box.face_lines == keep
    assert L.nt_scene_unlock(box._handle) == 0
    # off
    box.set_face_lines(None)
    assert box.face_lines is None
    assert L.nt_scene_get_box_lines(box._handle, C.byref(kinds := C.c_int(-1)), None, None) == 0 and kinds.value == 0
    # a view setting like fov, kept in the native handle: no part of what is pickled
    before = pickle.dumps({k: v for k, v in box.__dict__.items() if k != "_handle"}, 2)
    box.set_face_lines()
    assert pickle.dumps({k: v for k, v in box.__dict__.items() if k != "_handle"}, 2) == before
    assert not any("line" in k for k in box.__dict__)
    assert box.face_lines is not None and tracern.BoxScene(5).face_lines is None
    # a CompositeScene has outlines of its own
    g, n, flat = rq.scene("cell120_n4")
    comp = tracern.CompositeScene.from_flat(n, flat)
    assert L.nt_scene_set_box_lines(comp._handle, 3, black, 1.0) == _lib.NT_E_INVALID and "not a box scene" in _lib.last_error()
    assert L.nt_scene_set_box_lines(comp._handle, 0, None, 0.0) == _lib.NT_E_INVALID
    assert L.nt_scene_get_box_lines(comp._handle, C.byref(kinds), None, None) == _lib.NT_E_INVALID


def test_the_mask_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    box = tracern.BoxScene(4)
    g, n, flat = rq.scene("cell120_n4")
    comp = tracern.CompositeScene.from_flat(n, flat)
    comp.set_outlines()
    out = np.full(8 * 4, 77, np.uint8)
    host = lambda s, w, h, p: L.nt_box_line_mask(s, w, h, p, None, None)
    devf = lambda s, w, h, p: L.nt_box_line_mask_device(s, w, h, p, None, None)
    for call in (host, devf):
        # the setting is off
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "off" in _lib.last_error()
        box.set_face_lines()
        assert call(None, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert call(box._handle, 8, 4, None) == _lib.NT_E_INVALID
        for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
            assert call(box._handle, w, h, out.ctypes.data) == _lib.NT_E_INVALID, (w, h)
        assert call(comp._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "not a box scene" in _lib.last_error()
        box.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        box.set_lens(None)
        box.set_parallel_projection(2.0)
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        box.set_parallel_projection(None)
        box.set_face_lines(None)
    assert (out == 77).all()
    box.set_face_lines()
    # the options of the _device form: every field but device and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "strict_reference", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        assert L.nt_box_line_mask_device(box._handle, 8, 4, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the Python forms
    with pytest.raises(ValueError):
        box.face_line_mask(0, 4)
    box.set_face_lines(None)
    with pytest.raises(ValueError, match="off"):
        box.face_line_mask(8, 4)
    with pytest.raises(ValueError, match="off"):
        box.face_line_mask(8, 4, device="cuda")


def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device: NT_E_UNSUPPORTED with a message that starts "face lines", the
    destination as it was (the table form needs a device to make its table: test_box_lines_gpu.py)"""
    L = _lib.lib()
    n = 5
    box = tracern.BoxScene(n)
    box.set_face_lines()
    w, h = 8, 4
    fmt = sup.fmt_of(w, h)
    fst = fmt._as_struct()
    size = fmt.pitch * h
    dest = (C.c_char * size)(*([0x4E] * size))
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def forms(opts):
        po = None if opts is None else C.byref(opts)
        return [L.nt_render(box._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_device(box._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_frames_device(box._handle, dest, size, 1, origins.ctypes.data_as(_lib.f32p), axes.ctypes.data_as(_lib.f32p),
                                          C.byref(fst), po, None)]

    def refused(opts, word):
        for status in forms(opts):
            assert status == _lib.NT_E_UNSUPPORTED, (word, status, _lib.last_error())
            assert _lib.last_error().startswith("face lines") and word in _lib.last_error(), _lib.last_error()
        assert bytes(dest) == b"\x4e" * size

    # a supersampling factor, adaptive or not
    box.set_supersampling(2)
    refused(None, "supersampling")
    box.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    box.set_adaptive_supersampling(None)
    box.set_supersampling(1)
    # bands
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "band")
    # statistics
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    # a lens, the parallel projection
    box.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    box.set_lens(None)
    box.set_parallel_projection(2.0)
    refused(None, "parallel")
    box.set_parallel_projection(None)
    box.set_supersampling(3)
    with pytest.raises(NotImplementedError, match="face lines"):
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, box)
    assert not box.locked
    # each of them in the setting's own words, which tests/view_setting_refusals.py has byte for byte and
    # tests/test_view_setting_refusals.py holds every render form to; the sixth, the row range, is a guard for callers inside
    # nt_api.cpp, which the same test reads
    import view_setting_refusals as vr
    words = [m for (setting, _), m in vr.RENDER_REFUSALS.items() if setting == "face lines"]
    assert len(words) == 5 and all(m.startswith("face lines are not available") for m in words)
    # ... and every render entry point reaches them through render_checks, whose walk of the settings' table stands ahead of the
    # lens and the projection
    checks = sup.function_body(sup.source("nt_api.cpp"), "int render_checks(")
    assert checks.index("kViewSettings") < checks.index("whole_view_check(") < checks.index("lens_check(") < checks.index("parallel_check(")


@pytest.mark.skipif(_lib.lib().nt_device_count() > 0, reason="checks the no-GPU behaviour")
def test_without_a_gpu_the_mask_and_the_render_fail_loudly():
    box = tracern.BoxScene(4)
    box.set_face_lines()
    with pytest.raises(RuntimeError, match="no HIP device"):
        box.face_line_mask(8, 4)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ntracer_amd.BlockingRenderer().render(bytearray(8 * 4 * 4), sup.fmt_of(8, 4), box)
    assert not box.locked


def test_nothing_new_in_the_plain_routes_and_no_switch_of_its_own():
    # the plain BoxScene launchers launch what they launched: the face kernels have a dispatch of their own
    var = sup.source("nt_var.hip")
    for head in ("int nt_launch_box(", "int nt_launch_composite("):
        body = sup.function_body(var, head)
        assert "box_hits" not in body and "box_lines" not in body and "nt_box_faces" not in body, head
    assert "nt_boxhits" not in sup.source("nt_box.hpp") and "nt_boxhits" not in sup.source("nt_composite.hpp") and "nt_boxhits" not in sup.source("nt_inst_box.hip")
    # the routes obey NTRACER_FORCE_VAR and nothing of their own: no getenv in the kernels' files, the reader as it was
    for name in ("nt_boxhits.hpp", "nt_inst_boxhits.hip", "nt_var.hip"):
        assert "getenv" not in sup.source(name), name
    api = sup.source("nt_api.cpp")
    assert api.count("getenv(") == 12
    enq = sup.function_body(api, "int enqueue_box_lines(")
    assert "sw.force_var" in enq and "ss_scratch_mb" in enq and "nt_launch_box_faces(" in enq
