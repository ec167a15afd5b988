"""Outlines, the part that needs no GPU: the conditions that keep tests/test_outlines_gpu.py from being vacuous, asserted on the
oracle's masks (tests/outline_cases.py); every answer the ABI gives before a device is touched; the setting's round trip; the
exported symbols and the Python signatures; and the kernel routes, pinned to the C++ that picks them the way
tests/test_ao_host.py pins AO_ROUTES: every hipLaunchKernelGGL of launch_outline_fixed (nt_outline.hpp) and of
nt_launch_outline_mark and nt_launch_outline_apply (nt_var.hip) has a row in OUTLINE_ROUTES, and every row names cases that
tests/test_outlines_gpu.py runs."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import outline_cases as oc
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = [("cell120_n4", {}), ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}), ("cell600_n4", {}), ("orthoplex5_n5", {})]
SCALAR = [("simplex10_n10", {})]
GENERAL = [("cell120_n4", {"NTRACER_FORCE_VAR": "1"}), ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
           ("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}), ("feature5_n5", {}), ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
           ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}), ("feature11_n11", {}), ("feature16_n16", {})]
# kernel instantiation as its hipLaunchKernelGGL spells it (spaces dropped) -> what launches it in test_outlines_gpu.py: (scene,
# switches) cases of outline_cases.CASES for the mask kernels and the walk, (scene, variant) entries of outline_cases.RENDERED
# for the kernels only a render launches
OUTLINE_ROUTES = [
    ("packet_numerators<N>", PLAIN + SCALAR),
    ("composite_packet<N,32,false,false,true>", PLAIN),
    ("composite_packet<N,32,false,true,true>", SCALAR),
    ("outline_mark_fixed<N,false>", PLAIN),
    ("outline_mark_fixed<N,true>", SCALAR),
    ("outline_shade<N,false,false>", [("cell120_n4", "")]),
    ("outline_shade<N,true,false>", [("cell600_n4", "lit")]),
    ("outline_shade<N,true,true>", [("simplex10_n10", "")]),
    ("outline_mark", GENERAL),
    ("outline_apply", [("feature5_n5", "")]),
]
RENDER_ROWS = ("outline_shade<N,false,false>", "outline_shade<N,true,false>", "outline_shade<N,true,true>", "outline_apply")


def _traits(n, flat, params, env):
    m = np.asarray(flat["materials"]).reshape(-1, 10)
    opaque, reflective = bool((m[:, 6] >= 1).all()), bool((m[:, 7] > 0).any())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    faithful = not opaque or (solids and env.get("NTRACER_CLEAN_NORMALS") != "1")
    packet = not faithful and not var and env.get("NTRACER_COMPOSITE_KERNEL", "0") == "0"
    lights = np.asarray(params["point_light_color"]).size + np.asarray(params["global_light_color"]).size > 0
    return packet, scalar, (lights or reflective or scalar)


def _mask_routes(name, env):
    """the kernels nt_outline_mask launches for a (scene, switches) case, by the rule of enqueue_outlines (nt_api.cpp) and
    launch_outline_fixed (the golden trees are shallower than the packet walk's stack)"""
    g, n, flat = rq.scene(name)
    packet, scalar, _ = _traits(n, flat, fx.params_of(g), env)
    if not packet:
        return {"outline_mark"}
    s = "true" if scalar else "false"
    return {"packet_numerators<N>", "composite_packet<N,32,false,%s,true>" % s, "outline_mark_fixed<N,%s>" % s}


def _render_route(name, variant):
    """the kernel that draws a render of outline_cases.RENDERED"""
    n, flat, params = rc.case_scene((name, {}, variant))
    packet, scalar, feat = _traits(n, flat, params, {})
    if not packet:
        return "outline_apply"
    return "outline_shade<N,%s,%s>" % ("true" if feat else "false", "true" if scalar else "false")


def test_every_outline_launch_has_a_row_and_every_row_a_gpu_case():
    var = sup.source("nt_var.hip")
    launched = sup.launches_through(sup.source("nt_outline.hpp"), "int launch_outline_fixed(")
    assert len(launched) == 8
    for head in ("int nt_launch_outline(", "int nt_launch_outline_mask(", "static int nt_launch_outline_fixed(", "int nt_launch_outline_mark(",
                 "int nt_launch_outline_apply("):
        launched |= sup.launches(sup.function_body(var, head))
    rows = [k for k, _ in OUTLINE_ROUTES]
    assert len(rows) == len(set(rows)) == 10
    assert set(rows) == launched, (sorted(launched - set(rows)), sorted(set(rows) - launched))
    cases = [(name, tuple(sorted(env.items()))) for name, env in oc.CASES]
    for kernel, ways in OUTLINE_ROUTES:
        assert ways, kernel
        for way in ways:
            if kernel in RENDER_ROWS:
                assert way in oc.RENDERED, (kernel, way)
                assert _render_route(*way) == kernel, (kernel, way, _render_route(*way))
            else:
                name, env = way
                assert (name, tuple(sorted(env.items()))) in cases, (kernel, name, env)
                assert kernel in _mask_routes(name, env), (kernel, name, env, _mask_routes(name, env))
    # every case and every rendered scene lands on rows of the table
    for name, env in oc.CASES:
        assert _mask_routes(name, env) <= set(rows), (name, env)
    assert {_render_route(*r) for r in oc.RENDERED} == set(RENDER_ROWS)
    # the rule above is enqueue_outlines' own: composite_route's answer, no term of its own, no getenv of its own
    api = sup.source("nt_api.cpp")
    rule, enq = sup.function_body(api, "CompositeRoute composite_route("), sup.function_body(api, "int enqueue_outlines(")
    assert "r.packet_walk = !r.faithful && !r.var && sw.composite_kernel == 0 && std::max(s->depth + 1, 2) <= 32;" in rule
    assert "const bool fast = composite_route(s, sw).packet_walk;" in enq and "all_opaque" not in enq and "getenv" not in enq
    for name in ("nt_outline.hpp", "nt_inst_outline.hip"):
        assert "getenv" not in sup.source(name)
    # the outline dispatch stands in front of the ambient-occlusion one, and the check in front of ambient occlusion's
    body = sup.function_body(api, "int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in) {")
    assert 0 < body.index("return enqueue_outlines(") < body.index("return enqueue_ao(")
    # (render_checks walks the table of the settings, outlines above ambient occlusion: of the two the outlines refuse, as
    # tests/test_view_setting_refusals.py finds of the library)
    import view_setting_refusals as vr
    assert vr.RENDER_REFUSALS["outlines", "ao"] == "outlines are not available while ambient occlusion is on"
    assert ("ao", "outlines") not in vr.RENDER_REFUSALS and "kViewSettings" in sup.function_body(api, "int render_checks(")
    # the pair rule is written once
    assert len(re.findall(r"int outline_pair\(", sup.source("nt_outline.hpp"))) == 1 and "outline_pair(" in var
    assert "NT_DEV_OUTLINE_CREASE" not in var and "c * c <" not in sup.function_body(var, "void outline_mark(")
    # the new launches stay out of the render, query, hits, lens and ambient-occlusion launchers
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_query.hpp", "int launch_query_fixed("), ("nt_var.hip", "int nt_launch_query("),
                      ("nt_hits.hpp", "int launch_hits_fixed("), ("nt_var.hip", "int nt_launch_hits("),
                      ("nt_lens.hpp", "int launch_lens_fixed("), ("nt_ao.hpp", "int launch_ao_fixed("), ("nt_var.hip", "int nt_launch_ao(")):
        assert not any(k.startswith("outline_") for k in sup.launches(sup.function_body(sup.source(src), head))), head


# ------------------------------------------------------------------ the conditions that keep the GPU tests from being vacuous
def test_the_oracles_masks_are_not_vacuous():
    mask, c = oc.expected(oc.CASES[0], *oc.BIG, params=oc.A)
    assert (c["silhouette"], c["crease"], c["depth"]) == (272, 627, 406)
    assert (c["unmarked"], c["farther"]) == (199, 861)
    for bit in (oc.SILHOUETTE, oc.CREASE, oc.DEPTH):
        assert ((mask & bit) != 0).sum() > 100
    assert set(np.unique(mask)) <= set(range(8)) and len(np.unique(mask)) >= 5
    _, c = oc.expected(("cell600_n4", {}), 37, 21, params=oc.A)
    assert c["equal_dist"] == 16
    mask, c = oc.expected(("cell600_n4", {}), *oc.BIG, params=oc.B)
    assert (c["crease"], c["unmarked"], c["depth"]) == (5, 600, 0)
    assert not (mask & oc.DEPTH).any()
    # the golden scenes with Solids have normals that are not of unit length: the la * lb term is exercised
    for name in ("feature5_n5", "feature16_n16"):
        _, c = oc.expected((name, {}), 37, 21, params=oc.A)
        assert c["crease"] + c["unmarked"] > 0 and any(l in (0.8, 0.9) for l in c["lengths"]), (name, c)


@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_no_tested_pair_lies_at_the_crease_threshold(case):
    """fp32 against fp32 of the same operations needs no margin; this keeps the cases away from where a reordered sum would show"""
    marked = 0
    for w, h in oc.sizes(case):
        for label, params in oc.PARAMS:
            mask, c = oc.expected(case, w, h, params=params)
            assert c["margin"] >= 1e-2, (oc.case_id(case), w, h, label, c["margin"])
            marked += int((mask != 0).sum())
            if (w, h) == (1, 1):
                assert not mask.any()
    assert marked > 0


def test_a_mask_never_reads_across_a_row_or_an_image_edge():
    """mask_of on records made by hand: a hit pixel alone in the image, in a corner, and beside the wrapped end of the row above"""
    item = np.full((3, 4), -1, np.int32)
    lane = np.zeros((3, 4), np.int32)
    dist = np.full((3, 4), 1.0, np.float32)
    normal = np.zeros((3, 4, 3), np.float32)
    normal[..., 0] = 1.0
    item[:] = 8
    mask, c = oc.mask_of(dist, item, lane, normal, *oc.A)
    assert not mask.any() and c["same"] == 2 * (3 * 3 + 2 * 4)
    item[1, 0] = -1                                          # (x = 0 of row 1 follows x = 3 of row 0 in memory)
    mask, _ = oc.mask_of(dist, item, lane, normal, *oc.A)
    want = np.zeros((3, 4), np.uint8)
    want[0, 0] = want[2, 0] = want[1, 1] = oc.SILHOUETTE
    assert np.array_equal(mask, want)


# ------------------------------------------------------------------ the ABI and the Python surface
def test_the_exported_symbols_and_the_python_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_scene_set_outlines", "nt_scene_get_outlines", "nt_outline_mask", "nt_outline_mask_device"):
        assert hasattr(raw, name), name
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    for name, value in (("NT_OUTLINE_SILHOUETTE", 1), ("NT_OUTLINE_CREASE", 2), ("NT_OUTLINE_DEPTH", 4)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
        assert getattr(ntracer_amd, name) == getattr(tracern, name) == getattr(_lib, name) == value and name in ntracer_amd.__all__
    assert (oc.SILHOUETTE, oc.CREASE, oc.DEPTH) == (1, 2, 4)
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.set_outlines).parameters.values())[1:]]
    assert params == [("crease_angle", 0.1), ("depth_gap", 0.02), ("color", (0, 0, 0)), ("strength", 1.0)]
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.outline_mask).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", None), ("strict_reference", None)]
    assert isinstance(inspect.getattr_static(tracern.CompositeScene, "outlines"), property)
    assert inspect.getattr_static(tracern.CompositeScene, "outlines").fset is None


def _scene(name="cell120_n4"):
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat), n


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    sc, n = _scene()
    assert sc.outlines is None
    sc.set_outlines()
    assert sc.outlines == dict(crease_cos=float(np.float32(math.cos(0.1))), depth_gap=float(np.float32(0.02)), color=(0.0, 0.0, 0.0), strength=1.0)
    sc.set_outlines(0.25, depth_gap=0.0, color=(1, 0.5, 0.25), strength=0.75)
    assert sc.outlines == dict(crease_cos=float(np.float32(math.cos(0.25))), depth_gap=0.0, color=(1.0, 0.5, 0.25), strength=0.75)
    sc.set_outlines(oc.crease_angle(0.995))
    assert sc.outlines["crease_cos"] == float(np.float32(0.995))
    # the ABI's getter through whichever pointers are given
    on, gap, col = C.c_int(-1), C.c_float(-1), (C.c_float * 3)(-1, -1, -1)
    assert L.nt_scene_get_outlines(sc._handle, C.byref(on), None, C.byref(gap), None, None) == 0
    assert (on.value, gap.value) == (1, float(np.float32(0.02)))
    assert L.nt_scene_get_outlines(sc._handle, None, None, None, col, None) == 0 and list(col) == [0.0, 0.0, 0.0]
    assert L.nt_scene_get_outlines(sc._handle, None, None, None, None, None) == 0
    assert L.nt_scene_get_outlines(None, C.byref(on), None, None, None, None) == _lib.NT_E_INVALID
    # every refusal leaves it as it was
    sc.set_outlines(0.3, 0.125, (0.25, 0.5, 1.0), 0.5)
    keep = sc.outlines
    black = (C.c_float * 3)(0, 0, 0)
    refused = [(v, 0.02, black, 1.0) for v in (-0.001, 1.001, np.nan, np.inf, -np.inf)]
    refused += [(0.9, v, black, 1.0) for v in (-1e-9, np.nan, np.inf)]
    refused += [(0.9, 0.02, black, v) for v in (-0.001, 1.001, np.nan, np.inf)]
    refused += [(0.9, 0.02, None, 1.0)]
    for k in range(3):
        for v in (-0.001, 1.001, np.nan, np.inf):
            col = (C.c_float * 3)(0, 0, 0)
            col[k] = v
            refused.append((0.9, 0.02, col, 1.0))
    for cc, gap, col, strength in refused:
        assert L.nt_scene_set_outlines(sc._handle, 1, cc, gap, col, strength) == _lib.NT_E_INVALID, (cc, gap, strength)
        assert _lib.last_error()
        assert sc.outlines == keep
    assert L.nt_scene_set_outlines(None, 1, 0.9, 0.02, black, 1.0) == _lib.NT_E_INVALID
    for bad in (dict(crease_angle=True), dict(crease_angle="0.1"), dict(depth_gap=None), dict(strength="1"), dict(color=(0, 0)),
                dict(color=(0, 0, 2)), dict(crease_angle=2.0), dict(crease_angle=float("nan")), dict(crease_angle=-0.1),
                dict(crease_angle=2 * math.pi - 0.1), dict(crease_angle=float("inf")), dict(depth_gap=-1.0), dict(strength=1.5)):
        with pytest.raises((ValueError, TypeError)):
            sc.set_outlines(**bad)
        assert sc.outlines == keep
    # the limits are in
    sc.set_outlines(0.0, 0.0, (1, 1, 1), 0.0)
    assert sc.outlines == dict(crease_cos=1.0, depth_gap=0.0, color=(1.0, 1.0, 1.0), strength=0.0)
    sc.set_outlines(math.pi / 2, 1e30, (0, 0, 0), 1.0)
    assert 0.0 <= sc.outlines["crease_cos"] < 1e-7
    # locked while a render holds the scene, as nt_scene_set_camera
    assert L.nt_scene_lock(sc._handle) == 0
    keep = sc.outlines
    assert L.nt_scene_set_outlines(sc._handle, 1, 0.9, 0.02, black, 1.0) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_outlines(sc._handle, 0, 0.0, 0.0, None, 0.0) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        sc.set_outlines()
    assert sc.outlines == keep
    assert L.nt_scene_unlock(sc._handle) == 0
    # off
    sc.set_outlines(None)
    assert sc.outlines is None
    assert L.nt_scene_get_outlines(sc._handle, C.byref(on), None, None, None, None) == 0 and on.value == 0
    # a view setting like fov, kept in the native handle: no part of what is pickled, and -- as ambient occlusion -- not carried
    # over by with_rebuilt_tree or to another scene made from the same description
    sc.set_outlines(None)
    import pickle
    before = pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2)
    sc.set_outlines()
    sc.set_ambient_occlusion(4, 1.0)
    assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before
    assert not any("outline" in k for k in sc.__dict__)
    other = sc.with_rebuilt_tree()
    assert other.outlines is None and other.ambient_occlusion is None
    assert sc.outlines is not None and sc.ambient_occlusion is not None
    assert _scene()[0].outlines is None
    # a BoxScene has no records
    box = tracern.BoxScene(4)
    assert L.nt_scene_set_outlines(box._handle, 1, 0.9, 0.02, black, 1.0) == _lib.NT_E_INVALID
    assert L.nt_scene_set_outlines(box._handle, 0, 0.0, 0.0, None, 0.0) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_outlines()
    assert box.outlines is None


def test_the_mask_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    sc, n = _scene()
    box = tracern.BoxScene(4)
    out = np.full(8 * 4, 77, np.uint8)
    host = lambda s, w, h, p: L.nt_outline_mask(s, w, h, p, None, None)
    devf = lambda s, w, h, p: L.nt_outline_mask_device(s, w, h, p, None, None)
    for call in (host, devf):
        # the setting is off
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "off" in _lib.last_error()
        sc.set_outlines()
        assert call(None, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert call(sc._handle, 8, 4, None) == _lib.NT_E_INVALID
        for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
            assert call(sc._handle, w, h, out.ctypes.data) == _lib.NT_E_INVALID, (w, h)
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "not a composite scene" in _lib.last_error()
        sc.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        sc.set_lens(None)
        sc.set_parallel_projection(2.0)
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        sc.set_parallel_projection(None)
        sc.set_outlines(None)
    assert (out == 77).all()
    sc.set_outlines()
    # the options of the _device form: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        assert L.nt_outline_mask_device(sc._handle, 8, 4, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the Python forms
    with pytest.raises(ValueError):
        sc.outline_mask(0, 4)
    with pytest.raises(ValueError, match="not a composite scene"):
        box.outline_mask(8, 4)
    sc.set_outlines(None)
    with pytest.raises(ValueError, match="off"):
        sc.outline_mask(8, 4)


def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device: NT_E_UNSUPPORTED with a message that starts "outlines", the
    destination as it was (the table form needs a device to make its table: test_outlines_gpu.py)"""
    L = _lib.lib()
    sc, n = _scene()
    sc.set_outlines()
    w, h = 8, 4
    fmt = sup.fmt_of(w, h)
    fst = fmt._as_struct()
    size = fmt.pitch * h
    dest = (C.c_char * size)(*([0x4E] * size))
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def forms(opts):
        po = None if opts is None else C.byref(opts)
        return [L.nt_render(sc._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_device(sc._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_frames_device(sc._handle, dest, size, 1, origins.ctypes.data_as(_lib.f32p), axes.ctypes.data_as(_lib.f32p),
                                          C.byref(fst), po, None)]

    def refused(opts, word):
        for status in forms(opts):
            assert status == _lib.NT_E_UNSUPPORTED, (word, status, _lib.last_error())
            assert _lib.last_error().startswith("outlines") and word in _lib.last_error(), _lib.last_error()
        assert bytes(dest) == b"\x4e" * size

    # a supersampling factor, adaptive or not
    sc.set_supersampling(2)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(None)
    sc.set_supersampling(1)
    # bands
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "band")
    # statistics
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    # a lens, the parallel projection, ambient occlusion
    sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    sc.set_lens(None)
    sc.set_parallel_projection(2.0)
    refused(None, "parallel")
    sc.set_parallel_projection(None)
    sc.set_ambient_occlusion(4, 1.0)
    refused(None, "ambient occlusion")
    sc.set_ambient_occlusion(None)
    sc.set_supersampling(3)
    with pytest.raises(NotImplementedError, match="outlines"):
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, sc)
    # with the setting off again the other settings' own refusals are back, in their own words
    sc.set_outlines(None)
    sc.set_supersampling(1)
    sc.set_ambient_occlusion(4, 1.0)
    sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    for status in forms(None):
        assert status == _lib.NT_E_UNSUPPORTED and _lib.last_error().startswith("ambient occlusion")
    # each of them in the setting's own words, which tests/view_setting_refusals.py has byte for byte and
    # tests/test_view_setting_refusals.py holds every render form to; the seventh, the row range, is a guard for callers inside
    # nt_api.cpp, which the same test reads
    import view_setting_refusals as vr
    words = [m for (setting, _), m in vr.RENDER_REFUSALS.items() if setting == "outlines"]
    assert len(words) == 6 and all(m.startswith("outlines are not available") for m in words)
