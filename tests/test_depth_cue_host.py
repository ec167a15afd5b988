"""Depth cues, the part that needs no GPU: the conditions that keep tests/test_depth_cue_gpu.py from being vacuous, asserted on
the oracle's factors (tests/cue_cases.py); every answer the ABI gives before a device is touched; the setting's round trip; the
exported symbols and the Python signatures; and the kernel routes, pinned to the C++ that picks them the way
tests/test_outlines_host.py pins OUTLINE_ROUTES: every hipLaunchKernelGGL of launch_cue_fixed (nt_cue.hpp) and of
nt_launch_cue_factors and nt_launch_cue_apply (nt_var.hip) has a row in CUE_ROUTES, and every row names cases that
tests/test_depth_cue_gpu.py runs."""
import ctypes as C
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import cue_cases as cc
import fixtures as fx
import ntracer_amd
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = [("cell120_n4", {}), ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"})]
SCALAR = [("simplex10_n10", {})]
GENERAL = [("cell120_n4", {"NTRACER_FORCE_VAR": "1"}), ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}), ("feature5_n5", {}),
           ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}), ("feature11_n11", {}), ("lit12_n12", {}), ("feature16_n16", {})]
# kernel instantiation as its hipLaunchKernelGGL spells it (spaces dropped) -> what launches it in test_depth_cue_gpu.py: (scene,
# switches) cases of cue_cases.CASES for the factor kernels and the walk, (scene, variant) entries of cue_cases.RENDERED for the
# kernels only a render launches
CUE_ROUTES = [
    ("packet_numerators<N>", PLAIN + SCALAR),
    ("composite_packet<N,32,false,false,true>", PLAIN),
    ("composite_packet<N,32,false,true,true>", SCALAR),
    ("cue_factors_fixed<N>", PLAIN + SCALAR),
    ("cue_shade<N,false,false>", [("cell120_n4", "")]),
    ("cue_shade<N,true,false>", [("cell600_n4", "lit")]),
    ("cue_shade<N,true,true>", [("simplex10_n10", "")]),
    ("cue_factors", GENERAL),
    ("cue_apply", [("feature5_n5", "")]),
]
RENDER_ROWS = ("cue_shade<N,false,false>", "cue_shade<N,true,false>", "cue_shade<N,true,true>", "cue_apply")


def _traits(n, flat, params, env):
    m = np.asarray(flat["materials"]).reshape(-1, 10)
    opaque, reflective = bool((m[:, 6] >= 1).all()), bool((m[:, 7] > 0).any())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    faithful = not opaque or (solids and env.get("NTRACER_CLEAN_NORMALS") != "1")
    packet = not faithful and not var and env.get("NTRACER_COMPOSITE_KERNEL", "0") == "0"
    lights = np.asarray(params["point_light_color"]).size + np.asarray(params["global_light_color"]).size > 0
    return packet, scalar, (lights or reflective or scalar)


def _factor_routes(name, env):
    """the kernels nt_depth_cue_factors launches for a (scene, switches) case, by the rule of enqueue_cue (nt_api.cpp) and
    launch_cue_fixed (the golden trees are shallower than the packet walk's stack)"""
    g, n, flat = rq.scene(name)
    packet, scalar, _ = _traits(n, flat, fx.params_of(g), env)
    if not packet:
        return {"cue_factors"}
    return {"packet_numerators<N>", "composite_packet<N,32,false,%s,true>" % ("true" if scalar else "false"), "cue_factors_fixed<N>"}


def _render_route(name, variant):
    """the kernel that draws a render of cue_cases.RENDERED"""
    n, flat, params = rc.case_scene((name, {}, variant))
    packet, scalar, feat = _traits(n, flat, params, {})
    if not packet:
        return "cue_apply"
    return "cue_shade<N,%s,%s>" % ("true" if feat else "false", "true" if scalar else "false")


def test_every_cue_launch_has_a_row_and_every_row_a_gpu_case():
    var = sup.source("nt_var.hip")
    launched = sup.launches_through(sup.source("nt_cue.hpp"), "int launch_cue_fixed(")
    assert len(launched) == 7
    for head in ("int nt_launch_cue(", "int nt_launch_cue_factors_fixed(", "static int nt_launch_cue_packet(", "int nt_launch_cue_factors(",
                 "int nt_launch_cue_apply("):
        launched |= sup.launches(sup.function_body(var, head))
    rows = [k for k, _ in CUE_ROUTES]
    assert len(rows) == len(set(rows)) == 9
    assert set(rows) == launched, (sorted(launched - set(rows)), sorted(set(rows) - launched))
    cases = [(name, tuple(sorted(env.items()))) for name, env in cc.CASES]
    for kernel, ways in CUE_ROUTES:
        assert ways, kernel
        for way in ways:
            if kernel in RENDER_ROWS:
                assert way in cc.RENDERED, (kernel, way)
                assert _render_route(*way) == kernel, (kernel, way, _render_route(*way))
            else:
                name, env = way
                assert (name, tuple(sorted(env.items()))) in cases, (kernel, name, env)
                assert kernel in _factor_routes(name, env), (kernel, name, env, _factor_routes(name, env))
    # every case and every rendered scene lands on rows of the table
    for name, env in cc.CASES:
        assert _factor_routes(name, env) <= set(rows), (name, env)
    assert {_render_route(*r) for r in cc.RENDERED} == set(RENDER_ROWS)
    # the rule above is enqueue_cue's own: composite_route's answer, no term of its own, no getenv of its own
    api = sup.source("nt_api.cpp")
    rule, enq = sup.function_body(api, "CompositeRoute composite_route("), sup.function_body(api, "int enqueue_cue(")
    assert "r.packet_walk = !r.faithful && !r.var && sw.composite_kernel == 0 && std::max(s->depth + 1, 2) <= 32;" in rule
    assert "const bool fast = composite_route(s, sw).packet_walk;" in enq and "all_opaque" not in enq and "getenv" not in enq
    for name in ("nt_cue.hpp", "nt_inst_cue.hip"):
        assert "getenv" not in sup.source(name)
    assert api.count("getenv(") == sup.function_body(api, "RenderSwitches read_switches(").count("getenv(")
    # the cue's dispatch and its check stand in front of every other setting's
    body = sup.function_body(api, "int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in) {")
    assert 0 < body.index("return enqueue_cue(") < body.index("return enqueue_outlines(")
    # (render_checks walks the table of the settings, the cue above the outlines: of the two the cue refuses, as
    # tests/test_view_setting_refusals.py finds of the library)
    import view_setting_refusals as vr
    assert vr.RENDER_REFUSALS["cue", "outlines"] == "depth cues are not available while outlines are on"
    assert ("outlines", "cue") not in vr.RENDER_REFUSALS and "kViewSettings" in sup.function_body(api, "int render_checks(")
    # the rule is written once, for both routes
    hpp = sup.source("nt_cue.hpp")
    assert len(re.findall(r"void cue_pixel\(", hpp)) == 1 and len(re.findall(r"void cue_blend\(", hpp)) == 1
    assert "cue_pixel(" in var and "cue_blend(" in var and "inv_fog" not in var and "fog_strength" not in var
    # the new launches stay out of the launchers that were there
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_hits.hpp", "int launch_hits_fixed("), ("nt_var.hip", "int nt_launch_hits("),
                      ("nt_lens.hpp", "int launch_lens_fixed("), ("nt_outline.hpp", "int launch_outline_fixed("),
                      ("nt_var.hip", "int nt_launch_outline_mark("), ("nt_var.hip", "int nt_launch_outline_apply("),
                      ("nt_ao.hpp", "int launch_ao_fixed("), ("nt_var.hip", "int nt_launch_ao(")):
        assert not any(k.startswith("cue_") for k in sup.launches(sup.function_body(sup.source(src), head))), head
    assert "cue" not in sup.source("nt_composite.hpp")                       # the headline kernel is untouched


# ------------------------------------------------------------------ the conditions that keep the GPU tests from being vacuous
CENSUS = {"cell120_n4": (270, (41, 188, 41)), "feature5_n5": (132, (20, 92, 20)), "simplex10_n10": (16, (4, 8, 4)),
          "feature11_n11": (79, (12, 55, 12)), "lit12_n12": (94, (15, 65, 14))}


@pytest.mark.parametrize("name", sorted({c[0] for c in cc.CASES} | {r[0] for r in cc.RENDERED}))
def test_both_ramps_have_their_ends_and_their_middle(name):
    hits, fs, gs = cc.check_not_vacuous(name)
    if name in CENSUS:
        assert (hits, fs) == CENSUS[name]


def test_the_cases_cover_what_the_rule_distinguishes():
    import primary_hit_cases as ph
    # pixels with transparent hits only: left alone even under fog_background
    for k in cc.CAMERAS:
        e = ph.expected(("feature11_n11", {}), cc.W, cc.H, k)
        only = (e["item"] < 0) & (e["n_transparent"] > 0)
        assert only.sum() >= 9, (k, int(only.sum()))
        fg = cc.expected(("feature11_n11", {}), cc.W, cc.H, k, cc.setting("feature11_n11", background=True))
        assert (fg[only] == -1).all() and (fg[..., 0][(e["item"] < 0) & ~only] == 1).all() and ((e["item"] < 0) & ~only).sum() > 100
    # a view that hits nothing
    assert (ph.expected(("simplex10_n10", {}), 9, 7, 0)["item"] < 0).all()
    assert (cc.expected(("simplex10_n10", {}), 9, 7, 0, cc.setting("simplex10_n10"))[..., 0] == -1).all()
    # camera 1 spreads the hidden coordinates camera 0 keeps constant
    for name, least in (("cell120_n4", 1.0), ("feature5_n5", 1.5)):
        spread = []
        for k in cc.CAMERAS:
            e = ph.expected((name, {}), cc.W, cc.H, k)
            d, o = ph.rays(name, cc.W, cc.H, k)[0], ph.camera(name, k)[0]
            x = (d * e["dist"][..., None] + o)[e["item"] >= 0][:, 3:]
            spread.append(float((x.max(axis=0) - x.min(axis=0)).max()))
        assert spread[0] < 1e-3 and spread[1] > least, (name, spread)
    # without a tint g is -1 everywhere, and the blend with nothing to do is P itself
    fg = cc.expected(("cell120_n4", {}), cc.W, cc.H, 0, cc.setting("cell120_n4", tint=False))
    assert (fg[..., 1] == -1).all()
    P = np.random.default_rng(3).random((cc.H, cc.W, 3), np.float32)
    empty = cc.setting("cell120_n4", tint=False, strength=0.0)
    assert np.array_equal(cc.blend(P, fg[..., 0], fg[..., 1], empty).view(np.uint32), P.view(np.uint32))
    full = cc.expected(("cell120_n4", {}), cc.W, cc.H, 0, cc.setting("cell120_n4"))
    assert (cc.blend(P, full[..., 0], full[..., 1], cc.setting("cell120_n4")) != P).any(axis=2).sum() >= 200


# ------------------------------------------------------------------ the ABI and the Python surface
NAMES = ("nt_scene_set_depth_cue", "nt_scene_get_depth_cue", "nt_depth_cue_factors", "nt_depth_cue_factors_device")


def test_the_exported_symbols_the_header_and_the_python_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, code), name
    struct = re.search(r"typedef struct nt_depth_cue \{(.*?)\} nt_depth_cue;", code, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", struct)
    assert fields == ["fog_near", "fog_far", "fog_color", "fog_strength", "fog_background", "tint_lo", "tint_hi", "tint_color_lo", "tint_color_hi"]
    assert [f[0] for f in _lib.NtDepthCue._fields_] == fields and C.sizeof(_lib.NtDepthCue) == 60
    assert "int nt_scene_set_depth_cue(nt_scene_t *s, const nt_depth_cue *cue, const float *tint_axis);" in code
    # the header carries the rule
    for phrase in ("inv_fog = 1.0f / (fog_far - fog_near)", "clamp01((t - fog_near) * inv_fog)", "x_k = (d_k * t) + o_k",
                   "(tint_color_lo.c * (1.0f - g)) + (tint_color_hi.c * g)", "(Q.c * (1.0f - w)) + (fog_color.c * w)"):
        assert phrase in header, phrase
    for cls in (tracern.CompositeScene, tracern.BoxScene):
        params = [(p.name, p.default) for p in list(inspect.signature(cls.set_depth_cue).parameters.values())[1:]]
        assert params == [("near", 0.0), ("far", 1.0), ("color", (0, 0, 0)), ("strength", 1.0), ("background", False), ("tint_axis", None),
                          ("tint_range", None), ("tint_colors", None)]
        params = [(p.name, p.default) for p in list(inspect.signature(cls.depth_cue_factors).parameters.values())[1:]]
        assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", None), ("strict_reference", None)]
        assert isinstance(inspect.getattr_static(cls, "depth_cue"), property) and inspect.getattr_static(cls, "depth_cue").fset is None
    # methods of the scenes alone: the package exports no new name
    assert not [n for n in ntracer_amd.__all__ if "cue" in n.lower()] and "Scene" in ntracer_amd.__all__


def _scene(name="cell120_n4"):
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat), n


def _cue(**kw):
    c = _lib.NtDepthCue()
    c.fog_near, c.fog_far, c.fog_strength, c.fog_background = 1.0, 3.0, 0.5, 0
    c.fog_color[:] = (0.25, 0.5, 0.75)
    c.tint_lo, c.tint_hi = -1.0, 1.0
    c.tint_color_lo[:] = (1.0, 0.5, 0.25)
    c.tint_color_hi[:] = (0.25, 0.5, 1.0)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[:] = v
        else:
            setattr(c, k, v)
    return c


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    sc, n = _scene()
    assert sc.depth_cue is None
    sc.set_depth_cue()
    assert sc.depth_cue == dict(near=0.0, far=1.0, color=(0.0, 0.0, 0.0), strength=1.0, background=False, tint_axis=None, tint_range=None,
                                tint_colors=None)
    sc.set_depth_cue(1.5, 4.0, (1, 0.5, 0.25), 0.75, True, tint_axis=tracern.Vector(4, (0, 0, 0, 1)), tint_range=(-2, 0.5),
                     tint_colors=((1, 0, 0), (0, 0, 1)))
    assert sc.depth_cue == dict(near=1.5, far=4.0, color=(1.0, 0.5, 0.25), strength=0.75, background=True, tint_axis=(0.0, 0.0, 0.0, 1.0),
                                tint_range=(-2.0, 0.5), tint_colors=((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)))
    sc.set_depth_cue(far=2.0, tint_axis=[0.5, -0.25, 0.75, 1.0], tint_range=(0, 1), tint_colors=((1, 1, 1), (0, 0, 0)))
    assert sc.depth_cue["tint_axis"] == (0.5, -0.25, 0.75, 1.0) and sc.depth_cue["far"] == 2.0
    # the ABI's getter through whichever pointers are given
    on, tint, got, axis = C.c_int(-1), C.c_int(-1), _lib.NtDepthCue(), (C.c_float * n)(*([-1] * n))
    assert L.nt_scene_get_depth_cue(sc._handle, C.byref(on), None, None, None) == 0 and on.value == 1
    assert L.nt_scene_get_depth_cue(sc._handle, None, C.byref(got), None, None) == 0 and (got.fog_far, got.tint_hi) == (2.0, 1.0)
    assert L.nt_scene_get_depth_cue(sc._handle, None, None, C.byref(tint), axis) == 0 and tint.value == 1 and list(axis) == [0.5, -0.25, 0.75, 1.0]
    assert L.nt_scene_get_depth_cue(sc._handle, None, None, None, None) == 0
    assert L.nt_scene_get_depth_cue(None, C.byref(on), None, None, None) == _lib.NT_E_INVALID
    # without an axis the tint's fields are not read and come back as zeroes
    assert L.nt_scene_set_depth_cue(sc._handle, C.byref(_cue(tint_lo=5.0, tint_hi=float("nan"), tint_color_lo=(7.0, 7.0, 7.0))), None) == 0
    assert L.nt_scene_get_depth_cue(sc._handle, None, C.byref(got), C.byref(tint), axis) == 0
    assert tint.value == 0 and list(axis) == [0.0] * n and (got.tint_lo, got.tint_hi, list(got.tint_color_lo)) == (0.0, 0.0, [0.0] * 3)
    assert sc.depth_cue["tint_axis"] is None and sc.depth_cue["near"] == 1.0
    # every refusal leaves it as it was
    ax = (C.c_float * n)(0.5, -0.25, 0.75, 1.0)
    assert L.nt_scene_set_depth_cue(sc._handle, C.byref(_cue()), ax) == 0
    keep = sc.depth_cue
    nan, inf = float("nan"), float("inf")
    tiny = float(np.float32(1e-45))
    refused = [(_cue(fog_near=v), ax) for v in (-0.001, nan, inf, -inf, 3.0, 3.5)]
    refused += [(_cue(fog_far=v), ax) for v in (nan, inf, 1.0, 0.5)]
    refused += [(_cue(fog_near=0.0, fog_far=tiny), ax)]                          # the reciprocal overflows
    refused += [(_cue(fog_strength=v), ax) for v in (-0.001, 1.001, nan, inf)]
    refused += [(_cue(tint_lo=v), ax) for v in (nan, inf, -inf, 1.0, 2.0)]
    refused += [(_cue(tint_hi=v), ax) for v in (nan, inf, -1.0)]
    refused += [(_cue(tint_lo=0.0, tint_hi=tiny), ax)]
    for field in ("fog_color", "tint_color_lo", "tint_color_hi"):
        for k in range(3):
            for v in (-0.001, 1.001, nan, inf):
                col = [0.5, 0.5, 0.5]
                col[k] = v
                refused.append((_cue(**{field: tuple(col)}), ax))
    refused += [(_cue(), (C.c_float * n)(0, 0, 0, 0))]
    refused += [(_cue(), (C.c_float * n)(*[v if j == k else 1.0 for j in range(n)])) for k in (0, n - 1) for v in (nan, inf, -inf)]
    for cue, axis_arg in refused:
        assert L.nt_scene_set_depth_cue(sc._handle, C.byref(cue), axis_arg) == _lib.NT_E_INVALID, (cue.fog_near, cue.fog_far, cue.tint_lo, cue.tint_hi)
        assert "depth cue" in _lib.last_error()
        assert sc.depth_cue == keep
    assert L.nt_scene_set_depth_cue(None, C.byref(_cue()), ax) == _lib.NT_E_INVALID
    for bad in (dict(near=True), dict(near="0"), dict(far=None), dict(strength="1"), dict(color=(0, 0)), dict(color=(0, 0, 2)),
                dict(near=-1.0), dict(near=2.0, far=1.0), dict(far=float("nan")), dict(strength=1.5),
                dict(tint_axis=(0, 0, 0, 1)), dict(tint_range=(0, 1)), dict(tint_colors=((1, 1, 1), (0, 0, 0))),
                dict(tint_axis=(0, 0, 0, 1), tint_range=(0, 1)), dict(tint_axis=(0, 0, 0, 1), tint_colors=((1, 1, 1), (0, 0, 0))),
                dict(tint_axis=(0, 0, 1), tint_range=(0, 1), tint_colors=((1, 1, 1), (0, 0, 0))),
                dict(tint_axis=(0, 0, 0, 0), tint_range=(0, 1), tint_colors=((1, 1, 1), (0, 0, 0))),
                dict(tint_axis=(0, 0, 0, 1), tint_range=(1, 1), tint_colors=((1, 1, 1), (0, 0, 0))),
                dict(tint_axis=(0, 0, 0, 1), tint_range=(0, 1), tint_colors=((1, 1), (0, 0, 0)))):
        with pytest.raises((ValueError, TypeError)):
            sc.set_depth_cue(**bad)
        assert sc.depth_cue == keep
    # the limits are in
    sc.set_depth_cue(0.0, 1e-30, (1, 1, 1), 0.0)
    sc.set_depth_cue(0.0, 1e30, (0, 0, 0), 1.0, tint_axis=(0, 0, 0, 1e-30), tint_range=(-1e30, 1e30), tint_colors=((0, 0, 0), (1, 1, 1)))
    # locked while a render holds the scene, as nt_scene_set_camera
    assert L.nt_scene_lock(sc._handle) == 0
    keep = sc.depth_cue
    assert L.nt_scene_set_depth_cue(sc._handle, C.byref(_cue()), ax) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_depth_cue(sc._handle, None, None) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        sc.set_depth_cue()
    assert sc.depth_cue == keep
    assert L.nt_scene_unlock(sc._handle) == 0
    # off
    sc.set_depth_cue(None)
    assert sc.depth_cue is None
    assert L.nt_scene_get_depth_cue(sc._handle, C.byref(on), C.byref(got), None, None) == 0 and on.value == 0 and got.fog_far == 0.0
    # a view setting like fov, kept in the native handle: no part of what is pickled, and not carried over by with_rebuilt_tree or
    # to another scene made from the same description
    before = pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2)
    sc.set_depth_cue(1.0, 2.0)
    assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before
    assert not any("cue" in k for k in sc.__dict__)
    assert sc.with_rebuilt_tree().depth_cue is None and sc.depth_cue is not None
    assert _scene()[0].depth_cue is None
    # a BoxScene has no records
    box = tracern.BoxScene(4)
    assert L.nt_scene_set_depth_cue(box._handle, C.byref(_cue()), None) == _lib.NT_E_INVALID
    assert L.nt_scene_set_depth_cue(box._handle, None, None) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_depth_cue()
    assert box.depth_cue is None


def test_the_factor_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    sc, n = _scene()
    box = tracern.BoxScene(4)
    out = np.full(8 * 4 * 2, 77, np.float32)
    host = lambda s, w, h, p: L.nt_depth_cue_factors(s, w, h, p, None)
    devf = lambda s, w, h, p: L.nt_depth_cue_factors_device(s, w, h, p, None, None)
    for call in (host, devf):
        # the setting is off
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "off" in _lib.last_error()
        sc.set_depth_cue()
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
        sc.set_depth_cue(None)
    assert (out == 77).all()
    sc.set_depth_cue()
    # the options of the _device form: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        assert L.nt_depth_cue_factors_device(sc._handle, 8, 4, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the Python forms
    with pytest.raises(ValueError):
        sc.depth_cue_factors(0, 4)
    with pytest.raises(ValueError, match="not a composite scene"):
        box.depth_cue_factors(8, 4)
    sc.set_depth_cue(None)
    with pytest.raises(ValueError, match="off"):
        sc.depth_cue_factors(8, 4)


def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device: NT_E_UNSUPPORTED with a message that starts "depth cue", the
    destination as it was (the table form needs a device to make its table: test_depth_cue_gpu.py).  There is no device here: a
    refusal that reached one would show as another error."""
    L = _lib.lib()
    sc, n = _scene()
    sc.set_depth_cue(1.0, 2.0)
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
            assert _lib.last_error().startswith("depth cue") and word in _lib.last_error(), _lib.last_error()
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
    # a lens, the parallel projection, ambient occlusion, outlines
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
    with pytest.raises(NotImplementedError, match="depth cue"):
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, sc)
    # with the setting off again the other settings' own refusals are back, in their own words
    sc.set_depth_cue(None)
    sc.set_ambient_occlusion(4, 1.0)
    for status in forms(None):
        assert status == _lib.NT_E_UNSUPPORTED and _lib.last_error().startswith("outlines")
    # each of them in the setting's own words, which tests/view_setting_refusals.py has byte for byte and
    # tests/test_view_setting_refusals.py holds every render form to; the eighth, the row range, is a guard for callers inside
    # nt_api.cpp, which the same test reads
    import view_setting_refusals as vr
    words = [m for (setting, _), m in vr.RENDER_REFUSALS.items() if setting == "cue"]
    assert len(words) == 7 and all(m.startswith("depth cues are not available") for m in words)
