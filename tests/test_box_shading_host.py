"""BoxScene face shading (BoxScene.set_face_shading, face_shading, ntracer_amd.face_palette, nt_scene_set_box_shading /
nt_scene_get_box_shading and the renders that honour the setting) without a GPU: the setting's round trips and refusals, that the
expected frames of tests/box_shading_cases.py exercise what the GPU comparisons are meant to exercise, what the renders refuse
before they touch a device, and the pins on the sources."""
import ctypes as C
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import box_hit_cases as bc
import box_shading_cases as sc_
import ntracer_amd
import ray_query_cases as rq
import view_setting_refusals as vr
import support as sup
from ntracer_amd import _lib, build, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")
f32 = np.float32


# ------------------------------------------------------------------ the surface
def test_the_symbols_the_header_and_the_python_signatures():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_scene_set_box_shading", "nt_scene_get_box_shading"):
        assert hasattr(raw, name), name
    params = [(p.name, p.default, p.kind) for p in list(inspect.signature(tracern.BoxScene.set_face_shading).parameters.values())[1:]]
    kw = inspect.Parameter.KEYWORD_ONLY
    assert params == [("colors", None, inspect.Parameter.POSITIONAL_OR_KEYWORD), ("near", None, kw), ("far", None, kw), ("color", (0, 0, 0), kw),
                      ("strength", 1.0, kw), ("background", False, kw), ("tint_axis", None, kw), ("tint_range", None, kw),
                      ("tint_colors", None, kw)]
    prop = inspect.getattr_static(tracern.BoxScene, "face_shading")
    assert isinstance(prop, property) and prop.fset is None
    for name in ("set_face_shading", "face_shading"):
        assert hasattr(ntracer_amd.NTracer(4).BoxScene, name) and not hasattr(tracern.CompositeScene, name)
    assert ntracer_amd.face_palette is tracern.face_palette and "face_palette" in ntracer_amd.__all__
    assert not [n for n in ntracer_amd.__all__ if "cue" in n.lower()]
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    sec = header[header.index("BoxScene face shading"):]
    for phrase in ("shade = fabsf(d_i) and B.c = shade * T[i][l][c]", "every entry is (1.0f, 0.5f, 0.5f)", "P.c = clamp01(B.c)",
                   "f = clamp01((t - fog_near) * inv_fog)", "x_k = (d_k * t) + o_k", "g = clamp01((s - tint_lo) * inv_tint)",
                   "with fog_background set f = 1, g = -1", "without a cue f = g = -1 everywhere",
                   "Q.c = P.c * ((tint_color_lo.c * (1.0f - g)) + (tint_color_hi.c * g))", "w = f * fog_strength and Q.c = (Q.c * (1.0f - w)) + (fog_color.c * w)",
                   "(Q.c * (1.0f - strength)) + (color.c * strength)", "the frame is the plain frame byte for byte, in every format",
                   "face_colors == NULL && cue == NULL takes the setting off", "not a box scene", "not part of a\n   pickled scene",
                   "nt_scene_set_supersampling_scratch_mb", "no buffer entry point of its own"):
        assert phrase in sec, phrase
    for fn in ("nt_scene_set_box_shading", "nt_scene_get_box_shading"):
        assert re.search(r"\bint %s\(" % fn, sec), fn


def test_the_palette():
    for n in (1, 3, 6, 25):
        t = ntracer_amd.face_palette(n)
        assert t.dtype == np.float32 and t.shape == (n, 2, 3) and (t >= 0).all() and (t <= 1).all()
        assert np.array_equal(t, ntracer_amd.face_palette(n))                      # deterministic
        assert (t[:, 1].max(axis=1) == 1.0).all() and (t[:, 0].max(axis=1) == 0.5).all()       # +1 at full value, -1 darker
        assert len({tuple(c) for c in t[:, 1]}) == n                               # one hue an axis
    assert np.array_equal(ntracer_amd.face_palette(3)[:, 1], np.eye(3, dtype=np.float32))     # red, green, blue: spread evenly
    tracern.BoxScene(6).set_face_shading(ntracer_amd.face_palette(6))
    with pytest.raises(ValueError):
        ntracer_amd.face_palette(0)


def _get(box):
    """the ABI's getter, everything"""
    n = box.dimension
    on, hc, hq, ht, cue = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1), _lib.NtDepthCue()
    table, axis = np.full(6 * n, -7, f32), np.full(n, -7, f32)
    assert _lib.lib().nt_scene_get_box_shading(box._handle, C.byref(on), C.byref(hc), table.ctypes.data_as(_lib.f32p), C.byref(hq), C.byref(cue),
                                               C.byref(ht), axis.ctypes.data_as(_lib.f32p)) == 0
    return (on.value, hc.value, table.tobytes(), hq.value, bytes(cue), ht.value, axis.tobytes())


def _cue(**fields):
    cue = _lib.NtDepthCue()
    cue.fog_near, cue.fog_far, cue.fog_strength = 1.0, 2.0, 0.5
    cue.tint_lo, cue.tint_hi = -1.0, 1.0
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(cue, k)[:] = v
        else:
            setattr(cue, k, v)
    return cue


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    n = 5
    box = tracern.BoxScene(n)
    assert box.face_shading is None
    assert _get(box)[:2] == (0, 0) and np.array_equal(np.frombuffer(_get(box)[2], f32).reshape(n, 2, 3), sc_.default_table(n))
    T = sc_.table(n)
    # colours alone
    box.set_face_shading(T)
    got = box.face_shading
    assert np.array_equal(got.pop("colors"), T) and set(got.values()) == {None}
    # fog alone; far is needed, near is 0 without one
    box.set_face_shading(near=1, far=3, color=(0.25, 0.5, 1), strength=0.5, background=True)
    assert box.face_shading == dict(colors=None, near=1.0, far=3.0, color=(0.25, 0.5, 1.0), strength=0.5, background=True, tint_axis=None,
                                    tint_range=None, tint_colors=None)
    box.set_face_shading(far=2.5)
    assert (box.face_shading["near"], box.face_shading["far"], box.face_shading["strength"]) == (0.0, 2.5, 1.0)
    # a tint alone: no fog arguments means fog_strength = 0 with near, far = 0, 1
    axis = (1.0, -2.0, 3.0, -4.0, 5.0)
    box.set_face_shading(tint_axis=axis, tint_range=(-2, 2), tint_colors=((1, 0, 0), (0, 0, 1)))
    assert box.face_shading == dict(colors=None, near=0.0, far=1.0, color=(0.0, 0.0, 0.0), strength=0.0, background=False, tint_axis=axis,
                                    tint_range=(-2.0, 2.0), tint_colors=((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)))
    # all three, with a Vector for the axis
    box.set_face_shading(T, near=0.5, far=9, tint_axis=tracern.Vector(n, axis), tint_range=(-2, 2), tint_colors=((1, 0, 0), (0, 0, 1)))
    got = box.face_shading
    assert np.array_equal(got["colors"], T) and got["tint_axis"] == axis and (got["near"], got["far"]) == (0.5, 9.0)
    # the ABI's getter through whichever pointers are given
    on = C.c_int(-1)
    assert L.nt_scene_get_box_shading(box._handle, C.byref(on), None, None, None, None, None, None) == 0 and on.value == 1
    assert L.nt_scene_get_box_shading(box._handle, None, None, None, None, None, None, None) == 0
    assert L.nt_scene_get_box_shading(None, C.byref(on), None, None, None, None, None, None) == _lib.NT_E_INVALID
    # every NT_E_INVALID cause leaves it as it was
    keep = _get(box)
    good_axis = np.array(axis, f32)
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.f32p)
    refused = []
    for v in (-0.001, 1.001, np.nan, np.inf, -np.inf):
        for at in (0, 7, 6 * n - 1):
            t = np.array(T, f32).reshape(-1)
            t[at] = v
            refused.append((t, None, None))
    nan, inf = float("nan"), float("inf")
    bad_cues = [dict(fog_near=-0.5), dict(fog_near=nan), dict(fog_far=inf), dict(fog_far=1.0), dict(fog_far=0.5), dict(fog_strength=1.5),
                dict(fog_strength=-0.1), dict(fog_strength=nan), dict(fog_color=(0.0, 2.0, 0.0)), dict(fog_color=(nan, 0.0, 0.0)),
                dict(fog_near=0.0, fog_far=1e-45)]                  # (1 / (fog_far - fog_near) is not finite)
    for fields in bad_cues:
        refused.append((None, _cue(**fields), None))
        refused.append((np.array(T, f32).reshape(-1), _cue(**fields), good_axis))
    bad_tints = [dict(tint_lo=1.0, tint_hi=1.0), dict(tint_lo=2.0), dict(tint_hi=inf), dict(tint_lo=nan), dict(tint_color_lo=(0.0, 0.0, 1.5)),
                 dict(tint_color_hi=(nan, 0.0, 0.0)), dict(tint_color_hi=(0.0, -0.5, 0.0))]
    for fields in bad_tints:
        refused.append((None, _cue(**fields), good_axis))
    for bad_axis in (np.zeros(n, f32), np.array([1, nan, 0, 0, 0], f32), np.array([inf, 0, 0, 0, 0], f32)):
        refused.append((None, _cue(), bad_axis))
    refused.append((None, None, good_axis))                      # a tint axis without the cue that holds its range and colours
    refused.append((np.array(T, f32).reshape(-1), None, good_axis))
    for t, cue, ax in refused:
        assert L.nt_scene_set_box_shading(box._handle, p(t), None if cue is None else C.byref(cue), p(ax)) == _lib.NT_E_INVALID
        assert _lib.last_error()
        assert _get(box) == keep
    assert L.nt_scene_set_box_shading(None, None, C.byref(_cue()), None) == _lib.NT_E_INVALID
    # ... in nt_scene_set_depth_cue's own words
    assert L.nt_scene_set_box_shading(box._handle, None, C.byref(_cue(fog_far=0.5)), None) == _lib.NT_E_INVALID
    assert _lib.last_error() == "the depth cue's fog range must be finite with 0 <= fog_near < fog_far"
    for bad in (dict(colors=np.zeros((n, 2, 2))), dict(colors=np.zeros((n + 1, 2, 3))), dict(colors=np.full((n, 2, 3), 2.0)), dict(near=1.0),
                dict(near=2.0, far=1.0), dict(far=True), dict(far=2.0, strength="1"), dict(far=2.0, color=(0, 0)), dict(far=2.0, strength=1.5),
                dict(tint_axis=axis), dict(tint_range=(-1, 1)), dict(tint_axis=axis[:-1], tint_range=(-1, 1), tint_colors=((0, 0, 0), (1, 1, 1))),
                dict(tint_axis=axis, tint_range=(1, 1), tint_colors=((0, 0, 0), (1, 1, 1))),
                # the fog's other arguments without far: refused, not dropped
                dict(strength=0.5), dict(colors=T, color=(1, 0, 0)), dict(background=True),
                dict(strength=0.5, tint_axis=axis, tint_range=(-2, 2), tint_colors=((1, 0, 0), (0, 0, 1)))):
        with pytest.raises((ValueError, TypeError)):
            box.set_face_shading(**bad)
        assert _get(box) == keep
    # the limits are in
    ones = np.ones(6 * n, f32)
    assert L.nt_scene_set_box_shading(box._handle, p(ones), C.byref(_cue(fog_near=0.0, fog_strength=1.0, fog_color=(1.0, 1.0, 1.0))), None) == 0
    assert L.nt_scene_set_box_shading(box._handle, p(np.zeros(6 * n, f32)), None, None) == 0
    # locked while a render holds the scene, as nt_scene_set_camera
    keep = _get(box)
    assert L.nt_scene_lock(box._handle) == 0
    assert L.nt_scene_set_box_shading(box._handle, p(ones), None, None) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_box_shading(box._handle, None, None, None) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        box.set_face_shading(T)
    assert _get(box) == keep
    assert L.nt_scene_unlock(box._handle) == 0
    # off: set_face_shading(None) with nothing else
    box.set_face_shading(None)
    assert box.face_shading is None and _get(box)[0] == 0
    box.set_face_shading(T)
    box.set_face_shading()
    assert box.face_shading is None
    # a view setting like fov, kept in the native handle: no part of what is pickled
    before = pickle.dumps({k: v for k, v in box.__dict__.items() if k != "_handle"}, 2)
    box.set_face_shading(T, far=2.0)
    assert pickle.dumps({k: v for k, v in box.__dict__.items() if k != "_handle"}, 2) == before
    assert not any("shad" in k for k in box.__dict__)
    assert box.face_shading is not None and tracern.BoxScene(n).face_shading is None
    # nt_scene_set_depth_cue on a BoxScene stays what it was
    assert L.nt_scene_set_depth_cue(box._handle, C.byref(_cue()), None) == _lib.NT_E_INVALID
    # a CompositeScene has depth cues of its own
    g, cn, flat = rq.scene("cell120_n4")
    comp = tracern.CompositeScene.from_flat(cn, flat)
    t4 = np.ones(6 * cn, f32)
    assert L.nt_scene_set_box_shading(comp._handle, p(t4), None, None) == _lib.NT_E_INVALID and "not a box scene" in _lib.last_error()
    assert L.nt_scene_set_box_shading(comp._handle, None, None, None) == _lib.NT_E_INVALID
    assert L.nt_scene_get_box_shading(comp._handle, C.byref(on), None, None, None, None, None, None) == _lib.NT_E_INVALID
    assert comp.depth_cue is None


# ------------------------------------------------------------------ the expected data is worth comparing against
@pytest.mark.parametrize("n", sc_.DIMS)
def test_the_views_show_what_the_comparisons_need(n):
    for name in ("faces", "diagonal"):
        for w, h in sc_.SIZES[1:]:
            e = bc.expected(n, sc_.CAMERAS[name], w, h)
            assert 3 <= len(e["faces"]) <= 9 and 9 <= int((e["mask"] != 0).sum()) <= 261, (n, name, w, h, len(e["faces"]))
            hit = e["item"] >= 0
            b = sc_.expected(n, name, w, h, "b")
            fh = b["f"][hit]
            assert (fh == 0).any() and ((fh > 0) & (fh < 1)).any() and (fh == 1).any(), (n, name, w, h)
            assert (b["f"][~hit] == 1).all() and (b["g"] == -1).all()
            d = sc_.expected(n, name, w, h, "d")
            assert ((d["f"][hit] > 0) & (d["f"][hit] < 1)).all() and ((d["g"][hit] > 0) & (d["g"][hit] < 1)).all(), (n, name, w, h)
            assert (d["f"][~hit] == -1).all() and (d["g"][~hit] == -1).all()
            # every setting shows, and the lines on top of it
            P = np.clip(e["colors"], f32(0), f32(1))
            for which in sc_.SETTINGS:
                x = sc_.expected(n, name, w, h, which)
                assert (x["rgb"] != P).any(axis=2).sum() >= 9, (n, name, w, h, which)
                assert (x["rgb"] >= 0).all() and (x["rgb"] <= 1).all()
            x = sc_.expected(n, name, w, h, "e")
            assert np.array_equal(x["Q"], d["Q"]) and ((x["rgb"] != x["Q"]).any(axis=2) <= (e["mask"] != 0)).all()
            assert (x["rgb"] != x["Q"]).any(axis=2).sum() >= 9
            # the table's colours are told apart: g != b on the faces
            a = sc_.expected(n, name, w, h, "a")
            assert (a["rgb"][hit][:, 1] != a["rgb"][hit][:, 2]).any()
    c = sc_.expected(n, "diagonal", 70, 37, "c")
    hit = bc.expected(n, sc_.CAMERAS["diagonal"], 70, 37)["item"] >= 0
    assert (c["g"][hit] == 0).any() and (c["g"][hit] == 1).any(), n
    e = bc.expected(n, sc_.CAMERAS["on-plane"], 70, 37)
    assert len(e["faces"]) == 1 and (e["mask"] == bc.SILHOUETTE).any() and not (e["mask"] & bc.CREASE).any()
    for size in sc_.SIZES:
        assert not (bc.expected(n, sc_.CAMERAS["nothing"], *size)["item"] >= 0).any()


@pytest.mark.parametrize("n", sc_.DIMS)
def test_the_rule_with_the_default_table_is_the_plain_colour(n):
    for name in sc_.CAMERAS:
        for w, h in sc_.SIZES:
            k = sc_.CAMERAS[name]
            e = bc.expected(n, k, w, h)
            o = bc.camera(n, k)[0]
            # (the plain frame: the colours clamped as the packer clamps them, which leaves no negative zero)
            plain = np.clip(e["colors"], f32(0), f32(1)) + f32(0)
            assert np.array_equal(plain, e["colors"]) and not np.signbit(plain).any()
            for kw in ({}, dict(colors=sc_.default_table(n))):
                x = sc_.shade(o, e, **kw)
                assert np.array_equal(x["B"].view(np.uint32), e["colors"].view(np.uint32)), (n, name, w, h)
                assert np.array_equal(x["rgb"].view(np.uint32), plain.view(np.uint32))
            # ... and a fog of strength 0 without a tint leaves it alone
            x = sc_.shade(o, e, near=0.5, far=3.0, color=(1, 0, 1), strength=0.0, background=True)
            assert np.array_equal(x["rgb"].view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------ refusals
def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device: NT_E_UNSUPPORTED in "face shading is not available ..." words, the
    destination as it was; with face lines on as well, face lines' recorded words"""
    L = _lib.lib()
    n = 5
    box = tracern.BoxScene(n)
    box.set_face_shading(sc_.table(n), far=3.0)
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

    def refused(opts, cause):
        want = vr.RENDER_REFUSALS["face lines", cause]
        for lines in (False, True):
            box.set_face_lines() if lines else box.set_face_lines(None)
            for status in forms(opts):
                assert status == _lib.NT_E_UNSUPPORTED, (cause, status, _lib.last_error())
                if lines:
                    assert _lib.last_error() == want
                else:
                    # the table's rule: the same sentence with this row's subject and no band suffix
                    assert _lib.last_error() == want.replace("face lines are", "face shading is").split(": a pixel's")[0]
                    assert _lib.last_error().startswith("face shading is not available")
            assert bytes(dest) == b"\x4e" * size
        box.set_face_lines(None)

    box.set_supersampling(2)
    refused(None, "supersampling")
    box.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    box.set_adaptive_supersampling(None)
    box.set_supersampling(1)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "bands")
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    box.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    box.set_lens(None)
    box.set_parallel_projection(2.0)
    refused(None, "parallel")
    box.set_parallel_projection(None)
    box.set_supersampling(3)
    with pytest.raises(NotImplementedError, match="face shading"):
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, box)
    assert not box.locked
    # the row is the table's last, has no words for the rows above it, and enqueue asks it ahead of the face lines' line
    api = sup.source("nt_api.cpp")
    table = api[api.index("const ViewSetting kViewSettings[VS_COUNT] = {"):]
    table = table[:table.index("\n};")]
    assert table.rstrip().splitlines()[-1].strip() == \
        '{[](const nt_scene *s) { return s->box_shading && !s->composite; }, "face shading is", "", nullptr, nullptr},'
    enq = sup.function_body(api, "int enqueue(nt_scene *s, DeviceState *ds, const FrameJob &job_in) {")
    assert enq.index("enqueue_box_shading(") < enq.index("enqueue_box_lines(") < enq.index("enqueue_lens(")
    assert "for a row range" in sup.function_body(api, "int whole_view_check(")


@pytest.mark.skipif(_lib.lib().nt_device_count() > 0, reason="checks the no-GPU behaviour")
def test_without_a_gpu_the_render_fails_loudly():
    for lines in (False, True):
        box = tracern.BoxScene(4)
        box.set_face_shading(sc_.table(4))
        if lines:
            box.set_face_lines()
        with pytest.raises(RuntimeError, match="no HIP device"):
            ntracer_amd.BlockingRenderer().render(bytearray(8 * 4 * 4), sup.fmt_of(8, 4), box)
        assert not box.locked


# ------------------------------------------------------------------ the sources
def test_the_units_the_dispatch_and_no_switch_of_its_own():
    units = [(name, flags) for name, src, flags in build.units() if src == "nt_inst_boxshade.hip"]
    assert sorted(int(f[0].split("=")[1]) for _, f in units) == list(range(3, 25))
    assert len({name for name, _ in units}) == 22
    assert os.path.join(CSRC, "nt_boxshade.hpp") in [os.path.normpath(p) for p in build.HDR]
    src = sup.source("nt_inst_boxshade.hip")
    assert "#ifndef NT_INST_N\n#error" in src and "nt_box_shade<NT_INST_N>" in src and "_fixed" not in src
    out = os.popen("nm -D -C --defined-only %s" % _lib.LIB_PATH).read()
    assert sorted(int(v) for v in re.findall(r"\bnt_box_shade<(\d+)>\(", out)) == list(range(3, 25))
    hpp = sup.source("nt_boxshade.hpp")
    assert '#include "nt_boxhits.hpp"' in hpp
    for reused in ("box_face<N>(", "box_line_pair(", "box_line_record<N, false>(", "NT_BOXLINES_PITCH", "box_may_hit("):
        assert reused in hpp, reused
    var = sup.source("nt_var.hip")
    body = sup.function_body(var, "int nt_launch_box_shade(")
    assert "nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n" in body and "box_hits_var" in body and "box_shaded_var" in body
    # the plain launchers launch what they launched
    for head in ("int nt_launch_box(", "int nt_launch_composite(", "int nt_launch_box_faces("):
        b = sup.function_body(var, head)
        assert "box_shade" not in b and "nt_box_shade" not in b, head
    for name in ("nt_box.hpp", "nt_composite.hpp", "nt_inst_box.hip", "nt_boxhits.hpp", "nt_inst_boxhits.hip"):
        assert "boxshade" not in sup.source(name) and "box_shade" not in sup.source(name), name
    # the routes obey NTRACER_FORCE_VAR and nothing of their own
    for name in ("nt_boxshade.hpp", "nt_inst_boxshade.hip"):
        assert "getenv" not in sup.source(name) and "asm" not in sup.source(name), name
    api = sup.source("nt_api.cpp")
    assert api.count("getenv(") == 12
    enq = sup.function_body(api, "int enqueue_box_shading(")
    assert "sw.force_var" in enq and "ss_scratch_mb" in enq and "nt_launch_box_shade(" in enq and "getenv" not in enq
    # the cue's arguments are validated by the one function nt_scene_set_depth_cue asks
    assert "cue_validate(" in sup.function_body(api, "int nt_scene_set_depth_cue(") and "cue_validate(" in sup.function_body(api, "int nt_scene_set_box_shading(")
