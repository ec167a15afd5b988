"""The parallel projection (nt_scene_set_parallel; Scene.set_parallel_projection, Scene.parallel_rays), the part that needs
no GPU: the ABI symbols and the header's text, parallel_rays against a plain numpy-fp32 restatement of the formula, set / get /
off, invalid values, the lock, the exclusion with a lens in both directions, the refusals -- all answered before any device is
touched -- and the kernels of the new launchers pinned to the cases that reach them, as tests/test_lens_host.py does it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallel_cases as pc
import ray_query_cases as rq
import support as sup
import ntracer_amd
from ntracer_amd import Channel, ImageFormat, Lens, _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nt_scene_set_parallel", "nt_scene_get_parallel")
f32 = np.float32
RGBX8 = [Channel(8, 1, 0, 0), Channel(8, 0, 1, 0), Channel(8, 0, 0, 1), Channel(8, 0, 0, 0)]


def test_the_header_declares_and_the_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "ntracer_hip.h")) as f:
        header = f.read()
    raw = C.CDLL(_lib.LIB_PATH)
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in declared, name
    # the semantics are in the header: the formula, line for line, and what is refused
    for text in ("k  = half_width / half_w", "sx = k * ((float)x - half_w)", "sy = k * ((float)y - half_h)",
                 "o'[j] = (origin[j] + right[j] * sx) - up[j] * sy", "v = forward", "d = v / |v|", "half_w = float(width) / 2",
                 "exclude each other", "NT_E_LOCKED"):
        assert text in header, text
    for cls in (tracern.BoxScene, tracern.CompositeScene):
        assert callable(cls.set_parallel_projection) and callable(cls.parallel_rays) and isinstance(cls.parallel_projection, property)


def test_every_parallel_launch_is_reached_by_a_case():
    hpp, var = sup.source("nt_parallel.hpp"), sup.source("nt_var.hip")
    packet = sup.launches_through(hpp, "int launch_parallel_fixed(")          # (no numerators: not through the shared chunk head)
    helper = sup.launches(sup.function_body(var, "int nt_launch_parallel_expand("))
    assert packet == {"parallel_packet<N,32,true>", "parallel_packet<N,32,false>",
                      "parallel_shade<N,false,false>", "parallel_shade<N,true,true>", "parallel_shade<N,true,false>"}, sorted(packet)
    assert helper == {"parallel_expand"}, sorted(helper)
    assert not sup.launches(sup.function_body(var, "int nt_launch_parallel("))       # the dispatcher launches through the fixed-n units alone
    reached = set()
    for case in pc.CASES:
        reached |= set(pc.route(case))
    missing = (packet | helper) - reached
    assert not missing, sorted(missing)
    # the ray route ends in nt_launch_rays: every kernel it can launch is reached under the projection as well
    rays = (sup.launches(sup.function_body(sup.source("nt_rays.hpp"), "int launch_rays_fixed(")) | sup.launches(sup.function_body(sup.source("nt_rays.hpp"), "int launch_rays_box_fixed(")) |
            sup.launches(sup.function_body(var, "int nt_launch_rays(")))
    assert len(rays) >= 10 and rays <= reached, sorted(rays - reached)
    # the new kernels stay out of the render and lens launchers
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_lens.hpp", "int launch_lens_fixed("),
                      ("nt_var.hip", "int nt_launch_composite("), ("nt_var.hip", "int nt_launch_box("), ("nt_var.hip", "int nt_launch_rays(")):
        assert not any("parallel" in k for k in sup.launches(sup.function_body(sup.source(src), head)))
    assert "getenv" not in hpp
    # what enqueue_parallel sends to the packet walk is what enqueue_lens sends to its own: pinned text of the conditions, which
    # are composite_route's -- enqueue_parallel asks it and keeps no terms of its own
    rule, api = sup.function_body(sup.source("nt_api.cpp"), "CompositeRoute composite_route("), sup.function_body(sup.source("nt_api.cpp"), "int enqueue_parallel(")
    assert "r.packet_walk = !r.faithful && !r.var && sw.composite_kernel == 0 && std::max(s->depth + 1, 2) <= 32;" in rule
    assert "r.var = s->n > NT_MAX_FIXED_DIM || sw.force_var;" in rule
    assert "s->composite && composite_route(s, sw).packet_walk" in api and "all_opaque" not in api
    assert "rj.shared_origin = 0;" in api


def test_parallel_rays_is_the_formula_bit_for_bit():
    for name, (w, h), hw in (("cell600_n4", (37, 29), None), ("box6", (9, 17), 1.5), ("feature11_n11", (1, 1), 0.37), ("box25", (64, 3), 2.5)):
        o, q = pc.camera(name)
        n = len(o)
        hw = pc.half_width(name) if hw is None else hw
        sc = tracern.BoxScene(n)                          # (the rays depend on the camera and the setting alone)
        sc.set_parallel_projection(hw)
        org, fwd = sc.parallel_rays(w, h, pc.lc.camera_of(o, q))
        want_o, want_f = pc.parallel_rays(o, q, w, h, f32(hw))
        assert org.dtype == f32 and org.shape == (h * w, n) and fwd.dtype == f32 and fwd.shape == (n,)
        assert np.array_equal(org.view(np.uint32), want_o.view(np.uint32)), name
        assert np.array_equal(fwd.view(np.uint32), q[2].view(np.uint32)) and np.array_equal(want_f, fwd)
        # ... and the scene's own camera when none is given
        sc._set_camera_arrays(o, q)
        again, _ = sc.parallel_rays(w, h)
        assert np.array_equal(again.view(np.uint32), want_o.view(np.uint32))
    # the image spans 2 * half_width across: pixel x = w / 2 of an even width starts on the camera's axis
    sc = tracern.BoxScene(3)
    sc.set_parallel_projection(2.0)
    org, fwd = sc.parallel_rays(4, 2)
    assert np.array_equal(org[1 * 4 + 2], np.zeros(3, f32)) and np.array_equal(org[1 * 4 + 0], np.array([-2, 0, 0], f32))
    assert np.array_equal(org[0 * 4 + 2], np.array([0, 1, 0], f32)) and np.array_equal(fwd, np.array([0, 0, 1], f32))
    sc.set_parallel_projection(None)
    with pytest.raises(ValueError, match="no parallel projection"):
        sc.parallel_rays(4, 2)


def test_set_get_off_and_invalid_values():
    L = _lib.lib()
    for sc in (tracern.BoxScene(5), tracern.CompositeScene.from_flat(*rq.scene("cell600_n4")[1:])):
        assert sc.parallel_projection is None and L.nt_scene_get_parallel(sc._handle) == 0.0
        sc.set_parallel_projection(1.25)
        assert sc.parallel_projection == 1.25 and L.nt_scene_get_parallel(sc._handle) == 1.25
        sc.set_parallel_projection(0.1)
        assert sc.parallel_projection == float(f32(0.1))
        for bad in (-1.0, float("nan"), float("inf"), -float("inf"), -1e-30):
            assert L.nt_scene_set_parallel(sc._handle, bad) == _lib.NT_E_INVALID
            with pytest.raises(ValueError, match="half_width"):
                sc.set_parallel_projection(bad)
            assert sc.parallel_projection == float(f32(0.1))              # the state is unchanged
        for bad in ("1", True, [1.0]):
            with pytest.raises(ValueError):
                sc.set_parallel_projection(bad)
        sc.set_parallel_projection(0)
        assert sc.parallel_projection is None
        sc.set_parallel_projection(3)
        sc.set_parallel_projection(None)
        assert sc.parallel_projection is None and L.nt_scene_get_parallel(sc._handle) == 0.0
    assert L.nt_scene_set_parallel(None, 1.0) == _lib.NT_E_INVALID
    assert L.nt_scene_get_parallel(None) == 0.0


def test_the_lock_rule():
    L = _lib.lib()
    sc = tracern.BoxScene(5)
    assert L.nt_scene_lock(sc._handle) == _lib.NT_OK
    with pytest.raises(ntracer_amd.LockedError):
        sc.set_parallel_projection(1.0)
    assert L.nt_scene_set_parallel(sc._handle, 1.0) == _lib.NT_E_LOCKED
    assert sc.parallel_projection is None
    with pytest.raises(ntracer_amd.LockedError):
        sc.set_camera(tracern.Camera(5))                               # (the rule it shares)
    assert L.nt_scene_unlock(sc._handle) == _lib.NT_OK
    sc.set_parallel_projection(1.0)
    assert sc.parallel_projection == 1.0


def test_a_lens_and_the_projection_exclude_each_other():
    L = _lib.lib()
    sc = tracern.BoxScene(4)
    ln = Lens.pinhole(8, 5, 0.8)
    sc.set_lens(ln)
    assert L.nt_scene_set_parallel(sc._handle, 1.0) == _lib.NT_E_INVALID
    assert "lens" in _lib.last_error() and "parallel" in _lib.last_error()
    with pytest.raises(ValueError, match="lens"):
        sc.set_parallel_projection(1.0)
    assert sc.parallel_projection is None and sc.lens is ln           # unchanged
    sc.set_parallel_projection(None)                                   # taking it off is always allowed
    sc.set_lens(None)
    sc.set_parallel_projection(1.0)
    assert L.nt_scene_set_lens(sc._handle, ln._handle) == _lib.NT_E_INVALID
    assert "lens" in _lib.last_error() and "parallel" in _lib.last_error()
    with pytest.raises(ValueError, match="parallel"):
        sc.set_lens(ln)
    assert sc.parallel_projection == 1.0 and sc.lens is None and not L.nt_scene_get_lens(sc._handle)
    sc.set_lens(None)                                                  # taking it off is always allowed
    assert sc.parallel_projection == 1.0
    sc.set_parallel_projection(None)
    sc.set_lens(ln)
    assert sc.lens is ln


@pytest.mark.parametrize("kind", ["composite", "box"])
def test_what_the_projection_refuses_is_refused_before_a_device_is_touched(kind):
    """every refusal below answers on a machine without a GPU, where anything that reached for a device would say NT_E_DEVICE"""
    L = _lib.lib()
    if kind == "composite":
        g, n, flat = rq.scene("cell600_n4")
        sc = tracern.CompositeScene.from_flat(n, flat)
    else:
        n = 6
        sc = tracern.BoxScene(n)
    w, h = 8, 5
    fmt = ImageFormat(w, h, RGBX8)
    fst = fmt._as_struct()
    dest = np.full(w * h * 4, 0xab, np.uint8)
    sc.set_parallel_projection(1.5)

    def calls(opts=None):
        o = C.byref(opts) if opts is not None else None
        cams = np.zeros((1, n), f32), np.eye(n, dtype=f32)[None].copy()
        return [L.nt_render(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_device(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_frames_device(sc._handle, dest.ctypes.data, dest.nbytes, 1, cams[0].ctypes.data_as(_lib.f32p),
                                          cams[1].ctypes.data_as(_lib.f32p), C.byref(fst), o, None)]
    sc.set_supersampling(2)
    for r in calls():
        assert r == _lib.NT_E_UNSUPPORTED and "supersampling" in _lib.last_error() and "parallel" in _lib.last_error()
    sc.set_supersampling(1)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world, opts.band_rank = -1, 2, 1
    for r in calls(opts):
        assert r == _lib.NT_E_UNSUPPORTED and "band" in _lib.last_error()
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    for r in calls(opts):
        assert r == _lib.NT_E_UNSUPPORTED and "collect_stats" in _lib.last_error()
    with pytest.raises(NotImplementedError, match="parallel"):
        sc.calculate_color(1, 1, w, h)
    with pytest.raises(NotImplementedError, match="parallel"):
        sc.colors_at([1], [1], w, h)
    if kind == "composite":
        with pytest.raises(NotImplementedError, match="parallel"):
            sc.primary_hits(w, h)
    assert (dest == 0xab).all()                                        # nothing was drawn
    # with the projection off the same calls get past the checks: on a machine without a GPU they end at the device, not before.
    # (Only there: `dest` is host memory, which the device forms must not be let loose on where a device exists.)
    sc.set_parallel_projection(None)
    if L.nt_device_count() == 0:
        sc.set_supersampling(2)
        for r in calls():
            assert r == _lib.NT_E_DEVICE
        sc.set_supersampling(1)
        for o_ in (opts, None):
            for r in calls(o_):
                assert r == _lib.NT_E_DEVICE


@pytest.mark.parametrize("case", pc.SCENES, ids=pc.case_id)
def test_no_case_passes_on_background(case):
    pc.check_floors(case)


def test_the_floors_the_cases_were_chosen_by():
    """the oracle's own counts at 37 x 29, out of 1 073 pixels: the table the cases were accepted with"""
    got = {name: pc.counts(name) for name in ("cell600_n4", "simplex10_n10", "feature5_n5", "feature11_n11", "box6", "box25")}
    assert got == {"cell600_n4": (872, 0), "simplex10_n10": (169, 0), "feature5_n5": (140, 66), "feature11_n11": (71, 43),
                   "box6": (576, 0), "box25": (576, 0)}, got
    assert pc.counts("box6", hw=2.5)[0] == 196 and pc.counts("box25", hw=2.5)[0] == 196
    # rays that start inside the scene box
    o, q = pc.centre_camera("cell600_n4")
    org, _ = pc.parallel_rays(o, q, pc.W, pc.H, pc.half_width("cell600_n4"))
    assert pc.counts("cell600_n4", True)[0] == 872 and pc.inside_box("cell600_n4", org) == 1044
