"""Colours of caller-supplied rays (ray_colors / render_rays), the part that needs no GPU: the four ABI symbols, their
validation -- which answers before any device is touched -- through the C ABI and as ValueError from Python, the method the
GPU tests get their expected colours by (ray_color_cases.CentrePixel) pinned against the oracle's colors_at of real cameras,
and the kernel routes of nt_launch_rays pinned to the C++ that picks them the way tests/test_composite_routes.py pins the
render routes: every hipLaunchKernelGGL of nt_launch_rays (nt_var.hip) and of the fixed-n launchers it calls (nt_rays.hpp) is
reached by a case of ray_color_cases, which tests/test_ray_colors_gpu.py runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
from ntracer_amd import Channel, ImageFormat, _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nt_ray_colors", "nt_ray_colors_device", "nt_render_rays", "nt_render_rays_device")


def test_every_ray_launch_is_reached_by_a_case():
    hpp, var = sup.source("nt_rays.hpp"), sup.source("nt_var.hip")
    launched = (sup.launches(sup.function_body(hpp, "int launch_rays_fixed(")) | sup.launches(sup.function_body(hpp, "int launch_rays_box_fixed(")) |
                sup.launches(sup.function_body(var, "int nt_launch_rays(")))
    assert len(launched) >= 10, sorted(launched)             # the scan still finds the launches
    reached = {rc.route(case) for case in rc.CASES} | {rc.box_route(n) for n in rc.BOX_DIMS}
    assert reached == launched, ("launched without a case: %s; routes nothing launches: %s"
                                 % (sorted(launched - reached), sorted(reached - launched)))
    # the module's docstring names the instantiation of every case
    for kernel in launched:
        assert kernel in rc.__doc__, kernel
    # the launches stay out of the render launchers, whose every launch wants a row of the render matrix
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_var.hip", "int nt_launch_box(")):
        assert not any(k.startswith("rays_") for k in sup.launches(sup.function_body(sup.source(src), head)))
    # and route on the switches read_switches already reads: no getenv of their own
    assert "getenv" not in hpp and "getenv" not in sup.function_body(var, "int nt_launch_rays(")


def test_the_header_declares_and_the_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "ntracer_hip.h")) as f:
        header = f.read()
    raw = C.CDLL(_lib.LIB_PATH)
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(nt_scene_t \*s," % name, header), name
        assert hasattr(raw, name), name
        assert name in declared, name
    assert re.search(r"typedef struct \{[^}]*int32_t count;[^}]*const float \*origins;[^}]*const float \*directions;[^}]*"
                     r"int32_t shared_origin;\s*\} nt_rays;", header)
    assert C.sizeof(_lib.NtRays) == 32 and _lib.NtRays.shared_origin.offset == 24
    # the entry points' comment carries the semantics, the unspecified colour of a bad ray on the device among them
    assert "such a ray's colour is unspecified" in header


RGBX8 = [Channel(8, 1, 0, 0), Channel(8, 0, 1, 0), Channel(8, 0, 0, 1), Channel(8, 0, 0, 0)]


def _args(n, count=6, **kw):
    o = np.zeros((max(count, 1), n), np.float32)
    d = np.ones((max(count, 1), n), np.float32)
    rays = _lib.NtRays()
    rays.count, rays.origins, rays.directions, rays.shared_origin = count, o.ctypes.data, d.ctypes.data, 0
    for k, v in kw.items():
        setattr(rays, k, v)
    return rays, (o, d)


@pytest.mark.parametrize("kind", ["composite", "box"])
def test_the_abi_validates_before_it_touches_a_device(kind):
    L = _lib.lib()
    if kind == "composite":
        g, n, flat = rq.scene("cell600_n4")
        sc = tracern.CompositeScene.from_flat(n, flat)
    else:
        n = 4
        sc = tracern.BoxScene(n)
    INVALID, OK = _lib.NT_E_INVALID, _lib.NT_OK
    rgb = np.zeros((6, 3), np.float32)
    dest = np.zeros(3 * 2 * 4, np.uint8)
    fmt = ImageFormat(3, 2, RGBX8)._as_struct()
    colour_forms = [lambda s, r, out: L.nt_ray_colors(s, r, out, -1), lambda s, r, out: L.nt_ray_colors_device(s, r, out, None, None)]
    image_forms = [lambda s, r, out, f=fmt, ln=dest.nbytes: L.nt_render_rays(s, out, ln, C.byref(f) if f is not None else None, r, -1),
                   lambda s, r, out, f=fmt, ln=dest.nbytes: L.nt_render_rays_device(s, out, ln, C.byref(f) if f is not None else None, r, None, None)]
    for call, out in [(c, rgb.ctypes.data) for c in colour_forms] + [(c, dest.ctypes.data) for c in image_forms]:
        rays, keep = _args(n)
        assert call(None, C.byref(rays), out) == INVALID
        assert call(sc._handle, None, out) == INVALID
        assert call(sc._handle, C.byref(rays), None) == INVALID
        for bad in (dict(origins=None), dict(directions=None), dict(count=-1)):
            rays, keep = _args(n, **bad)
            assert call(sc._handle, C.byref(rays), out) == INVALID, bad
            assert _lib.last_error()
    # count == 0: nothing to do, no device is asked for (the image forms want a count that fills the format, so 0 never does)
    for call in colour_forms:
        rays, keep = _args(n, count=0)
        assert call(sc._handle, C.byref(rays), rgb.ctypes.data) == OK
    # the image forms: a count that does not match the format, a buffer too small, an invalid format with nt_render's message
    for call in image_forms:
        rays, keep = _args(n, count=5)
        assert call(sc._handle, C.byref(rays), dest.ctypes.data) == INVALID
        assert "do not fill an image of 3 x 2" in _lib.last_error()
        rays, keep = _args(n)
        assert call(sc._handle, C.byref(rays), dest.ctypes.data, ln=dest.nbytes - 1) == INVALID
        assert "too small" in _lib.last_error()
        assert call(sc._handle, C.byref(rays), dest.ctypes.data, f=None) == INVALID
        for field, value in (("pitch", 11), ("pitch", -1), ("width", 0), ("height", -2), ("nchannels", -1)):
            f = ImageFormat(3, 2, RGBX8)._as_struct()
            setattr(f, field, value)
            assert call(sc._handle, C.byref(rays), dest.ctypes.data, f=f) == INVALID
            message = _lib.last_error()
            assert L.nt_render(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(f), None, None) == INVALID
            assert message == _lib.last_error() and message
    # the host forms look at the rays: the first bad one is named
    for call, out in ((colour_forms[0], rgb.ctypes.data), (image_forms[0], dest.ctypes.data)):
        for value, what in ((np.nan, "non-finite"), (np.inf, "non-finite"), (-np.inf, "non-finite")):
            rays, (o, d) = _args(n)
            d[4, 1] = value
            d[5, 0] = value
            assert call(sc._handle, C.byref(rays), out) == INVALID
            assert "ray 4" in _lib.last_error() and what in _lib.last_error()
            rays, (o, d) = _args(n)
            o[3, n - 1] = value
            assert call(sc._handle, C.byref(rays), out) == INVALID
            assert "ray 3" in _lib.last_error() and what in _lib.last_error()
        rays, (o, d) = _args(n)
        d[2] = 0.0
        d[5] = -0.0
        assert call(sc._handle, C.byref(rays), out) == INVALID
        assert "ray 2" in _lib.last_error() and "all-zero direction" in _lib.last_error()
        # a shared origin is [n]: what lies behind it is not looked at
        rays, (o, d) = _args(n, shared_origin=1)
        o[0, 0] = np.nan
        assert call(sc._handle, C.byref(rays), out) == INVALID
        assert "ray 0" in _lib.last_error()
    # the options of the device forms: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        rays, keep = _args(n)
        assert L.nt_ray_colors_device(sc._handle, C.byref(rays), rgb.ctypes.data, C.byref(opts), None) == INVALID, field
        assert L.nt_render_rays_device(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fmt), C.byref(rays), C.byref(opts), None) == INVALID, field


@pytest.mark.parametrize("kind", ["composite", "box"])
def test_python_refuses_what_does_not_fit_and_answers_an_empty_batch(kind):
    if kind == "composite":
        g, n, flat = rq.scene("cell600_n4")
        sc = tracern.CompositeScene.from_flat(n, flat)
    else:
        n = 4
        sc = tracern.BoxScene(n)
    ones = np.ones((3, n), np.float32)
    for o, d in ((ones, np.ones((3, n + 1), np.float32)), (np.ones((2, n), np.float32), ones), (np.ones(n + 1, np.float32), ones),
                 (ones, np.ones(n, np.float32)), (np.ones((3, n + 1), np.float32), np.ones((3, n + 1), np.float32))):
        with pytest.raises(ValueError):
            sc.ray_colors(o, d)
    with pytest.raises(ValueError, match="out must be"):
        sc.ray_colors(ones, ones, out=np.zeros((3, 3), np.float64))
    bad = ones.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="ray 1 has a non-finite component"):
        sc.ray_colors(ones, bad)
    with pytest.raises(ValueError, match="ray 1 has a non-finite component"):
        sc.ray_colors(bad, ones)
    with pytest.raises(ValueError, match="ray 2 has an all-zero direction"):
        sc.ray_colors(np.zeros(n, np.float32), np.array([[1] * n, [0, 1] + [0] * (n - 2), [0] * n], np.float32))
    empty = sc.ray_colors(np.zeros((0, n), np.float32), np.zeros((0, n), np.float32))
    assert empty.shape == (0, 3) and empty.dtype == np.float32
    assert sc.ray_colors(np.zeros(n, np.float32), np.zeros((0, n), np.float32)).shape == (0, 3)
    # render_rays: the format and the buffer are checked as BlockingRenderer.render checks them
    fmt = ImageFormat(3, 1, RGBX8)
    with pytest.raises(TypeError):
        sc.render_rays(bytearray(12), "RGBX8", ones, ones)
    with pytest.raises(ValueError, match="too small"):
        sc.render_rays(bytearray(11), fmt, ones, ones)
    with pytest.raises(ValueError, match="do not fill"):
        sc.render_rays(bytearray(16), ImageFormat(2, 2, RGBX8), ones, ones)
    with pytest.raises(BufferError):
        sc.render_rays(bytes(12), fmt, ones, ones)
    with pytest.raises(ValueError, match="ray 1 has a non-finite component"):
        sc.render_rays(bytearray(12), fmt, ones, bad)


def test_the_centre_pixel_method_reproduces_colors_at_bit_for_bit():
    """what the GPU tests take as the oracle's colour of a ray is the oracle's colour of the pixel the ray belongs to: 500
    pixels of a feature5_n5 frame with transparent hits and of a BoxScene(6) view, through the real camera and ray by ray"""
    g, n, flat = rq.scene("feature5_n5")
    params = fx.params_of(g)
    w, h, fov = int(g["width"]), int(g["height"]), float(g["fov"])
    f = int(g["frames"][1])
    pick = np.linspace(0, len(g["xs"]) - 1, 500).astype(int)
    xs, ys = np.asarray(g["xs"])[pick], np.asarray(g["ys"])[pick]
    real = ob.OracleScene(n, g["origins"][f], g["axes"][f], fov, flat=flat, params=params).colors_at(xs, ys, w, h)
    v = rc.camera_rays(g["axes"][f], xs, ys, w, h, fov)
    by_ray = rc.CentrePixel(n, flat, params).colors(np.asarray(g["origins"][f], np.float32), v)
    assert np.array_equal(real.view(np.uint32), by_ray.view(np.uint32))
    assert len(np.unique(real, axis=0)) > 100                     # (a frame with something in it)
    # ... and with one origin a ray, scaled directions: the source normalises
    assert np.array_equal(rc.CentrePixel(n, flat, params).colors(np.repeat(np.asarray(g["origins"][f], np.float32)[None], 500, axis=0), v).view(np.uint32),
                          real.view(np.uint32))

    gb = fx.load("box_n6_1920x1080")
    o, q = gb["origins"][17], gb["axes"][17]
    w, h = 640, 480
    xs, ys = np.meshgrid(7 + 25 * np.arange(25), 11 + 23 * np.arange(20))
    xs, ys = xs.ravel(), ys.ravel()
    real = ob.OracleScene(6, o, q).colors_at(xs, ys, w, h)
    by_ray = rc.CentrePixel(6).colors(np.asarray(o, np.float32), rc.camera_rays(q, xs, ys, w, h))
    assert np.array_equal(real.view(np.uint32), by_ray.view(np.uint32))
    assert (real[:, 0] != real[:, 1]).sum() >= 50                  # rays that hit the cube
