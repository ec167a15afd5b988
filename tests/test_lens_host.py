"""Lens tables (nt_lens_*, nt_scene_set_lens; tracern.Lens, Scene.set_lens), the part that needs no GPU: the ABI symbols, the
constructors' tables against their float64 formulas where those are delicate, the library-built pinhole against the ray
source's own expressions, the method the GPU tests get their expected colours by pinned against the oracle's colors_at of
real cameras, the errors and refusals -- all answered before any device is touched -- and the kernel routes of the lens
dispatchers pinned to the C++ that picks them, the way tests/test_composite_routes.py pins the render routes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fixtures as fx
import lens_cases as lc
import oracle_binding as ob
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
import ntracer_amd
from ntracer_amd import Channel, ImageFormat, Lens, _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")
SYMBOLS = ("nt_lens_create", "nt_lens_create_pinhole", "nt_lens_destroy", "nt_lens_width", "nt_lens_height", "nt_lens_coeffs",
           "nt_scene_set_lens", "nt_scene_get_lens")
f32 = np.float32
RGBX8 = [Channel(8, 1, 0, 0), Channel(8, 0, 1, 0), Channel(8, 0, 0, 1), Channel(8, 0, 0, 0)]


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, head):
    start = src.index(head)
    return src[start:re.compile(r"\n\}(\n|$)").search(src, start).start()]


def _launches(body):
    """the regular expression of tests/test_composite_routes.py"""
    names = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*(?:\s*<[^<>]*>)?)", body)
    return {re.sub(r"\s+", "", n) for n in names}


def test_the_header_declares_and_the_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "ntracer_hip.h")) as f:
        header = f.read()
    raw = C.CDLL(_lib.LIB_PATH)
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in declared, name
    assert "typedef struct nt_lens nt_lens_t;" in header
    # the semantics are in the header: the formula, the masked pixel, what is refused
    for text in ("(forward[j] * sz + right[j] * sx) - up[j] * sy", "masked pixel", "NT_E_UNSUPPORTED"):
        assert text in header, text
    assert ntracer_amd.Lens is tracern.Lens and "Lens" in ntracer_amd.__all__
    for cls in (tracern.BoxScene, tracern.CompositeScene):
        assert callable(cls.set_lens) and isinstance(cls.lens, property)


def test_every_lens_launch_is_reached_by_a_case():
    hpp, var = _read("nt_lens.hpp"), _read("nt_var.hip")
    packet = sup.launches_through(hpp, "int launch_lens_fixed(")      # (with the numerators of the shared chunk head)
    helpers = _launches(_body(var, "int nt_launch_lens_expand(")) | _launches(_body(var, "int nt_launch_lens_mask("))
    assert packet == {"packet_numerators<N>", "composite_packet<N,32,false,true,true,true>", "composite_packet<N,32,false,false,true,true>",
                      "lens_shade<N,false,false>", "lens_shade<N,true,true>", "lens_shade<N,true,false>"}, sorted(packet)
    assert helpers == {"lens_expand", "lens_mask_fill"}, sorted(helpers)
    assert not _launches(_body(var, "int nt_launch_lens("))           # the dispatcher launches through the fixed-n units alone
    reached = set()
    for case in lc.ORACLE_CASES:
        reached |= set(lc.route(case))
        if lc.route(case)[0] == "lens_expand" and lc.lens(case).masked.any():
            reached.add("lens_mask_fill")
        if lc.route(case)[0].startswith("composite_packet"):
            reached.add("packet_numerators<N>")                        # (NTRACER_NUMERATORS is on unless switched off)
    missing = (packet | helpers) - reached
    assert not missing, sorted(missing)
    # the ray route ends in nt_launch_rays: every kernel it can launch is reached through a lens as well
    rays = (_launches(_body(_read("nt_rays.hpp"), "int launch_rays_fixed(")) | _launches(_body(_read("nt_rays.hpp"), "int launch_rays_box_fixed(")) |
            _launches(_body(var, "int nt_launch_rays(")))
    assert len(rays) >= 10 and rays <= reached, sorted(rays - reached)
    # the lens kernels stay out of the render launchers, whose every launch wants a row of the render matrix
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("), ("nt_var.hip", "int nt_launch_box(")):
        assert not any("lens" in k or k.endswith(",true,true>") and k.startswith("composite_packet") for k in _launches(_body(_read(src), head)))
    assert "getenv" not in hpp
    # what enqueue_lens sends to the packet walk is what launch_composite_fixed would: pinned text of the conditions, which are
    # composite_route's -- enqueue_lens asks it and keeps no terms of its own
    rule, api = _body(_read("nt_api.cpp"), "CompositeRoute composite_route("), _body(_read("nt_api.cpp"), "int enqueue_lens(")
    assert "r.packet_walk = !r.faithful && !r.var && sw.composite_kernel == 0 && std::max(s->depth + 1, 2) <= 32;" in rule
    assert "r.var = s->n > NT_MAX_FIXED_DIM || sw.force_var;" in rule
    assert "s->composite && composite_route(s, sw).packet_walk" in api and "all_opaque" not in api


def test_the_pinhole_table_is_the_ray_sources_own_arithmetic():
    for w, h, fov in ((37, 29, 0.8), (64, 48, 1.3), (1, 1, 0.8)):
        c = Lens.pinhole(w, h, fov).coeffs
        assert c.shape == (h, w, 3) and c.dtype == f32
        fov_i = rc.fov_inverse(fov, w)
        sx = (fov_i * (np.arange(w).astype(f32) - f32(w) / f32(2))).astype(f32)
        sy = (fov_i * (np.arange(h).astype(f32) - f32(h) / f32(2))).astype(f32)
        assert np.array_equal(c[:, :, 0].view(np.uint32), np.broadcast_to(sx[None, :], (h, w)).view(np.uint32))
        assert np.array_equal(c[:, :, 1].view(np.uint32), np.broadcast_to(sy[:, None], (h, w)).copy().view(np.uint32))
        assert (c[:, :, 2] == 1.0).all()
    # ... so its directions are the camera's own rays, bit for bit
    g = fx.load("box_n6_1920x1080")
    q = np.asarray(g["axes"][17], f32)
    xs, ys = np.meshgrid(np.arange(37), np.arange(29))
    v = Lens.pinhole(37, 29, 0.8).directions(lc.camera_of(np.zeros(6, f32), q))
    assert np.array_equal(v.view(np.uint32), rc.camera_rays(q, xs.ravel(), ys.ravel(), 37, 29, 0.8).view(np.uint32))


def _close(got, want):
    want = np.asarray(want, np.float64)
    assert np.array_equal(np.asarray(got, f32).view(np.uint32), want.astype(f32).view(np.uint32)), (got, want)


def test_the_constructors_tables_at_the_delicate_pixels():
    w, h = 37, 29
    # ---- fisheye, equidistant: theta = r (fov / 2) / (W / 2)
    fe = Lens.fisheye(w, h, 3.0).coeffs

    def fisheye(x, y, fov=3.0, ww=w, hh=h):
        u, v = x - ww / 2.0, y - hh / 2.0
        r = math.hypot(u, v)
        if r == 0.0:
            return (0.0, 0.0, 1.0)
        th = r * (fov / 2.0) / (ww / 2.0)
        if th > math.pi:
            return (0.0, 0.0, 0.0)
        return (math.sin(th) * u / r, math.sin(th) * v / r, math.cos(th))
    for x, y in ((0, 0), (w - 1, h - 1), (w - 1, 0), (18, 14), (19, 15), (0, 14)):
        _close(fe[y, x], fisheye(x, y))
    assert not Lens.fisheye(w, h, 3.0).masked.any()                   # (1.9 rad at the corner)
    even = Lens.fisheye(36, 28, 3.0)                                  # an even size has a pixel at r = 0
    _close(even.coeffs[14, 18], (0.0, 0.0, 1.0))
    assert not even.masked[14, 18]
    full = Lens.fisheye(w, h, 2.0 * math.pi)                          # corners beyond pi: masked, exactly zero
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        assert fisheye(x, y, 2.0 * math.pi) == (0.0, 0.0, 0.0)
        assert full.masked[y, x] and (full.coeffs[y, x].view(np.uint32) == 0).all()
    assert full.masked[14, 0]                                         # r = 18.507 at (0, 14): a hair beyond pi
    _close(full.coeffs[14, 1], fisheye(1, 14, 2.0 * math.pi))         # the last pixel inside: looks almost straight back
    assert not full.masked[14, 1] and full.coeffs[14, 1, 2] < -0.98
    assert int(full.masked.sum()) == sum(fisheye(x, y, 2.0 * math.pi) == (0.0, 0.0, 0.0) for y in range(h) for x in range(w))
    for bad in (0.0, -1.0, 6.3):
        with pytest.raises(ValueError):
            Lens.fisheye(w, h, bad)
    # ---- equirectangular: lambda = u hfov / W, phi = v vfov / H
    ww, hh = 36, 18
    eq = Lens.equirectangular(ww, hh).coeffs

    def equirect(x, y, hfov=2.0 * math.pi, vfov=math.pi):
        lam, phi = (x - ww / 2.0) * hfov / ww, (y - hh / 2.0) * vfov / hh
        return (math.sin(lam) * math.cos(phi), math.sin(phi), math.cos(lam) * math.cos(phi))
    for x, y in ((0, 9), (0, 0), (ww - 1, hh - 1), (18, 9), (18, 0), (35, 9), (9, 9)):
        _close(eq[y, x], equirect(x, y))
    assert eq[9, 0, 2] == -1.0 and abs(eq[9, 0, 0]) < 1e-15            # lambda = -pi, the seam: straight back, not masked
    assert not Lens.equirectangular(ww, hh).masked.any()              # (the pole row is sin(phi) = -1)
    assert eq[0, 18, 1] == -1.0 and eq[9, 18, 2] == 1.0
    half = Lens.equirectangular(ww, hh, math.pi, math.pi / 2).coeffs
    _close(half[3, 0], equirect(0, 3, math.pi, math.pi / 2))
    # ---- cylindrical: (sin lambda, v hfov / W, cos lambda)
    cy = Lens.cylindrical(w, h, 3.0).coeffs
    for x, y in ((0, 0), (w - 1, h - 1), (18, 14), (5, 28)):
        lam = (x - w / 2.0) * 3.0 / w
        _close(cy[y, x], (math.sin(lam), (y - h / 2.0) * 3.0 / w, math.cos(lam)))
    # ---- a table of the caller's own, NaN and zero entries masked
    t = np.ones((2, 3, 3), f32)
    t[0, 1] = 0.0
    t[1, 2, 1] = np.nan
    ln = Lens(3, 2, t)
    assert (ln.width, ln.height) == (3, 2)
    assert np.array_equal(ln.coeffs.view(np.uint32), t.view(np.uint32))
    assert np.array_equal(ln.masked, [[False, True, False], [False, False, True]])
    d = ln.directions(tracern.Camera(5))
    assert d.shape == (6, 5) and d.dtype == f32 and not d[1].any() and not d[5].any()
    assert np.array_equal(d[0], np.array([1, -1, 1, 0, 0], f32))      # (forward * sz + right * sx) - up * sy


def test_the_expectation_method_reproduces_colors_at_through_the_pinhole_lens():
    """what the GPU tests take as the oracle's colour of a lens pixel: CentrePixel of Lens.directions.  Through the pinhole lens
    that is the oracle's colors_at of the real camera, bit for bit -- a composite golden with transparent hits and BoxScene(6)"""
    w, h = lc.W, lc.H
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    xs, ys = xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)
    ln = Lens.pinhole(w, h, lc.FOV)
    g, n, flat = rq.scene("feature5_n5")
    params = fx.params_of(g)
    f = int(g["frames"][1])
    o, q = np.asarray(g["origins"][f], f32), np.asarray(g["axes"][f], f32)
    real = ob.OracleScene(n, o, q, lc.FOV, flat=flat, params=params).colors_at(xs, ys, w, h)
    by_lens = rc.CentrePixel(n, flat, params).colors(o, ln.directions(lc.camera_of(o, q)))
    assert np.array_equal(real.view(np.uint32), by_lens.view(np.uint32))
    assert len(np.unique(real, axis=0)) > 100
    gb = fx.load("box_n6_1920x1080")
    o, q = np.asarray(gb["origins"][17], f32), np.asarray(gb["axes"][17], f32)
    real = ob.OracleScene(6, o, q, lc.FOV).colors_at(xs, ys, w, h)
    by_lens = rc.CentrePixel(6).colors(o, ln.directions(lc.camera_of(o, q)))
    assert np.array_equal(real.view(np.uint32), by_lens.view(np.uint32))
    assert (real[:, 0] != real[:, 1]).sum() >= 50


@pytest.mark.parametrize("case", lc.ORACLE_CASES, ids=lc.case_id)
def test_no_case_passes_on_background(case):
    lc.check_floors(case)


def test_argument_errors():
    L = _lib.lib()
    ones = np.ones((2, 3, 3), f32)
    for shape in ((3, 2, 3), (2, 3), (2, 3, 4), (6, 3)):
        with pytest.raises(ValueError, match="shape"):
            Lens(3, 2, np.ones(shape, f32))
    for w, h in ((0, 2), (3, 0), (-1, 2), (3, -5)):
        with pytest.raises(ValueError):
            Lens(w, h, ones)
        with pytest.raises(ValueError):
            Lens.pinhole(w, h, 0.8)
        assert not L.nt_lens_create(w, h, ones.ctypes.data_as(_lib.f32p)) and "invalid lens size" in _lib.last_error()
        assert not L.nt_lens_create_pinhole(w, h, 0.8)
    with pytest.raises(ValueError):
        Lens(True, 2, ones)
    assert not L.nt_lens_create(3, 2, None)
    assert L.nt_lens_width(None) == _lib.NT_E_INVALID and L.nt_lens_height(None) == _lib.NT_E_INVALID
    assert L.nt_scene_set_lens(None, None) == _lib.NT_E_INVALID
    L.nt_lens_destroy(None)
    sc = tracern.BoxScene(4)
    with pytest.raises(TypeError):
        sc.set_lens(ones)
    with pytest.raises(TypeError):
        Lens(3, 2, ones).directions("camera")


@pytest.mark.parametrize("kind", ["composite", "box"])
def test_what_a_lens_refuses_is_refused_before_a_device_is_touched(kind):
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
    sc.set_lens(Lens.pinhole(w + 1, h, 0.8))
    assert sc.lens.width == w + 1

    def calls(opts=None):
        o = C.byref(opts) if opts is not None else None
        cams = np.zeros((1, n), f32), np.eye(n, dtype=f32)[None].copy()
        return [L.nt_render(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_device(sc._handle, dest.ctypes.data, dest.nbytes, C.byref(fst), o, None),
                L.nt_render_frames_device(sc._handle, dest.ctypes.data, dest.nbytes, 1, cams[0].ctypes.data_as(_lib.f32p),
                                          cams[1].ctypes.data_as(_lib.f32p), C.byref(fst), o, None)]
    # a lens of another size than the render: NT_E_INVALID, and the message names both sizes
    for r in calls():
        assert r == _lib.NT_E_INVALID
        assert "9 x 5" in _lib.last_error() and "8 x 5" in _lib.last_error()
    with pytest.raises(ValueError, match="the lens is for 9 x 5 pixels, the render is of 8 x 5"):
        ntracer_amd.BlockingRenderer().render(bytearray(w * h * 4), fmt, sc)
    # a second lens replaces the first; what a lens does not do is NT_E_UNSUPPORTED
    sc.set_lens(Lens.fisheye(w, h, 3.0))
    assert (sc.lens.width, sc.lens.height) == (w, h)
    sc.set_supersampling(2)
    for r in calls():
        assert r == _lib.NT_E_UNSUPPORTED and "supersampling" in _lib.last_error()
    sc.set_supersampling(1)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world, opts.band_rank = -1, 2, 1
    for r in calls(opts):
        assert r == _lib.NT_E_UNSUPPORTED and "band" in _lib.last_error()
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    for r in calls(opts):
        assert r == _lib.NT_E_UNSUPPORTED and "collect_stats" in _lib.last_error()
    with pytest.raises(NotImplementedError, match="lens"):
        sc.calculate_color(1, 1, w, h)
    with pytest.raises(NotImplementedError, match="lens"):
        sc.colors_at([1], [1], w, h)
    if kind == "composite":
        with pytest.raises(NotImplementedError, match="lens"):
            sc.primary_hits(w, h)
    assert (dest == 0xab).all()                                        # nothing was drawn
    # without the lens the same calls get past the checks: on a machine without a GPU they end at the device, not before
    sc.set_lens(None)
    assert sc.lens is None
    assert not L.nt_scene_get_lens(sc._handle)
    for r in calls():
        assert r in (_lib.NT_OK, _lib.NT_E_DEVICE)


def test_the_lock_rule_and_shared_ownership():
    L = _lib.lib()
    sc = tracern.BoxScene(5)
    ln = Lens.pinhole(4, 3, 0.8)
    assert L.nt_scene_lock(sc._handle) == _lib.NT_OK
    with pytest.raises(ntracer_amd.LockedError):
        sc.set_lens(ln)
    assert sc.lens is None and not L.nt_scene_get_lens(sc._handle)
    with pytest.raises(ntracer_amd.LockedError):
        sc.set_camera(tracern.Camera(5))                               # (the rule it shares)
    assert L.nt_scene_unlock(sc._handle) == _lib.NT_OK
    sc.set_lens(ln)
    table = ln.coeffs
    # the handle goes, the scene keeps the table: a handle of the scene's own still reads it
    h = ln._handle
    ln._handle = None
    L.nt_lens_destroy(h)
    del ln
    sc._lens = None
    again = L.nt_scene_get_lens(sc._handle)
    assert again
    got = Lens._adopt(again)
    assert (got.width, got.height) == (4, 3) and np.array_equal(got.coeffs.view(np.uint32), table.view(np.uint32))
    # one lens on two scenes; the scenes go first, then the last handle
    other = tracern.BoxScene(7)
    other.set_lens(got)
    del sc, other
    assert got.coeffs.shape == (3, 4, 3)
    del got
