"""Renders through a lens (Scene.set_lens; nt_render, nt_render_device, nt_render_frames_device, nt_render_table_device) on
the GPU: the pinhole lens against the plain render, byte for byte; the fisheye and the equirectangular panorama against the
oracle on every pixel; masked pixels, shapes, formats, camera tables, the ray path, state and refusals.

Expected colours come from lens_cases: the oracle's colour of the ray `Lens.directions` gives for the pixel (the method is
pinned by tests/test_lens_host.py), the oracle in the GPU's mode.  Tolerances are the project's own: CompositeScene fp32
colours within 1e-5 of the oracle on every pixel and packed channels within 1; BoxScene bit for bit.  Every test prints its
worst difference.  Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import lens_cases as lc
import oracle_binding as ob
import support as sup
import ntracer_amd
from ntracer_amd import Lens, _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

TOL = 1e-5
f32 = np.float32
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# fp32 x 3 at a quarter of the colour: the lit scenes' colours reach 3.1 under the close cameras of lens_cases, and a format clamps at
# 1 -- a comparison of clamped colours would pass on white.  A quarter is exact in fp32, so nothing is lost: got * 4 is the colour.
QUARTER = [(32, 0.25, 0, 0, 0, True), (32, 0, 0.25, 0, 0, True), (32, 0, 0, 0.25, 0, True)]


def _bpp(chans):
    return sum(c[0] for c in chans) // 8


def _render(sc, fmt):
    buf = bytearray(fmt.pitch * fmt.height)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc) is True
    return np.frombuffer(bytes(buf), np.uint8).reshape(fmt.height, fmt.pitch)


def _floats(img, w, h):
    """[h * w][3] colours of an RGBF32 image (big-endian floats, no padding)"""
    return np.ascontiguousarray(img[:, :w * 12]).view(">f4").astype(f32).reshape(h * w, 3)


def _packed(colours, chans, rev, w, h):
    return np.frombuffer(b"".join(ob.pack_pixel(c, chans, rev) for c in colours), np.uint8).reshape(h, w * _bpp(chans))


def _channels(img, chans, rev, w):
    """the packed image as integers a channel (8- and 16-bit channels): [h][w * channels]"""
    bits = chans[0][0]
    a = np.ascontiguousarray(img[:, :w * _bpp(chans)])
    return a.astype(int) if bits == 8 else a.view("<u2" if rev else ">u2").astype(int)


def _check(case, got_f32, want, what="", scale=1.0):
    """fp32 colours [pixels][3] against the oracle's (clamped as the format clamps; scale 4: rendered into QUARTER): BoxScene bit
    for bit, else within TOL"""
    want = (np.clip(want, 0.0, scale) + 0.0).astype(f32)         # (+ 0.0: the clamp gives +0 where the oracle's colour is -0)
    got_f32 = (got_f32 * f32(scale)).astype(f32)
    if lc.is_box(case[0]):
        bad = np.nonzero((got_f32.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, "%s%s: %d pixels differ, first %d: got %r, oracle %r" % (lc.case_id(case), what, len(bad), bad[0], got_f32[bad[0]], want[bad[0]])
        return 0.0
    err = np.abs(got_f32.astype(np.float64) - want).max(axis=1)
    bad = np.nonzero(~(err <= TOL))[0]
    assert len(bad) == 0, "%s%s: %d pixels beyond %g (worst %g), first %d: got %r, oracle %r" % (lc.case_id(case), what, len(bad), TOL, err.max(), bad[0],
                                                                                           got_f32[bad[0]], want[bad[0]])
    return float(err.max())


PINHOLE_FORMATS = [(fx.RGBF32, "f32x3"), (fx.RGBX8, "rgbx8"), (QUARTER, "quarter")]


@pytest.mark.parametrize("scene", lc.SCENES, ids=lambda s: s[0] + ("," + s[2] if s[2] else ""))
def test_the_pinhole_lens_is_the_plain_render_byte_for_byte(scene):
    w, h = lc.size(scene[0])
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        for chans, _ in PINHOLE_FORMATS:
            fmt = sup.fmt_of(w, h, chans)
            sc.set_lens(None)
            plain = _render(sc, fmt)
            sc.set_lens(Lens.pinhole(w, h, lc.FOV))
            sc.set_fov(2.0)                                             # (ignored while a lens is set)
            through = _render(sc, fmt)
            sc.set_fov(lc.FOV)
            assert np.array_equal(plain, through), (scene, chans[0], int((plain != through).sum()))
        assert len(np.unique(plain.reshape(h * w, -1), axis=0)) > 20            # (QUARTER: an image, not one colour)


@pytest.mark.parametrize("case", lc.ORACLE_CASES, ids=lc.case_id)
def test_lens_renders_equal_the_oracle_on_every_pixel(case):
    counts = lc.check_floors(case)
    w, h = lc.size(case[0])
    ln = lc.lens(case)
    want = lc.expected(case)
    masked = ln.masked.reshape(-1)
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(case, mp)
        sc.set_lens(ln)
        assert want.max() < 4.0
        got = _floats(_render(sc, sup.fmt_of(w, h, QUARTER)), w, h)
        worst = _check(case, got, want, scale=4.0)
        assert (got[masked].view(np.uint32) == 0).all()                 # masked pixels: exactly (0, 0, 0)
        plain = _floats(_render(sc, sup.fmt_of(w, h, fx.RGBF32)), w, h)       # ... and the plain fp32 x 3 format: the same colours, clamped
        worst = max(worst, _check(case, plain, want))
        assert (plain[masked].view(np.uint32) == 0).all()
        img = _render(sc, sup.fmt_of(w, h, fx.RGBX8))
        ref = _packed(want, fx.RGBX8, False, w, h)
        diff = np.abs(img.astype(int) - ref.astype(int)).max()
        assert diff <= (0 if lc.is_box(case[0]) else 1), (lc.case_id(case), int(diff))
        assert not img.reshape(h * w, 4)[masked].any()                  # ... and pack as black
    print("%s: %d pixels (%d masked; oracle: %d opaque hits, %d with a transparent hit), worst difference %g, worst byte %d"
          % ((lc.case_id(case), w * h, int(masked.sum())) + counts + (worst, int(diff))))


SHAPE_SCENES = [("cell600_n4", {}, "lit"), ("cell600_n4", {}, ""), ("feature5_n5", {}, ""), ("box6", {}, "")]
SHAPES = [(1, 1), (8, 8), (9, 17), (64, 48)]


def _expected_for(scene, ln):
    """the oracle's image through any Lens under the scene's case camera"""
    o, q = lc.camera(scene[0])
    live = ~ln.masked.reshape(-1)
    v = ln.directions(lc.camera_of(o, q))
    out = np.zeros((len(v), 3), f32)
    if live.any():
        out[live] = lc.oracle_colors(scene[0], scene[1], scene[2], o, v[live])
    return out


@pytest.mark.parametrize("scene", SHAPE_SCENES, ids=lambda s: s[0] + ("," + s[2] if s[2] else ""))
def test_shapes_and_formats(scene):
    """1 x 1, one tile, odd sizes, more than one block; RGB24 at an odd width (shared dword stores on the packet route, pixel by
    pixel on the ray route: 9 and 37 pixels of 3 bytes with one byte of padding are rows of whole dwords), reversed formats, a
    padded pitch whose bytes stay the caller's"""
    case = scene + ("",)
    worst = 0.0
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        for w, h in SHAPES:
            for name in ("fisheye", "equirect"):
                ln = lc.LENSES[name](w, h)
                want = _expected_for(scene, ln)
                sc.set_lens(ln)
                worst = max(worst, _check(case, _floats(_render(sc, sup.fmt_of(w, h, fx.RGBF32)), w, h), want, " %dx%d %s" % (w, h, name)))
        for (w, h), chans, pad, rev in (((9, 17), RGB24, 1, False), ((37, 29), RGB24, 0, True), ((37, 29), RGB24, 1, False),
                                        ((9, 17), fx.RGBX8, 0, True), ((37, 29), fx.RGB16, 7, False), ((9, 17), fx.RGBF32, 12, True)):
            ln = lc.LENSES["fisheye"](w, h)
            want = _expected_for(scene, ln)
            bpp = _bpp(chans)
            pitch = w * bpp + pad
            fmt = sup.fmt_of(w, h, chans, pitch if pad else 0, rev)
            sc.set_lens(ln)
            buf = bytearray(b"\xab" * (pitch * h))
            assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc) is True
            img = np.frombuffer(bytes(buf), np.uint8).reshape(h, pitch)
            assert (img[:, w * bpp:] == 0xab).all(), (w, h, chans[0], pad)
            if chans is fx.RGBF32:
                px = np.ascontiguousarray(img[:, :w * 12]).view("<f4").astype(f32).reshape(h * w, 3)[:, ::-1]       # reversed: b, g, r little-endian
                worst = max(worst, _check(case, np.ascontiguousarray(px), want, " reversed f32"))
            else:
                ref = _packed(want, chans, rev, w, h)
                diff = np.abs(_channels(img, chans, rev, w) - _channels(ref, chans, rev, w)).max()
                assert diff <= (0 if lc.is_box(scene[0]) else 1), (scene, w, h, chans[0], pad, rev, int(diff))
    print("%s: worst difference over the shapes %g" % (scene[0], worst))


@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("feature5_n5", {}, ""), ("box6", {}, "")], ids=lambda s: s[0])
def test_masked_pixels_and_the_bytes_outside_the_image(scene):
    """the device path into a buffer with a padded pitch and a guard region behind the image: masked pixels are written as
    black, and not a byte outside the pixels changes"""
    import torch
    w, h = lc.W, lc.H
    ln = lc.lens_at("fisheye", w, h)
    masked = ln.masked
    assert masked[0, 0] and masked[h - 1, w - 1] and not masked[h // 2, w // 2]
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        sc.set_lens(ln)
        for chans in (fx.RGBF32, fx.RGBX8, RGB24):
            bpp = _bpp(chans)
            pitch = w * bpp + 8
            fmt = sup.fmt_of(w, h, chans, pitch)
            dest = torch.full((h + 3, pitch), 0xab, dtype=torch.uint8, device=sup.cuda_device())
            assert ntracer_amd.BlockingRenderer().render(dest, fmt, sc) is True
            torch.cuda.synchronize()
            got = dest.cpu().numpy()
            assert (got[h:] == 0xab).all() and (got[:h, w * bpp:] == 0xab).all(), chans[0]
            px = got[:h, :w * bpp].reshape(h, w, bpp)
            assert not px[masked].any(), chans[0]
            assert np.array_equal(got[:h, :w * bpp], _render(sc, sup.fmt_of(w, h, chans))), chans[0]       # the host path: the same bytes
            assert px[~masked].any()


def _three_cameras(name):
    o, q = lc.camera(name)
    return [(o, q), ((o + f32(0.3) * q[0]).astype(f32), q), ((o - f32(0.2) * q[1] + f32(0.1) * q[2]).astype(f32), q)]


@pytest.mark.parametrize("chunk", [None, "1"], ids=["one_launch", "a_frame_a_chunk"])
@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("cell600_n4", {}, "lit"), ("feature5_n5", {}, "")], ids=lambda s: s[0] + s[2])
def test_a_camera_table_with_a_padded_frame_stride(scene, chunk):
    """three cameras in one nt_render_table_device call, every frame against the oracle; with NTRACER_CHUNK_FRAMES=1 the hit
    scratch holds one frame a chunk; then the same frames through nt_render_frames_device with host cameras: the same bytes"""
    import torch
    w, h = lc.W, lc.H
    case = scene + ("fisheye",)
    ln = lc.lens(case)
    cams = _three_cameras(scene[0])
    n = len(cams[0][0])
    fmt = sup.fmt_of(w, h, QUARTER)
    frame = w * h * 12
    stride = frame + 20
    worst = 0.0
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        if chunk:
            mp.setenv("NTRACER_CHUNK_FRAMES", chunk)
        sc.set_lens(ln)
        origins = np.stack([c[0] for c in cams]).astype(f32)
        axes = np.stack([c[1] for c in cams]).astype(f32)
        table = CameraTable(n, origins, axes, sup.cuda_device().index)
        dest = torch.full((3 * stride,), 0xab, dtype=torch.uint8, device=sup.cuda_device())
        assert table.render(sc, dest, fmt, frame_bytes=stride) is True
        torch.cuda.synchronize()
        got = dest.cpu().numpy().reshape(3, stride)
        assert (got[:, frame:] == 0xab).all()
        for k, cam in enumerate(cams):
            px = got[k, :frame].view(">f4").astype(f32).reshape(w * h, 3)
            worst = max(worst, _check(case, px, lc.expected(case, cam), " frame %d" % k, scale=4.0))
        assert not np.array_equal(got[0, :frame], got[1, :frame]) and not np.array_equal(got[1, :frame], got[2, :frame])
        # host cameras
        dest2 = torch.full((3 * stride,), 0xab, dtype=torch.uint8, device=sup.cuda_device())
        fst = fmt._as_struct()
        opts = _lib.NtRenderOpts()
        opts.device = sup.cuda_device().index
        stream = torch.cuda.current_stream(sup.cuda_device()).cuda_stream
        _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest2.data_ptr()), stride, 3, origins.ctypes.data_as(_lib.f32p),
                                                      axes.ctypes.data_as(_lib.f32p), C.byref(fst), C.byref(opts), C.c_void_p(stream)))
        torch.cuda.synchronize()
        assert np.array_equal(dest2.cpu().numpy(), dest.cpu().numpy())
    print("%s: worst difference over three frames %g" % (lc.case_id(case), worst))


@pytest.mark.parametrize("scene", [("cell600_n4", {}, "lit"), ("box6", {}, "")], ids=lambda s: s[0])
def test_the_ray_path_gives_the_lens_renders_bytes(scene):
    """scene.render_rays on lens.directions(camera): what a render through the lens casts, so the same bytes (lenses without
    masked pixels: the host form of render_rays refuses a zero direction)"""
    w, h = lc.size(scene[0])
    o, q = lc.camera(scene[0])
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        for name in ("equirect", "fisheye_open", "cylindrical"):
            ln = lc.lens_at(name, w, h)
            assert not ln.masked.any()
            v = ln.directions(lc.camera_of(o, q))
            for chans in (fx.RGBF32, fx.RGBX8):
                fmt = sup.fmt_of(w, h, chans)
                sc.set_lens(ln)
                through = _render(sc, fmt)
                sc.set_lens(None)
                buf = bytearray(fmt.pitch * h)
                assert sc.render_rays(buf, fmt, o, v) is True
                by_rays = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
                assert np.array_equal(through, by_rays), (scene[0], name, chans[0], int((through != by_rays).sum()))
                assert len(np.unique(through.reshape(h * w, -1), axis=0)) > 20


@pytest.mark.parametrize("scene", [("cell600_n4", {}, "lit"), ("feature5_n5", {}, ""), ("box6", {}, "")], ids=lambda s: s[0])
def test_state(scene):
    """set_lens(None) restores the plain render; a second lens of another size replaces the first; a plain render after a lens
    render on the same scene and stream is right (the hit and `checked` scratch is shared); the abort word on the device path"""
    import torch
    w, h = lc.W, lc.H
    fmt = sup.fmt_of(w, h, fx.RGBF32)
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        plain = _render(sc, fmt)
        ln = lc.lens_at("fisheye", w, h)
        sc.set_lens(ln)
        through = _render(sc, fmt)
        assert not np.array_equal(plain, through)
        sc.set_lens(None)
        assert np.array_equal(_render(sc, fmt), plain)
        # a larger lens replaces the first: the old size is refused, the new one renders, and the first renders again afterwards
        big = lc.lens_at("fisheye", 64, 48)
        sc.set_lens(ln)
        sc.set_lens(big)
        with pytest.raises(ValueError, match="the lens is for 64 x 48 pixels"):
            _render(sc, fmt)
        big_img = _render(sc, sup.fmt_of(64, 48, fx.RGBF32))
        _check(scene + ("",), _floats(big_img, 64, 48), _expected_for(scene, big), " 64x48")
        sc.set_lens(ln)
        assert np.array_equal(_render(sc, fmt), through)
        sc.set_lens(None)
        assert np.array_equal(_render(sc, fmt), plain)
        # the abort word, raised before the call: nothing is written; lowered: the lens render's bytes
        sc.set_lens(ln)
        dev = sup.cuda_device()
        word = torch.ones(1, dtype=torch.int32, device=dev)
        dest = torch.full((h, fmt.pitch), 0xab, dtype=torch.uint8, device=dev)
        fst = fmt._as_struct()
        opts = _lib.NtRenderOpts()
        opts.device = dev.index
        opts.abort_device = word.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def go():
            _lib.check(_lib.lib().nt_render_device(sc._handle, C.c_void_p(dest.data_ptr()), dest.numel(), C.byref(fst), C.byref(opts), C.c_void_p(stream)))
            torch.cuda.synchronize()
        go()
        assert bool((dest == 0xab).all())
        word.fill_(0)
        torch.cuda.synchronize()
        go()
        assert np.array_equal(dest.cpu().numpy(), through)


@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("box6", {}, "")], ids=lambda s: s[0])
def test_refusals_draw_nothing(scene):
    import torch
    w, h = lc.W, lc.H
    fmt = sup.fmt_of(w, h, fx.RGBX8)
    with pytest.MonkeyPatch.context() as mp:
        sc = lc.scene(scene, mp)
        sc.set_lens(lc.lens_at("fisheye", w, h))
        dest = torch.full((h, fmt.pitch), 0xab, dtype=torch.uint8, device=sup.cuda_device())
        r = ntracer_amd.BlockingRenderer()
        sc.set_supersampling(2)
        with pytest.raises(NotImplementedError, match="supersampling"):
            r.render(dest, fmt, sc)
        with pytest.raises(NotImplementedError, match="supersampling"):
            r.render(bytearray(fmt.pitch * h), fmt, sc)
        sc.set_supersampling(1)
        with pytest.raises(NotImplementedError, match="band"):
            r.render(dest, fmt, sc, band_rank=1, band_world=2)
        with pytest.raises(NotImplementedError, match="collect_stats"):
            r.render(dest, fmt, sc, collect_stats=True)
        with pytest.raises(NotImplementedError, match="lens"):
            sc.calculate_color(3, 4, w, h)
        if not lc.is_box(scene[0]):
            with pytest.raises(NotImplementedError, match="lens"):
                sc.primary_hits(w, h)
        with pytest.raises(ValueError, match="the lens is for"):
            r.render(torch.zeros((h, 4 * (w + 1)), dtype=torch.uint8, device=sup.cuda_device()), sup.fmt_of(w + 1, h, fx.RGBX8), sc)
        torch.cuda.synchronize()
        assert bool((dest == 0xab).all())
        # the ray entry points ignore the lens
        o, q = lc.camera(scene[0])
        v = lc.lens_at("equirect", w, h).directions(lc.camera_of(o, q))
        a = sc.ray_colors(o, v)
        sc.set_lens(None)
        assert np.array_equal(a.view(np.uint32), sc.ray_colors(o, v).view(np.uint32))
