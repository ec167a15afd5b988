"""Renders under the parallel projection (Scene.set_parallel_projection; nt_render, nt_render_device, nt_render_frames_device,
nt_render_table_device) on the GPU: every scene of parallel_cases against the oracle on every pixel, rays that start inside the
scene box, the switched cases (the per-lane kernels' second opinion on the packet walk), the ray path, shapes, formats, camera
tables, state and refusals.

Expected colours come from parallel_cases: the oracle's colour of the ray (o', forward) of the pixel, the oracle in the GPU's
mode.  Tolerances are the project's own: CompositeScene fp32 colours within 1e-5 of the oracle on every pixel and packed
channels within 1; BoxScene bit for bit.  Every test prints its worst difference.  Each test runs its GPU work once; nothing
is retried."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import parallel_cases as pc
import support as sup
import ntracer_amd
from ntracer_amd import _lib
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

TOL = 1e-5
f32 = np.float32
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# fp32 x 3 at a quarter of the colour: the lit scene's colours exceed 1 in 871 of its 872 hit pixels, and a format clamps at 1 -- a
# comparison of clamped colours would pass on white.  A quarter is exact in fp32, so nothing is lost: got * 4 is the colour (five
# pixels of the lit 600-cell exceed 4, up to 4.18, and are compared at the clamp).
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
    if pc.is_box(case[0]):
        bad = np.nonzero((got_f32.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, "%s%s: %d pixels differ, first %d: got %r, oracle %r" % (pc.case_id(case), what, len(bad), bad[0], got_f32[bad[0]], want[bad[0]])
        return 0.0
    err = np.abs(got_f32.astype(np.float64) - want).max(axis=1)
    bad = np.nonzero(~(err <= TOL))[0]
    assert len(bad) == 0, "%s%s: %d pixels beyond %g (worst %g), first %d: got %r, oracle %r" % (pc.case_id(case), what, len(bad), TOL, err.max(), bad[0],
                                                                                           got_f32[bad[0]], want[bad[0]])
    return float(err.max())


def _against_the_oracle(case, sc, want, what=""):
    """the case in three formats: a quarter-scale fp32 (unclamped colours), plain fp32 x 3 and RGBX8"""
    w, h = pc.W, pc.H
    assert (want.max(axis=1) >= 4.0).mean() < 0.01             # (the lit 600-cell: 5 of 1 073 pixels reach the quarter format's clamp)
    worst = _check(case, _floats(_render(sc, sup.fmt_of(w, h, QUARTER)), w, h), want, what, scale=4.0)
    worst = max(worst, _check(case, _floats(_render(sc, sup.fmt_of(w, h, fx.RGBF32)), w, h), want, what))
    img = _render(sc, sup.fmt_of(w, h, fx.RGBX8))
    diff = np.abs(img.astype(int) - _packed(want, fx.RGBX8, False, w, h).astype(int)).max()
    assert diff <= (0 if pc.is_box(case[0]) else 1), (pc.case_id(case), what, int(diff))
    return worst, int(diff)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_parallel_renders_equal_the_oracle_on_every_pixel(case):
    counts = pc.check_floors(case)
    want = pc.expected(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(case, mp)
        sc.set_fov(2.0)                                                 # (ignored while the projection is set)
        worst, diff = _against_the_oracle(case, sc, want)
    print("%s: %d pixels (oracle: %d opaque hits, %d with a transparent hit), worst difference %g, worst byte %d"
          % ((pc.case_id(case), pc.W * pc.H) + counts + (worst, diff)))


@pytest.mark.parametrize("env", [{}, pc.PLAIN], ids=["packet", "per_lane"])
def test_rays_that_start_inside_the_scene_box(env):
    """the 600-cell's camera at the centre of the scene's box: t_near = 0 for nearly every ray"""
    case = ("cell600_n4", env, "")
    cam = pc.centre_camera(case[0])
    assert pc.counts(case[0], True)[0] >= pc.MIN_OPAQUE
    org = pc.parallel_rays(cam[0], cam[1], pc.W, pc.H, pc.half_width(case[0]))[0]
    assert pc.inside_box(case[0], org) > 1000
    want = pc.expected(case, cam)
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(case, mp, cam)
        worst, diff = _against_the_oracle(case, sc, want, " from inside")
    print("%s from inside its box: worst difference %g, worst byte %d" % (pc.case_id(case), worst, diff))


SHAPE_SCENES = [("cell600_n4", {}, "lit"), ("cell600_n4", {}, ""), ("feature5_n5", {}, ""), ("box6", {}, "")]
SHAPES = [(1, 1), (8, 8), (9, 17), (64, 48)]


@pytest.mark.parametrize("scene", SHAPE_SCENES, ids=pc.case_id)
def test_shapes_and_formats(scene):
    """1 x 1, one tile, odd sizes (partial tiles, partial 2 x 2 quads), more than one block; RGB24 at odd widths, reversed
    formats, a padded pitch whose guard bytes stay the caller's; a quarter-scale fp32 format for the lit scene"""
    worst = 0.0
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
        for w, h in SHAPES:
            want = pc.expected(scene, size=(w, h))
            worst = max(worst, _check(scene, _floats(_render(sc, sup.fmt_of(w, h, QUARTER)), w, h), want, " %dx%d" % (w, h), scale=4.0))
        for (w, h), chans, pad, rev in (((9, 17), RGB24, 1, False), ((37, 29), RGB24, 0, True), ((37, 29), RGB24, 1, False),
                                        ((9, 17), fx.RGBX8, 0, True), ((37, 29), fx.RGB16, 7, False), ((9, 17), fx.RGBF32, 12, True)):
            want = pc.expected(scene, size=(w, h))
            bpp = _bpp(chans)
            pitch = w * bpp + pad
            fmt = sup.fmt_of(w, h, chans, pitch if pad else 0, rev)
            buf = bytearray(b"\xab" * (pitch * h))
            assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc) is True
            img = np.frombuffer(bytes(buf), np.uint8).reshape(h, pitch)
            assert (img[:, w * bpp:] == 0xab).all(), (w, h, chans[0], pad)
            if chans is fx.RGBF32:
                px = np.ascontiguousarray(img[:, :w * 12]).view("<f4").astype(f32).reshape(h * w, 3)[:, ::-1]       # reversed: b, g, r little-endian
                worst = max(worst, _check(scene, np.ascontiguousarray(px), want, " reversed f32"))
            else:
                ref = _packed(want, chans, rev, w, h)
                diff = np.abs(_channels(img, chans, rev, w) - _channels(ref, chans, rev, w)).max()
                assert diff <= (0 if pc.is_box(scene[0]) else 1), (scene, w, h, chans[0], pad, rev, int(diff))
    print("%s: worst difference over the shapes %g" % (pc.case_id(scene), worst))


@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("feature5_n5", {}, ""), ("box6", {}, "")], ids=pc.case_id)
def test_the_device_path_leaves_the_bytes_outside_the_image(scene):
    import torch
    w, h = pc.W, pc.H
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
        for chans in (fx.RGBF32, fx.RGBX8, RGB24):
            bpp = _bpp(chans)
            pitch = w * bpp + 8
            fmt = sup.fmt_of(w, h, chans, pitch)
            dest = torch.full((h + 3, pitch), 0xab, dtype=torch.uint8, device=sup.cuda_device())
            assert ntracer_amd.BlockingRenderer().render(dest, fmt, sc) is True
            torch.cuda.synchronize()
            got = dest.cpu().numpy()
            assert (got[h:] == 0xab).all() and (got[:h, w * bpp:] == 0xab).all(), chans[0]
            assert np.array_equal(got[:h, :w * bpp], _render(sc, sup.fmt_of(w, h, chans))), chans[0]       # the host path: the same bytes


def _three_cameras(name):
    o, q = pc.camera(name)
    return [(o, q), ((o + f32(0.3) * q[0]).astype(f32), q), ((o - f32(0.2) * q[1] + f32(0.1) * q[2]).astype(f32), q)]


@pytest.mark.parametrize("chunk", [None, "1"], ids=["one_launch", "a_frame_a_chunk"])
@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("cell600_n4", {}, "lit"), ("feature5_n5", {}, "")], ids=pc.case_id)
def test_a_camera_table_with_a_padded_frame_stride(scene, chunk):
    """three cameras in one nt_render_table_device call, every frame against the oracle; with NTRACER_CHUNK_FRAMES=1 the hit
    scratch holds one frame a chunk; then the same frames through nt_render_frames_device with host cameras: the same bytes"""
    import torch
    w, h = pc.W, pc.H
    cams = _three_cameras(scene[0])
    n = len(cams[0][0])
    fmt = sup.fmt_of(w, h, QUARTER)
    frame = w * h * 12
    stride = frame + 20
    worst = 0.0
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
        if chunk:
            mp.setenv("NTRACER_CHUNK_FRAMES", chunk)
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
            worst = max(worst, _check(scene, px, pc.expected(scene, cam), " frame %d" % k, scale=4.0))
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
    print("%s: worst difference over three frames %g" % (pc.case_id(scene), worst))


@pytest.mark.parametrize("scene", [("cell600_n4", {}, "lit"), ("feature5_n5", {}, ""), ("box6", {}, "")], ids=pc.case_id)
def test_the_ray_path_gives_the_parallel_renders_bytes(scene):
    """scene.render_rays on scene.parallel_rays: what a parallel render casts, so the same bytes -- a packet scene against the
    per-lane ray kernels, and two ray-route scenes against the route they share"""
    w, h = pc.W, pc.H
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
        org, fwd = sc.parallel_rays(w, h)
        want_o, want_f = pc.parallel_rays(*pc.camera(scene[0]), w, h, pc.half_width(scene[0]))
        assert np.array_equal(org.view(np.uint32), want_o.view(np.uint32)) and np.array_equal(fwd, want_f)
        rays = (org, np.broadcast_to(fwd, org.shape))                       # (the ray entry points take a direction a ray)
        for chans in (fx.RGBF32, fx.RGBX8):
            fmt = sup.fmt_of(w, h, chans)
            through = _render(sc, fmt)
            buf = bytearray(fmt.pitch * h)
            assert sc.render_rays(buf, fmt, *rays) is True                  # (the ray entry points ignore the setting)
            by_rays = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
            assert np.array_equal(through, by_rays), (scene[0], chans[0], int((through != by_rays).sum()))
            assert len(np.unique(through.reshape(h * w, -1), axis=0)) >= 2      # (an image: the oracle's boxes show two colours, feature5_n5 16)
        a = sc.ray_colors(*rays)
        sc.set_parallel_projection(None)
        assert np.array_equal(a.view(np.uint32), sc.ray_colors(*rays).view(np.uint32))


@pytest.mark.parametrize("scene", [("cell600_n4", {}, "lit"), ("feature5_n5", {}, ""), ("box6", {}, "")], ids=pc.case_id)
def test_state(scene):
    """set_parallel_projection(None) restores the plain render's bytes; a plain render after a parallel one on the same scene
    and stream is right (the hit and `checked` scratch is shared); the abort word on the device path"""
    import torch
    w, h = pc.W, pc.H
    fmt = sup.fmt_of(w, h, fx.RGBF32)
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
        sc.set_parallel_projection(None)
        plain = _render(sc, fmt)
        sc.set_parallel_projection(pc.half_width(scene[0]))
        through = _render(sc, fmt)
        assert not np.array_equal(plain, through)
        _check(scene, _floats(through, w, h), pc.expected(scene))
        sc.set_parallel_projection(None)
        assert np.array_equal(_render(sc, fmt), plain)
        sc.set_parallel_projection(2.0 * pc.half_width(scene[0]))         # another width: another image, then the first again
        assert not np.array_equal(_render(sc, fmt), through)
        sc.set_parallel_projection(pc.half_width(scene[0]))
        assert np.array_equal(_render(sc, fmt), through)
        # the abort word, raised before the call: nothing is written; lowered: the parallel render's bytes
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
        sc.set_parallel_projection(None)
        assert np.array_equal(_render(sc, fmt), plain)


@pytest.mark.parametrize("scene", [("cell600_n4", {}, ""), ("box6", {}, "")], ids=pc.case_id)
def test_refusals_draw_nothing(scene):
    import torch
    w, h = pc.W, pc.H
    fmt = sup.fmt_of(w, h, fx.RGBX8)
    with pytest.MonkeyPatch.context() as mp:
        sc = pc.scene(scene, mp)
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
        with pytest.raises(NotImplementedError, match="parallel"):
            sc.calculate_color(3, 4, w, h)
        if not pc.is_box(scene[0]):
            with pytest.raises(NotImplementedError, match="parallel"):
                sc.primary_hits(w, h)
        torch.cuda.synchronize()
        assert bool((dest == 0xab).all())
