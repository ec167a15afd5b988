"""Depth cues (scene.set_depth_cue, scene.depth_cue_factors, nt_depth_cue_factors*, and the renders that honour the setting) on the
GPU against the oracle.

The expected factors never come from the library: tests/cue_cases.py works them out for every pixel from the oracle's primary-hit
records and ray directions, by the definition in include/ntracer_hip.h.  Factors must be equal bit for bit, no tolerance: the
existing suite pins dist to the oracle bitwise, and everything after it is specified fp32 arithmetic without contraction.  A
render with the setting on must be, byte for byte, the library's own plain fp32 x 3 frame P (pinned to the oracle by the existing
suite) blended by cue_cases.blend with the oracle-derived factors and packed by the oracle's pack_pixel.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import cue_cases as cc
import fixtures as fx
import ntracer_amd
import primary_hit_cases as ph
import ray_color_cases as rc
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
PAD = 29                        # bytes behind the factors
W, H = cc.W, cc.H
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# (name, channels, reversed): 4-, 3-, 6- and 12-byte pixels, and a reversed one
FORMATS = [("rgbx8", fx.RGBX8, False), ("rgb24", RGB24, False), ("rgb16", fx.RGB16, False), ("rgbf32", fx.RGBF32, False),
           ("rgb24-reversed", RGB24, True)]
# (tint, fog_background): fog alone, fog + tint, and the background either way
SETTINGS = [(False, False), (True, True), (False, True), (True, False)]


def _scene(case, mp, k=0, variant=""):
    name, env = case
    sup.set_switches(mp, cc.SWITCHES, env)
    n, flat, params = rc.case_scene((name, env, variant))
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(params)
    sc.set_fov(ph.fov_of(name))
    sc._set_camera_arrays(*ph.camera(name, k))
    return sc


def _set(sc, st):
    """the setting through the ABI, every value as cue_cases has it"""
    cue = _lib.NtDepthCue()
    cue.fog_near, cue.fog_far, cue.fog_strength = st["fog_near"], st["fog_far"], st["fog_strength"]
    cue.fog_background = 1 if st["fog_background"] else 0
    cue.fog_color[:] = st["fog_color"]
    axis = None
    if st["tint_axis"] is not None:
        cue.tint_lo, cue.tint_hi = st["tint_lo"], st["tint_hi"]
        cue.tint_color_lo[:] = st["tint_color_lo"]
        cue.tint_color_hi[:] = st["tint_color_hi"]
        axis = (C.c_float * len(st["tint_axis"]))(*st["tint_axis"])
    _lib.check(_lib.lib().nt_scene_set_depth_cue(sc._handle, C.byref(cue), axis))


def _device_factors(sc, w, h, abort=None):
    """nt_depth_cue_factors_device on a sentinel-filled buffer with PAD bytes behind it: the raw buffer"""
    import torch
    buf = torch.full((w * h * 8 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    opts = sup.render_opts(abort, strict_reference=sup.strict_reference())
    _lib.check(_lib.lib().nt_depth_cue_factors_device(sc._handle, w, h, C.c_void_p(buf.data_ptr()), C.byref(opts),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _host_factors(sc, w, h):
    out = np.full((h, w, 2), 77, np.float32)
    opts = sup.render_opts(strict_reference=sup.strict_reference())
    _lib.check(_lib.lib().nt_depth_cue_factors(sc._handle, w, h, out.ctypes.data, C.byref(opts)))
    return out


def _assert_factors(got, want, label):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, "%s: the factors differ in %d places, first (y, x, c) = %r: got %r, oracle %r" % (
        label, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _both_forms(sc, w, h, want, label):
    _assert_factors(_host_factors(sc, w, h), want, label + " host")
    raw = _device_factors(sc, w, h)
    _assert_factors(raw[:w * h * 8].view(np.float32).reshape(h, w, 2), want, label + " device")
    assert (raw[w * h * 8:] == SENTINEL).all(), label + ": a byte behind the factors was written"


# ------------------------------------------------------------------ 1. factors
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_factors_equal_the_oracle(case):
    name = case[0]
    cc.check_not_vacuous(name)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        for k in cc.CAMERAS:
            sc._set_camera_arrays(*ph.camera(name, k))
            for tint, background in SETTINGS:
                st = cc.setting(name, tint=tint, background=background)
                _set(sc, st)
                for w, h in cc.SIZES:
                    want = cc.expected(case, w, h, k, st)
                    label = "%s camera %d%s%s %dx%d" % (cc.case_id(case), k, " tint" if tint else "", " background" if background else "", w, h)
                    f, g = want[..., 0], want[..., 1]
                    print("%s: f = 0 / between / 1 / none: %d / %d / %d / %d, g between %d" % (
                        label, int((f == 0).sum()), int(((f > 0) & (f < 1)).sum()), int((f == 1).sum()), int((f < 0).sum()),
                        int(((g > 0) & (g < 1)).sum())))
                    _both_forms(sc, w, h, want, label)


def test_the_python_forms():
    import torch
    case = ("feature5_n5", {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp, k=1)
        st = cc.setting("feature5_n5")
        _set(sc, st)
        want = cc.expected(case, W, H, 1, st)
        got = sc.depth_cue_factors(W, H)
        assert got.dtype == np.float32 and got.shape == (H, W, 2)
        _assert_factors(got, want, "feature5_n5 python host form")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got = sc.depth_cue_factors(W, H, device="cuda")
        stream.synchronize()
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (H, W, 2)
        _assert_factors(got.cpu().numpy(), want, "feature5_n5 python device form")
        # the Python setter hands the same numbers over
        sc.set_depth_cue(float(st["fog_near"]), float(st["fog_far"]), [float(c) for c in st["fog_color"]], float(st["fog_strength"]), False,
                         tint_axis=tracern.Vector(5, [float(v) for v in st["tint_axis"]]), tint_range=(float(st["tint_lo"]), float(st["tint_hi"])),
                         tint_colors=([float(c) for c in st["tint_color_lo"]], [float(c) for c in st["tint_color_hi"]]))
        _assert_factors(sc.depth_cue_factors(W, H), want, "feature5_n5 through set_depth_cue")


# ------------------------------------------------------------------ renders: helpers
def plain_colors(sc, w, h):
    """P: the library's plain fp32 x 3 frame of a scene whose setting is off, [h][w][3] float32, clamped by the packer"""
    assert sc.depth_cue is None
    return sup.render_host(sc, sup.fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h, w, 3)


def _want_rgb(name, P, k=0, **kw):
    st = cc.setting(name, **kw)
    fg = cc.expected((name, {}), P.shape[1], P.shape[0], k, st)
    return cc.blend(P, fg[..., 0], fg[..., 1], st)


# ------------------------------------------------------------------ 2. the routes agree
def test_the_routes_give_equal_factors_and_equal_bytes():
    w, h = cc.BIG
    st = cc.setting("cell120_n4", background=True)
    factors, images = [], []
    for env in ({}, {"NTRACER_FORCE_VAR": "1"}, {"NTRACER_COMPOSITE_KERNEL": "2"}):
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(("cell120_n4", env), mp, k=1)
            _set(sc, st)
            factors.append(_host_factors(sc, w, h))
            images.append([sup.render_host(sc, sup.fmt_of(w, h, chans, rev=rev)) for _, chans, rev in FORMATS])
    _assert_factors(factors[1], factors[0], "NTRACER_FORCE_VAR=1 against the packet walk")
    _assert_factors(factors[2], factors[0], "NTRACER_COMPOSITE_KERNEL=2 against the packet walk")
    _assert_factors(factors[0], cc.expected(("cell120_n4", {}), w, h, 1, st), "cell120_n4 64x48")
    f, g = factors[0][..., 0], factors[0][..., 1]
    assert ((f > 0) & (f < 1)).sum() > 300 and ((g > 0) & (g < 1)).sum() > 300 and (f == 1).sum() > 300
    for k in range(len(FORMATS)):
        assert np.array_equal(images[0][k], images[1][k]) and np.array_equal(images[0][k], images[2][k]), FORMATS[k][0]


# ------------------------------------------------------------------ 3. renders
@pytest.mark.parametrize("scene", cc.RENDERED[:3], ids=lambda s: s[0] + ("," + s[1] if s[1] else ""))
def test_renders_equal_the_plain_frame_blended_by_the_oracles_factors(scene):
    name, variant = scene
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp, variant=variant)
        P = plain_colors(sc, W, H)
        for background in (False, True):
            want_rgb = _want_rgb(name, P, background=background)
            assert (want_rgb != P).any(axis=2).sum() >= 30            # the setting shows
            _set(sc, cc.setting(name, background=background))
            for fname, chans, rev in FORMATS:
                want = sx.pack(want_rgb, chans, rev)
                fmt = sup.fmt_of(W, H, chans, rev=rev)
                img = sup.render_host(sc, fmt)
                assert np.array_equal(img, want), (name, fname, background, "BlockingRenderer", int((img != want).sum()))
                status, img = sup.render_device(sc, fmt)
                assert status == 0 and np.array_equal(img, want), (name, fname, background, "nt_render_device", int((img != want).sum()))
        # fog alone
        want_rgb = _want_rgb(name, P, tint=False)
        _set(sc, cc.setting(name, tint=False))
        assert np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, fx.RGBF32)), sx.pack(want_rgb, fx.RGBF32, False)), (name, "fog alone")
        # a padded pitch keeps its padding
        bpp = 3
        fmt = sup.fmt_of(W, H, RGB24, pitch=W * bpp + 5)
        buf = bytearray(b"\xb3" * (fmt.pitch * H))
        assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
        got = np.frombuffer(bytes(buf), np.uint8).reshape(H, fmt.pitch)
        assert np.array_equal(got[:, :W * bpp], sx.pack(want_rgb, RGB24)) and (got[:, W * bpp:] == 0xb3).all()
        sc.set_depth_cue(None)


# ------------------------------------------------------------------ 4. off, and empty
def test_the_empty_setting_and_the_setting_taken_off_give_the_plain_bytes():
    for name in ("cell120_n4", "feature5_n5"):
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene((name, {}), mp)
            plain = {f[0]: sup.render_host(sc, sup.fmt_of(W, H, f[1], rev=f[2])) for f in FORMATS}
            tiny = {f[0]: sup.render_host(sc, sup.fmt_of(1, 1, f[1], rev=f[2])) for f in FORMATS}
            _set(sc, cc.setting(name, tint=False, background=True, strength=0.0))
            for fname, chans, rev in FORMATS:
                assert np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, chans, rev=rev)), plain[fname]), (name, fname)
                assert np.array_equal(sup.render_host(sc, sup.fmt_of(1, 1, chans, rev=rev)), tiny[fname]), (name, fname, "1 x 1")
            assert len(np.unique(plain["rgbx8"])) > 8
            _set(sc, cc.setting(name, background=True))
            assert not np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, fx.RGBX8)), plain["rgbx8"])
            assert sup.render_host(sc, sup.fmt_of(1, 1, fx.RGBX8)).shape == (1, 4)
            # and taking the setting off again is the plain render
            sc.set_depth_cue(None)
            for fname, chans, rev in FORMATS:
                assert np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, chans, rev=rev)), plain[fname]), (name, fname, "off")


# ------------------------------------------------------------------ 5. frames
@pytest.mark.parametrize("scene", cc.RENDERED, ids=lambda s: s[0] + ("," + s[1] if s[1] else ""))
def test_three_frames_equal_three_single_renders(scene):
    """nt_render_table_device and nt_render_frames_device with a frame_stride larger than a frame: each frame is its single-frame
    render, frame 0 is the oracle's blend, the gap stays as it was"""
    import torch
    name, variant = scene
    nf = 3
    cams = [ph.camera(name, k) for k in range(nf)]
    origins, axes = np.ascontiguousarray(np.stack([c[0] for c in cams])), np.ascontiguousarray(np.stack([c[1] for c in cams]))
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp, variant=variant)
        n = sc.dimension
        P = plain_colors(sc, W, H)
        _set(sc, cc.setting(name, background=True))
        for fname, chans, rev in (FORMATS[0], FORMATS[1]):
            fmt = sup.fmt_of(W, H, chans, rev=rev)
            singles = []
            for o, a in cams:
                sc._set_camera_arrays(o, a)
                singles.append(sup.render_host(sc, fmt))
            singles = np.stack(singles)
            assert np.array_equal(singles[0], sx.pack(_want_rgb(name, P, background=True), chans, rev))
            assert not np.array_equal(singles[0], singles[1])
            table = CameraTable(n, origins, axes)
            frame_bytes = fmt.pitch * H + 64
            buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
            assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().reshape(nf, frame_bytes)
            assert np.array_equal(got[:, :fmt.pitch * H].reshape(nf, H, fmt.pitch), singles), (name, fname, "table")
            assert (got[:, fmt.pitch * H:] == 0x3D).all()
            buf.fill_(0x3D)
            fst = fmt._as_struct()
            _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, nf, origins.ctypes.data_as(_lib.f32p),
                                                          axes.ctypes.data_as(_lib.f32p), C.byref(fst), None,
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            got = buf.cpu().numpy().reshape(nf, frame_bytes)
            assert np.array_equal(got[:, :fmt.pitch * H].reshape(nf, H, fmt.pitch), singles), (name, fname, "frames")
            assert (got[:, fmt.pitch * H:] == 0x3D).all()
            # the table form refuses what the setting excludes, drawing nothing
            buf.fill_(0x3D)
            with pytest.raises(NotImplementedError, match="depth cue"):
                table.render(sc, buf, fmt, frame_bytes=frame_bytes, band_rank=0, band_world=2)
            torch.cuda.synchronize()
            assert bool((buf == 0x3D).all())


# ------------------------------------------------------------------ 6. the scratch cap
# (scene, bytes a pixel of a render, size at which a cap of 1 MiB holds the scratch of one frame and not of two, size at which it
# holds neither a render's frame nor the host form's factors): 16 bytes a pixel on the packet route, 28 elsewhere, and 24 for the
# factors of the host form on either
CAPPED = [("cell120_n4", 16, (256, 160), (320, 240)), ("feature5_n5", 28, (200, 150), (256, 192))]


@pytest.mark.parametrize("name,per_pixel,size,too_big", CAPPED, ids=[c[0] for c in CAPPED])
def test_a_small_scratch_cap_gives_the_same_bytes(name, per_pixel, size, too_big):
    import torch
    w, h = size
    nf = 3
    assert w * h * per_pixel <= (1 << 20) < 2 * w * h * per_pixel
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp)
        n = sc.dimension
        _set(sc, cc.setting(name, background=True))
        table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        fmt = sup.fmt_of(w, h, RGB24)
        frame_bytes = fmt.pitch * h
        images = []
        for mib in (1024, 1):
            sc.set_supersampling_scratch_mb(mib)
            buf = torch.zeros((nf * frame_bytes,), dtype=torch.uint8, device="cuda")
            assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
            torch.cuda.synchronize()
            images.append(buf.cpu().numpy())
        assert np.array_equal(images[0], images[1])
        frames = images[0].reshape(nf, -1)
        assert len(np.unique(images[0])) > 16 and not np.array_equal(frames[0], frames[1])
        sc._set_camera_arrays(*cams[2])
        assert np.array_equal(frames[2].reshape(h, fmt.pitch), sup.render_host(sc, fmt))


@pytest.mark.parametrize("name,per_pixel,size,too_big", CAPPED, ids=[c[0] for c in CAPPED])
def test_a_frame_that_does_not_fit_the_scratch_cap_is_refused_before_anything_is_launched(name, per_pixel, size, too_big):
    w, h = too_big
    assert w * h * per_pixel > (1 << 20) and w * h * 24 > (1 << 20)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp)
        _set(sc, cc.setting(name))
        sc.set_supersampling_scratch_mb(1)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        status, img = sup.render_device(sc, fmt, fill=0x4E)
        assert status == _lib.NT_E_UNSUPPORTED and (img == 0x4E).all()
        assert _lib.last_error().startswith("depth cue") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        with pytest.raises(NotImplementedError, match="depth cue"):
            sc.depth_cue_factors(w, h)
        sc.set_supersampling_scratch_mb(1024)
        assert (sc.depth_cue_factors(w, h)[..., 0] >= 0).sum() > 300


# ------------------------------------------------------------------ 7. abort, 8. capture
@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_an_abort_word_raised_before_the_launch_leaves_the_buffers_untouched(name):
    import torch
    case = (name, {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        st = cc.setting(name)
        _set(sc, st)
        word = torch.ones(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        raw = _device_factors(sc, W, H, abort=word)
        assert (raw == SENTINEL).all()
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word, strict_reference=sup.strict_reference()), fill=0x6A)
        assert status == 0 and (img == 0x6A).all()
        word.zero_()
        torch.cuda.synchronize()
        raw = _device_factors(sc, W, H, abort=word)
        _assert_factors(raw[:W * H * 8].view(np.float32).reshape(H, W, 2), cc.expected(case, W, H, 0, st), name + " after the abort word went down")
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word, strict_reference=sup.strict_reference()), fill=0x6A)
        assert status == 0 and np.array_equal(img, sup.render_host(sc, fmt))


@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_two_calls_in_a_row_agree_and_a_warm_table_render_is_capturable(name):
    """after a warm-up call of the same shape a table render with the setting on only enqueues -- no allocation, no read-back --:
    captured into a HIP graph on one stream and replayed, it gives the direct call's bytes"""
    import torch
    nf = 2
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene((name, {}), mp)
        n = sc.dimension
        _set(sc, cc.setting(name, background=True))
        a, b = _device_factors(sc, W, H), _device_factors(sc, W, H)
        assert np.array_equal(a, b)
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        assert np.array_equal(sup.render_host(sc, fmt), sup.render_host(sc, fmt))
        fst = fmt._as_struct()
        tab = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        st = torch.cuda.Stream()
        ref = torch.zeros((nf, H * fmt.pitch), dtype=torch.uint8, device="cuda")
        fb = torch.zeros_like(ref)

        def call(buf):
            return _lib.lib().nt_render_table_device(sc._handle, C.c_void_p(buf.data_ptr()), H * fmt.pitch, tab._h, 0, nf, C.byref(fst), None,
                                                     C.c_void_p(st.cuda_stream))
        with torch.cuda.stream(st):
            _lib.check(call(ref))
        st.synchronize()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            _lib.check(call(fb))
        fb.zero_()
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(fb, ref)
        del gr
        sc._set_camera_arrays(*cams[1])
        assert np.array_equal(ref[1].cpu().numpy().reshape(H, fmt.pitch), sup.render_host(sc, fmt))


# ------------------------------------------------------------------ 9. refusals, and the calls that ignore the setting
def test_the_python_surface_refuses_what_the_setting_excludes():
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(("cell120_n4", {}), mp)
        _set(sc, cc.setting("cell120_n4"))
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        size = fmt.pitch * H

        def refused(**kw):
            buf = bytearray(b"\x4e" * size)
            with pytest.raises(NotImplementedError, match="depth cue"):
                ntracer_amd.BlockingRenderer().render(buf, fmt, sc, **kw)
            assert bytes(buf) == b"\x4e" * size

        sc.set_supersampling(2)
        refused()
        sc.set_adaptive_supersampling(0.1)
        refused()
        sc.set_adaptive_supersampling(None)
        sc.set_supersampling(1)
        sc.set_ambient_occlusion(4, 1.0)
        refused()
        sc.set_ambient_occlusion(None)
        sc.set_outlines()
        refused()
        sc.set_outlines(None)
        sc.set_lens(tracern.Lens.pinhole(W, H, 0.8))
        refused()
        sc.set_lens(None)
        sc.set_parallel_projection(2.0)
        refused()
        sc.set_parallel_projection(None)
        refused(band_rank=0, band_world=2)
        refused(collect_stats=True)
        # and with nothing in the way it draws
        assert len(np.unique(sup.render_host(sc, fmt))) > 8


def test_the_probes_the_hits_and_the_masks_ignore_the_setting():
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = _scene(("cell120_n4", {}), mp), _scene(("cell120_n4", {}), mp)
        _set(sc, cc.setting("cell120_n4", background=True))
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        rng = np.random.default_rng(5)
        xs, ys = rng.integers(0, W, 60), rng.integers(0, H, 60)
        assert np.array_equal(sc.colors_at(xs, ys, W, H).view(np.uint32), plain.colors_at(xs, ys, W, H).view(np.uint32))
        got, want = sc.primary_hits(W, H, normals=True), plain.primary_hits(W, H, normals=True)
        assert np.array_equal(got.hits, want.hits) and np.array_equal(got.normal_dir.view(np.uint32), want.normal_dir.view(np.uint32))
        origin, _ = ph.camera("cell120_n4", 0)
        d = np.ascontiguousarray(ph.rays("cell120_n4", W, H, 0)[0].reshape(W * H, 4), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float32), d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
        for s in (sc, plain):
            s.set_outlines()
        assert np.array_equal(sc.outline_mask(W, H), plain.outline_mask(W, H)) and plain.outline_mask(W, H).any()
        for s in (sc, plain):
            s.set_outlines(None)
            s.set_adaptive_supersampling(0.1)
            s.set_ambient_occlusion(4, 1.0)
        assert np.array_equal(sc.refinement_mask(W, H), plain.refinement_mask(W, H))
        assert np.array_equal(sc.occlusion_counts(W, H), plain.occlusion_counts(W, H))
