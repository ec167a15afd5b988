"""Outlines (scene.set_outlines, scene.outline_mask, nt_outline_mask*, and the renders that honour the setting) on the GPU against
the oracle.

The expected masks never come from the library: tests/outline_cases.py works them out for every pixel from the oracle's
primary-hit records and normals, by the definition in include/ntracer_hip.h.  Masks must be equal, no tolerance: DESIGN.md 4.4 and
4.5 measured these walks and hit_normal as bit-equal to the oracle, and test_outlines_host.py keeps every tested pair a relative
1e-2 away from the crease threshold.  A render with the setting on must be, byte for byte, the library's own plain fp32 x 3 frame
P (pinned to the oracle by the existing suite) blended with the colour where the oracle's mask is set, packed by the oracle's
pack_pixel.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C
import os

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import outline_cases as oc
import primary_hit_cases as ph
import ray_color_cases as rc
import ray_query_cases as rq
import ss_expected as sx
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
PAD = 29                        # bytes behind the mask
W, H = 37, 21
COLOR, STRENGTH = (0.9, 0.2, 0.1), 0.75
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# (name, channels, reversed): 4-, 3-, 6- and 12-byte pixels, and a reversed one
FORMATS = [("rgbx8", fx.RGBX8, False), ("rgb24", RGB24, False), ("rgb16", fx.RGB16, False), ("rgbf32", fx.RGBF32, False),
           ("rgb24-reversed", RGB24, True)]


def _scene(case, mp, k=0, variant=""):
    name, env = case
    for key in oc.SWITCHES:
        mp.delenv(key, raising=False)
    for key, v in env.items():
        mp.setenv(key, v)
    n, flat, params = rc.case_scene((name, env, variant))
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(params)
    sc.set_fov(ph.fov_of(name))
    sc._set_camera_arrays(*ph.camera(name, k))
    return sc


def _set(sc, params=oc.A, color=COLOR, strength=STRENGTH):
    """the setting through the ABI: crease_cos as given, not through an angle"""
    col = (C.c_float * 3)(*color)
    _lib.check(_lib.lib().nt_scene_set_outlines(sc._handle, 1, params[0], params[1], col, strength))


def _opts(abort=None):
    opts = _lib.NtRenderOpts()
    opts.device = -1
    opts.strict_reference = 1 if os.environ.get("NTRACER_STRICT_REFERENCE", "0") not in ("", "0") else 0
    if abort is not None:
        opts.abort_device = abort.data_ptr()
    return opts


def _device_mask(sc, w, h, abort=None):
    """nt_outline_mask_device on a sentinel-filled buffer with PAD bytes behind it: the raw buffer"""
    import torch
    buf = torch.full((w * h + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    opts = _opts(abort)
    _lib.check(_lib.lib().nt_outline_mask_device(sc._handle, w, h, C.c_void_p(buf.data_ptr()), C.byref(opts),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _host_mask(sc, w, h):
    """nt_outline_mask: (mask, marked)"""
    mask = np.full((h, w), 0xEE, np.uint8)
    marked = C.c_longlong(-1)
    opts = _opts()
    _lib.check(_lib.lib().nt_outline_mask(sc._handle, w, h, mask.ctypes.data, C.byref(marked), C.byref(opts)))
    return mask, int(marked.value)


def _assert_mask(got, want, label):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: the masks differ on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
        label, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _both_forms(sc, w, h, want, label):
    got, marked = _host_mask(sc, w, h)
    _assert_mask(got, want, label + " host")
    assert marked == int((want != 0).sum()), label
    raw = _device_mask(sc, w, h)
    _assert_mask(raw[:w * h].reshape(h, w), want, label + " device")
    assert (raw[w * h:] == SENTINEL).all(), label + ": a byte behind the mask was written"


# ------------------------------------------------------------------ 1. masks
@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_masks_equal_the_oracle(case):
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        for label, params in oc.PARAMS:
            _set(sc, params)
            for w, h in oc.sizes(case):
                want, c = oc.expected(case, w, h, params)
                print("%s %s %dx%d: marked %d (silhouette %d, crease %d, depth %d pairs)" % (
                    oc.case_id(case), label, w, h, int((want != 0).sum()), c["silhouette"], c["crease"], c["depth"]))
                _both_forms(sc, w, h, want, "%s %s %dx%d" % (oc.case_id(case), label, w, h))


def test_the_python_forms():
    import torch
    case = ("feature5_n5", {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        sc.set_outlines(oc.crease_angle(oc.A[0]), oc.A[1])
        want = oc.expected(case, W, H, oc.A)[0]
        got = sc.outline_mask(W, H)
        assert got.dtype == np.uint8 and got.shape == (H, W)
        _assert_mask(got, want, "feature5_n5 python host form")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = sc.outline_mask(W, H, device="cuda")
        st.synchronize()
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (H, W)
        _assert_mask(got.cpu().numpy(), want, "feature5_n5 python device form")


# ------------------------------------------------------------------ renders: helpers
def fmt_of(w, h, chans, pitch=0, rev=False):
    return ntracer_amd.ImageFormat(w, h, [ntracer_amd.Channel(*c) for c in chans], pitch, rev)


def render_host(scene, fmt, **kw):
    buf = bytearray(fmt.pitch * fmt.height)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, scene, **kw)
    return np.frombuffer(bytes(buf), np.uint8).reshape(fmt.height, fmt.pitch)


def plain_colors(sc, w, h):
    """P: the library's plain fp32 x 3 frame of a scene whose setting is off, [h][w][3] float32, clamped by the packer"""
    assert sc.outlines is None
    return render_host(sc, fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h, w, 3)


def render_device(sc, fmt, opts=None, fill=0x3D):
    import torch
    size = fmt.pitch * fmt.height
    buf = torch.full((size + 16,), fill, dtype=torch.uint8, device="cuda")
    fst = fmt._as_struct()
    status = _lib.lib().nt_render_device(sc._handle, C.c_void_p(buf.data_ptr()), size, C.byref(fst), None if opts is None else C.byref(opts),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[size:] == fill).all()
    return status, got[:size].reshape(fmt.height, fmt.pitch)


# ------------------------------------------------------------------ 2. the routes agree
def test_the_routes_give_equal_masks_and_equal_bytes():
    w, h = oc.BIG
    masks, images = [], []
    for env in ({}, {"NTRACER_FORCE_VAR": "1"}, {"NTRACER_COMPOSITE_KERNEL": "2"}):
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(("cell120_n4", env), mp)
            _set(sc)
            masks.append(_host_mask(sc, w, h)[0])
            images.append([render_host(sc, fmt_of(w, h, chans, rev=rev)) for _, chans, rev in FORMATS])
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2])
    _assert_mask(masks[0], oc.expected(("cell120_n4", {}), w, h)[0], "cell120_n4 64x48")
    assert (masks[0] != 0).sum() > 500
    for k in range(len(FORMATS)):
        assert np.array_equal(images[0][k], images[1][k]) and np.array_equal(images[0][k], images[2][k]), FORMATS[k][0]


# ------------------------------------------------------------------ 3. renders
@pytest.mark.parametrize("name", ["feature5_n5", "cell120_n4"])
def test_renders_equal_the_plain_frame_blended_by_the_oracles_mask(name):
    case = (name, {})
    mask = oc.expected(case, W, H)[0]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        P = plain_colors(sc, W, H)
        want_rgb = oc.blend(P, mask, COLOR, STRENGTH)
        assert (want_rgb != P).any(axis=2).sum() >= 30            # the setting shows
        _set(sc)
        for fname, chans, rev in FORMATS:
            want = sx.pack(want_rgb, chans, rev)
            fmt = fmt_of(W, H, chans, rev=rev)
            img = render_host(sc, fmt)
            assert np.array_equal(img, want), (name, fname, "BlockingRenderer", int((img != want).sum()))
            status, img = render_device(sc, fmt)
            assert status == 0 and np.array_equal(img, want), (name, fname, "nt_render_device", int((img != want).sum()))
        # a padded pitch keeps its padding
        bpp = 3
        fmt = fmt_of(W, H, RGB24, pitch=W * bpp + 5)
        buf = bytearray(b"\xb3" * (fmt.pitch * H))
        assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
        got = np.frombuffer(bytes(buf), np.uint8).reshape(H, fmt.pitch)
        assert np.array_equal(got[:, :W * bpp], sx.pack(want_rgb, RGB24)) and (got[:, W * bpp:] == 0xb3).all()


def test_strength_zero_and_an_all_zero_mask_give_the_plain_bytes():
    for name in ("cell120_n4", "feature5_n5"):
        case = (name, {})
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp)
            plain = {f[0]: render_host(sc, fmt_of(W, H, f[1], rev=f[2])) for f in FORMATS}
            tiny = {f[0]: render_host(sc, fmt_of(1, 1, f[1], rev=f[2])) for f in FORMATS}
            _set(sc, strength=0.0)
            for fname, chans, rev in FORMATS:
                assert np.array_equal(render_host(sc, fmt_of(W, H, chans, rev=rev)), plain[fname]), (name, fname)
            assert len(np.unique(plain["rgbx8"])) > 8
            _set(sc, strength=1.0)
            assert not np.array_equal(render_host(sc, fmt_of(W, H, fx.RGBX8)), plain["rgbx8"])
            for fname, chans, rev in FORMATS:
                assert np.array_equal(render_host(sc, fmt_of(1, 1, chans, rev=rev)), tiny[fname]), (name, fname, "1 x 1")
            # and taking the setting off again is the plain render
            sc.set_outlines(None)
            assert np.array_equal(render_host(sc, fmt_of(W, H, fx.RGBX8)), plain["rgbx8"])


# ------------------------------------------------------------------ 4. frames
@pytest.mark.parametrize("scene", oc.RENDERED, ids=lambda s: s[0] + ("," + s[1] if s[1] else ""))
def test_three_frames_equal_three_single_renders(scene):
    """nt_render_table_device and nt_render_frames_device with a frame_stride larger than a frame: each frame is its single-frame
    render -- a neighbour read across a frame boundary would show here --, frame 0 is the oracle's blend, the gap stays as it was"""
    import torch
    name, variant = scene
    case = (name, {})
    nf = 3
    cams = [ph.camera(name, k) for k in range(nf)]
    origins, axes = np.ascontiguousarray(np.stack([c[0] for c in cams])), np.ascontiguousarray(np.stack([c[1] for c in cams]))
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp, variant=variant)
        n = sc.dimension
        P = plain_colors(sc, W, H)
        _set(sc)
        for fname, chans, rev in (FORMATS[0], FORMATS[1]):
            fmt = fmt_of(W, H, chans, rev=rev)
            singles = []
            for o, a in cams:
                sc._set_camera_arrays(o, a)
                singles.append(render_host(sc, fmt))
            singles = np.stack(singles)
            assert np.array_equal(singles[0], sx.pack(oc.blend(P, oc.expected(case, W, H)[0], COLOR, STRENGTH), chans, rev))
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
            with pytest.raises(NotImplementedError, match="outlines"):
                table.render(sc, buf, fmt, frame_bytes=frame_bytes, band_rank=0, band_world=2)
            torch.cuda.synchronize()
            assert bool((buf == 0x3D).all())


# ------------------------------------------------------------------ 5. the scratch cap, abort
# (scene, bytes a pixel of a render, size at which a cap of 1 MiB holds the scratch of one frame and not of two, size at which it
# holds neither a render's frame nor the mask's alone): 16 bytes a pixel on the packet route, 29 + 4 n elsewhere, and 17 and
# 17 + 4 n for the mask alone
CAPPED = [("cell120_n4", 16, (256, 160), (320, 240)), ("feature5_n5", 29 + 4 * 5, (128, 96), (200, 150))]


@pytest.mark.parametrize("name,per_pixel,size,too_big", CAPPED, ids=[c[0] for c in CAPPED])
def test_a_small_scratch_cap_gives_the_same_bytes(name, per_pixel, size, too_big):
    import torch
    case = (name, {})
    w, h = size
    nf = 3
    assert w * h * per_pixel <= (1 << 20) < 2 * w * h * per_pixel
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        n = sc.dimension
        _set(sc)
        table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        fmt = fmt_of(w, h, RGB24)
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
        assert np.array_equal(frames[2].reshape(h, fmt.pitch), render_host(sc, fmt))


@pytest.mark.parametrize("name,per_pixel,size,too_big", CAPPED, ids=[c[0] for c in CAPPED])
def test_a_frame_that_does_not_fit_the_scratch_cap_is_refused_before_anything_is_launched(name, per_pixel, size, too_big):
    case = (name, {})
    w, h = too_big
    assert w * h * per_pixel > (1 << 20) and w * h * (per_pixel - 12 if per_pixel > 16 else 17) > (1 << 20)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _set(sc)
        sc.set_supersampling_scratch_mb(1)
        fmt = fmt_of(w, h, fx.RGBX8)
        status, img = render_device(sc, fmt, fill=0x4E)
        assert status == _lib.NT_E_UNSUPPORTED and (img == 0x4E).all()
        assert _lib.last_error().startswith("outlines") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        with pytest.raises(NotImplementedError, match="outlines"):
            sc.outline_mask(w, h)
        sc.set_supersampling_scratch_mb(1024)
        assert (sc.outline_mask(w, h) != 0).sum() > 300


@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_an_abort_word_raised_before_the_launch_leaves_the_buffers_untouched(name):
    import torch
    case = (name, {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _set(sc)
        word = torch.ones(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        raw = _device_mask(sc, W, H, abort=word)
        assert (raw == SENTINEL).all()
        fmt = fmt_of(W, H, fx.RGBX8)
        status, img = render_device(sc, fmt, opts=_opts(word), fill=0x6A)
        assert status == 0 and (img == 0x6A).all()
        word.zero_()
        torch.cuda.synchronize()
        raw = _device_mask(sc, W, H, abort=word)
        _assert_mask(raw[:W * H].reshape(H, W), oc.expected(case, W, H)[0], name + " after the abort word went down")
        status, img = render_device(sc, fmt, opts=_opts(word), fill=0x6A)
        assert status == 0 and np.array_equal(img, render_host(sc, fmt))


@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_two_calls_in_a_row_agree_and_a_warm_table_render_is_capturable(name):
    """after a warm-up call of the same shape a table render with the setting on only enqueues -- no allocation, no read-back --:
    captured into a HIP graph on one stream and replayed, it gives the direct call's bytes"""
    import torch
    case = (name, {})
    nf = 2
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        n = sc.dimension
        _set(sc)
        a, b = _device_mask(sc, W, H), _device_mask(sc, W, H)
        assert np.array_equal(a, b)
        fmt = fmt_of(W, H, fx.RGBX8)
        assert np.array_equal(render_host(sc, fmt), render_host(sc, fmt))
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
        assert np.array_equal(ref[1].cpu().numpy().reshape(H, fmt.pitch), render_host(sc, fmt))


# ------------------------------------------------------------------ 6. refusals, and the calls that ignore the setting
def test_the_python_surface_refuses_what_the_setting_excludes():
    case = ("cell120_n4", {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        sc.set_outlines()
        fmt = fmt_of(W, H, fx.RGBX8)
        size = fmt.pitch * H

        def refused(**kw):
            buf = bytearray(b"\x4e" * size)
            with pytest.raises(NotImplementedError, match="outlines"):
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
        sc.set_lens(tracern.Lens.pinhole(W, H, 0.8))
        refused()
        sc.set_lens(None)
        sc.set_parallel_projection(2.0)
        refused()
        sc.set_parallel_projection(None)
        refused(band_rank=0, band_world=2)
        refused(collect_stats=True)
        # and with nothing in the way it draws
        assert len(np.unique(render_host(sc, fmt))) > 8


def test_the_probes_the_hits_and_the_other_masks_ignore_the_setting():
    case = ("cell120_n4", {})
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = _scene(case, mp), _scene(case, mp)
        _set(sc)
        fmt = fmt_of(W, H, fx.RGBX8)
        assert not np.array_equal(render_host(sc, fmt), render_host(plain, fmt))
        rng = np.random.default_rng(5)
        xs, ys = rng.integers(0, W, 60), rng.integers(0, H, 60)
        assert np.array_equal(sc.colors_at(xs, ys, W, H).view(np.uint32), plain.colors_at(xs, ys, W, H).view(np.uint32))
        got, want = sc.primary_hits(W, H, normals=True), plain.primary_hits(W, H, normals=True)
        assert np.array_equal(got.hits, want.hits) and np.array_equal(got.normal_dir.view(np.uint32), want.normal_dir.view(np.uint32))
        for s in (sc, plain):
            s.set_adaptive_supersampling(0.1)
            s.set_ambient_occlusion(4, 1.0)
        assert np.array_equal(sc.refinement_mask(W, H), plain.refinement_mask(W, H))
        assert np.array_equal(sc.occlusion_counts(W, H), plain.occlusion_counts(W, H))
        origin, _ = ph.camera("cell120_n4", 0)
        d = np.ascontiguousarray(ph.rays("cell120_n4", W, H, 0)[0].reshape(W * H, 4), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float32), d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
