"""BoxScene face lines (BoxScene.set_face_lines, face_line_mask, nt_box_line_mask*, and the renders that honour the setting) on the
GPU against the oracle.

The expected masks never come from the library: tests/box_hit_cases.py works them out for every pixel from the oracle's
primary_dir by the rules of include/ntracer_hip.h.  Masks must be equal, no tolerance.  A render with the setting on must be,
byte for byte, the library's own plain fp32 x 3 frame P (pinned to the oracle by the existing suite, and here against the
expected colours once more) blended with the colour where the oracle's mask is set, packed by the oracle's pack_pixel -- on the
fused kernel and, under NTRACER_FORCE_VAR=1 and above 24 dimensions, on the two passes at run-time n.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import box_hit_cases as bc
import fixtures as fx
import ntracer_amd
import outline_cases as oc
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a
PAD = 29                        # bytes behind the mask
COLOR = (0.9, 0.2, 0.1)
FORMATS = [("rgbx8", fx.RGBX8), ("rgb16", fx.RGB16), ("rgbf32", fx.RGBF32)]
# (dimension, switches): the fused kernel at the bench's dimension, at one with a second tile kernel behind the plain render and
# at the last compiled one; the two passes at run-time n under the switch and at their own dimensions
ROUTES = [(6, {}), (10, {}), (24, {}), (6, {"NTRACER_FORCE_VAR": "1"}), (10, {"NTRACER_FORCE_VAR": "1"}), (25, {}), (64, {})]
route_id = lambda r: "n%d%s" % (r[0], "-force-var" if r[1] else "")


def scene(n, k, mp, env=None):
    sup.set_switches(mp, ("NTRACER_FORCE_VAR",), env or {})
    sc = tracern.BoxScene(n)
    sc.set_fov(bc.FOV)
    sc._set_camera_arrays(*bc.camera(n, k))
    return sc


def _set(sc, kinds=3, color=COLOR, strength=0.75):
    col = (C.c_float * 3)(*color)
    _lib.check(_lib.lib().nt_scene_set_box_lines(sc._handle, kinds, col, strength))


def _device_mask(sc, w, h, abort=None):
    """nt_box_line_mask_device on a sentinel-filled buffer with PAD bytes behind it: the raw buffer"""
    import torch
    buf = torch.full((w * h + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    opts = sup.render_opts(abort)
    _lib.check(_lib.lib().nt_box_line_mask_device(sc._handle, w, h, C.c_void_p(buf.data_ptr()), C.byref(opts),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _host_mask(sc, w, h):
    mask = np.full((h, w), 0xEE, np.uint8)
    marked = C.c_longlong(-1)
    opts = sup.render_opts()
    _lib.check(_lib.lib().nt_box_line_mask(sc._handle, w, h, mask.ctypes.data, C.byref(marked), C.byref(opts)))
    return mask, int(marked.value)


def _assert_mask(got, want, label):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: the masks differ on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
        label, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------ 1. masks
@pytest.mark.parametrize("route", [(n, {}) for n in bc.DIMS] + [(6, {"NTRACER_FORCE_VAR": "1"}), (10, {"NTRACER_FORCE_VAR": "1"})], ids=route_id)
def test_masks_equal_the_oracle(route):
    n, env = route
    with pytest.MonkeyPatch.context() as mp:
        for v in bc.views(n):
            _, k, (w, h) = v
            sc = scene(n, k, mp, env)
            full = bc.expected(n, k, w, h)["mask"]
            for kinds in (1, 2, 3):
                _set(sc, kinds)
                want = full & np.uint8(kinds)
                label = "%s%s kinds %d" % (bc.view_id(v), " force-var" if env else "", kinds)
                got, marked = _host_mask(sc, w, h)
                _assert_mask(got, want, label + " host")
                assert marked == int((want != 0).sum()), label
                raw = _device_mask(sc, w, h)
                _assert_mask(raw[:w * h].reshape(h, w), want, label + " device")
                assert (raw[w * h:] == SENTINEL).all(), label + ": a byte behind the mask was written"


def test_the_python_forms():
    import torch
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, k, mp)
        sc.set_face_lines(edges=False)
        want = bc.expected(n, k, w, h)["mask"]
        got = sc.face_line_mask(w, h)
        assert got.dtype == np.uint8 and got.shape == (h, w)
        _assert_mask(got, want & 1, "python host form, silhouette alone")
        sc.set_face_lines()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = sc.face_line_mask(w, h, device="cuda")
        st.synchronize()
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (h, w)
        _assert_mask(got.cpu().numpy(), want, "python device form")
        # the mask is one sample a pixel whatever the supersampling factor says
        sc.set_supersampling(2)
        _assert_mask(sc.face_line_mask(w, h), want, "supersampling 2")


# ------------------------------------------------------------------ renders: helpers
def plain_colors(sc, w, h):
    """P: the library's plain fp32 x 3 frame of a scene whose setting is off, [h][w][3] float32, clamped by the packer"""
    assert sc.face_lines is None
    return sup.render_host(sc, sup.fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h, w, 3)


# ------------------------------------------------------------------ 2. renders
@pytest.mark.parametrize("route", ROUTES, ids=route_id)
def test_renders_equal_the_plain_frame_blended_by_the_oracles_mask(route):
    """strength 0: the bytes of the plain render of the same view; 1 and 0.5: outline_cases.blend of the plain fp32 frame packed by
    the oracle -- in RGBX8, RGB16 and RGBF32, the host and the device form, at every size of the cases"""
    n, env = route
    with pytest.MonkeyPatch.context() as mp:
        for k in (2, 4):
            for w, h in bc.ALL_SIZES:
                sc = scene(n, k, mp, env)
                e = bc.expected(n, k, w, h)
                P = plain_colors(sc, w, h)
                clamped = np.clip(e["colors"], np.float32(0), np.float32(1))
                assert np.array_equal(P.view(np.uint32), clamped.view(np.uint32)), "the plain frame is not the expected colours"
                plain = {name: sup.render_host(sc, sup.fmt_of(w, h, chans)) for name, chans in FORMATS}
                label = "n%d %s %dx%d%s" % (n, bc.CAMERA_NAMES[k], w, h, " force-var" if env else "")
                for strength in (0.0, 1.0, 0.5):
                    _set(sc, 3, COLOR, strength)
                    want_rgb = oc.blend(P, e["mask"], COLOR, strength)
                    if strength > 0 and w * h > 60:
                        assert (want_rgb != P).any(axis=2).sum() >= 10, label          # the setting shows
                    for name, chans in FORMATS:
                        want = plain[name] if strength == 0.0 else sx.pack(want_rgb, chans)
                        fmt = sup.fmt_of(w, h, chans)
                        img = sup.render_host(sc, fmt)
                        assert np.array_equal(img, want), (label, name, strength, "BlockingRenderer", int((img != want).sum()))
                        status, img = sup.render_device(sc, fmt)
                        assert status == 0 and np.array_equal(img, want), (label, name, strength, "nt_render_device", int((img != want).sum()))
                sc.set_face_lines(None)
                assert np.array_equal(sup.render_host(sc, sup.fmt_of(w, h, fx.RGBX8)), plain["rgbx8"]), label + ": off again"


def test_each_kind_alone_and_other_formats():
    """silhouette or edges alone draw their own pixels; a 3-byte pixel, a reversed one and a padded pitch go through the generic
    packer and keep the padding"""
    RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        for env in ({}, {"NTRACER_FORCE_VAR": "1"}):
            sc = scene(n, k, mp, env)
            P = plain_colors(sc, w, h)
            mask = bc.expected(n, k, w, h)["mask"]
            for kinds in (1, 2):
                _set(sc, kinds, COLOR, 1.0)
                want_rgb = oc.blend(P, mask & np.uint8(kinds), COLOR, 1.0)
                for chans, rev in ((fx.RGBX8, False), (RGB24, False), (RGB24, True)):
                    img = sup.render_host(sc, sup.fmt_of(w, h, chans, rev=rev))
                    assert np.array_equal(img, sx.pack(want_rgb, chans, rev)), (env, kinds, chans, rev)
            fmt = sup.fmt_of(w, h, RGB24, pitch=w * 3 + 5)
            buf = bytearray(b"\xb3" * (fmt.pitch * h))
            assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
            got = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
            assert np.array_equal(got[:, :w * 3], sx.pack(want_rgb, RGB24)) and (got[:, w * 3:] == 0xb3).all()


# ------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("route", [(6, {}), (6, {"NTRACER_FORCE_VAR": "1"}), (6, {"NTRACER_FORCE_VAR": "1", "NTRACER_CHUNK_FRAMES": "2"}), (25, {})],
                         ids=lambda r: "n%d%s" % (r[0], "".join("-" + k[8:].lower() for k in sorted(r[1]))))
def test_three_frames_equal_three_single_renders(route):
    """nt_render_table_device and nt_render_frames_device with a frame_stride larger than a frame: each frame is its single-frame
    render -- a line drawn across a frame boundary would show here --, the gap stays as it was"""
    import torch
    n, env = route
    nf = 3
    ks = (2, 4, 0)
    cams = [bc.camera(n, k) for k in ks]
    origins, axes = np.ascontiguousarray(np.stack([c[0] for c in cams])), np.ascontiguousarray(np.stack([c[1] for c in cams]))
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, ks[0], mp, env)
        for w, h in ((37, 21), bc.BIG):
            sc.set_face_lines(None)
            sc._set_camera_arrays(*cams[0])
            P = plain_colors(sc, w, h)
            _set(sc)
            for name, chans in FORMATS[:2]:
                fmt = sup.fmt_of(w, h, chans)
                singles = []
                for o, a in cams:
                    sc._set_camera_arrays(o, a)
                    singles.append(sup.render_host(sc, fmt))
                singles = np.stack(singles)
                assert np.array_equal(singles[0], sx.pack(oc.blend(P, bc.expected(n, ks[0], w, h)["mask"], COLOR, 0.75), chans))
                assert not np.array_equal(singles[0], singles[1])
                table = CameraTable(n, origins, axes)
                frame_bytes = fmt.pitch * h + 64
                buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
                assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
                torch.cuda.synchronize()
                got = buf.cpu().numpy().reshape(nf, frame_bytes)
                assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (route_id(route), name, "table")
                assert (got[:, fmt.pitch * h:] == 0x3D).all()
                buf.fill_(0x3D)
                fst = fmt._as_struct()
                _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, nf, origins.ctypes.data_as(_lib.f32p),
                                                              axes.ctypes.data_as(_lib.f32p), C.byref(fst), None,
                                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                got = buf.cpu().numpy().reshape(nf, frame_bytes)
                assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (route_id(route), name, "frames")
                assert (got[:, fmt.pitch * h:] == 0x3D).all()
                # the table form refuses what the setting excludes, drawing nothing
                buf.fill_(0x3D)
                with pytest.raises(NotImplementedError, match="face lines"):
                    table.render(sc, buf, fmt, frame_bytes=frame_bytes, band_rank=0, band_world=2)
                torch.cuda.synchronize()
                assert bool((buf == 0x3D).all())


# ------------------------------------------------------------------ 4. the scratch cap of the run-time-n route, abort
def test_a_small_scratch_cap_gives_the_same_bytes_and_a_frame_that_does_not_fit_is_refused():
    """16 bytes a pixel and frame at run-time n: 256 x 160 fits a cap of 1 MiB once and not twice, 320 x 240 not at all; the fused
    kernel needs no scratch and draws either"""
    import torch
    n, nf = 6, 3
    cams = [bc.camera(n, k) for k in (2, 4, 0)]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, 2, mp, {"NTRACER_FORCE_VAR": "1"})
        _set(sc)
        table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        w, h = 256, 160
        assert w * h * 16 <= (1 << 20) < 2 * w * h * 16
        fmt = sup.fmt_of(w, h, fx.RGBX8)
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
        # the fused kernel draws the same frames
        mp.delenv("NTRACER_FORCE_VAR")
        buf = torch.zeros((nf * frame_bytes,), dtype=torch.uint8, device="cuda")
        assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), images[0])
        # too big for the cap: refused before anything is launched, at run-time n alone
        w, h = 320, 240
        assert w * h * 16 > (1 << 20)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        status, fused = sup.render_device(sc, fmt, fill=0x4E)
        assert status == 0 and len(np.unique(fused)) > 16
        mp.setenv("NTRACER_FORCE_VAR", "1")
        status, img = sup.render_device(sc, fmt, fill=0x4E)
        assert status == _lib.NT_E_UNSUPPORTED and (img == 0x4E).all()
        assert _lib.last_error().startswith("face lines") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        with pytest.raises(NotImplementedError, match="face lines"):
            sc.face_line_mask(w, h)
        sc.set_supersampling_scratch_mb(1024)
        status, img = sup.render_device(sc, fmt, fill=0x4E)
        assert status == 0 and np.array_equal(img, fused)


@pytest.mark.parametrize("env", ({}, {"NTRACER_FORCE_VAR": "1"}), ids=("", "force-var"))
def test_an_abort_word_raised_before_the_launch_leaves_the_buffers_untouched(env):
    import torch
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, k, mp, env)
        _set(sc)
        word = torch.ones(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        raw = _device_mask(sc, w, h, abort=word)
        assert (raw == SENTINEL).all()
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word), fill=0x6A)
        assert status == 0 and (img == 0x6A).all()
        word.zero_()
        torch.cuda.synchronize()
        raw = _device_mask(sc, w, h, abort=word)
        _assert_mask(raw[:w * h].reshape(h, w), bc.expected(n, k, w, h)["mask"], "after the abort word went down")
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word), fill=0x6A)
        assert status == 0 and np.array_equal(img, sup.render_host(sc, fmt))


def test_a_warm_table_render_is_capturable():
    """the fused kernel allocates nothing: a table render with the setting on, captured into a HIP graph on one stream and
    replayed, gives the direct call's bytes"""
    import torch
    n, nf, (w, h) = 6, 2, (37, 21)
    cams = [bc.camera(n, k) for k in (2, 4)]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, 2, mp)
        _set(sc)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        fst = fmt._as_struct()
        tab = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        st = torch.cuda.Stream()
        ref = torch.zeros((nf, h * fmt.pitch), dtype=torch.uint8, device="cuda")
        fb = torch.zeros_like(ref)

        def call(buf):
            return _lib.lib().nt_render_table_device(sc._handle, C.c_void_p(buf.data_ptr()), h * fmt.pitch, tab._h, 0, nf, C.byref(fst), None,
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
        assert np.array_equal(ref[1].cpu().numpy().reshape(h, fmt.pitch), sup.render_host(sc, fmt))


# ------------------------------------------------------------------ 5. refusals, and the calls that ignore the setting
def test_the_python_surface_refuses_what_the_setting_excludes():
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, k, mp)
        sc.set_face_lines()
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        size = fmt.pitch * h

        def refused(**kw):
            buf = bytearray(b"\x4e" * size)
            with pytest.raises(NotImplementedError, match="face lines"):
                ntracer_amd.BlockingRenderer().render(buf, fmt, sc, **kw)
            assert bytes(buf) == b"\x4e" * size

        sc.set_supersampling(2)
        refused()
        sc.set_adaptive_supersampling(0.1)
        refused()
        sc.set_adaptive_supersampling(None)
        sc.set_supersampling(1)
        sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
        refused()
        sc.set_lens(None)
        sc.set_parallel_projection(2.0)
        refused()
        sc.set_parallel_projection(None)
        refused(band_rank=0, band_world=2)
        refused(collect_stats=True)
        # and with nothing in the way it draws
        assert len(np.unique(sup.render_host(sc, fmt))) > 8


def test_the_probes_the_rays_and_the_other_mask_ignore_the_setting():
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = scene(n, k, mp), scene(n, k, mp)
        _set(sc)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        rng = np.random.default_rng(5)
        xs, ys = rng.integers(0, w, 60), rng.integers(0, h, 60)
        assert np.array_equal(sc.colors_at(xs, ys, w, h).view(np.uint32), plain.colors_at(xs, ys, w, h).view(np.uint32))
        assert np.array_equal(sc.face_hits(w, h).records, plain.face_hits(w, h).records)
        e = bc.expected(n, k, w, h)
        d = np.ascontiguousarray(e["dirs"].reshape(w * h, n), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(bc.camera(n, k)[0], d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
        for s in (sc, plain):
            s.set_supersampling(2)
            s.set_adaptive_supersampling(0.1)
        assert np.array_equal(sc.refinement_mask(w, h), plain.refinement_mask(w, h))
