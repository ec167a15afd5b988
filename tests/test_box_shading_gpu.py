"""BoxScene face shading (BoxScene.set_face_shading and the renders that honour it) on the GPU against the rule.

The expected frames never come from the library: tests/box_shading_cases.py works them out for every pixel, in sequential fp32
numpy, from what tests/box_hit_cases.py takes from the oracle.  The rule is sequential fp32, so every comparison is bit-exact:
the plain fp32 x 3 format as uint32, every other format byte for byte through the oracle's pack_pixel (ss_expected.pack) -- on the
fused kernels and, under NTRACER_FORCE_VAR=1 and above 24 dimensions, on the two passes at run-time n.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import box_hit_cases as bc
import box_shading_cases as cases
import fixtures as fx
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
ENVS = ({}, {"NTRACER_FORCE_VAR": "1"})


def scene(n, k, mp, env=None):
    sup.set_switches(mp, ("NTRACER_FORCE_VAR",), env or {})
    sc = tracern.BoxScene(n)
    sc.set_fov(bc.FOV)
    sc._set_camera_arrays(*bc.camera(n, k))
    return sc


def apply(sc, n, name, w, h, which):
    kw, lines = cases.setting(n, name, w, h, which)
    sc.set_face_shading(**kw)
    if lines is None:
        sc.set_face_lines(None)
    else:
        sc.set_face_lines(**lines)


def as_rgb(img, w, h):
    """the floats of a frame in the plain fp32 x 3 format"""
    return img.view(">f4").astype(np.float32).reshape(h, w, 3)


def _differ(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
    return "equal" if len(bad) == 0 else "%d pixels differ, first (y, x) = %r: got %r, rule %r" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ------------------------------------------------------------------ 1. every view under every setting
@pytest.mark.parametrize("route", cases.ROUTES, ids=cases.route_id)
def test_frames_equal_the_rule(route):
    """settings a to e of every view: the plain fp32 x 3 format as uint32 and RGBX8 byte for byte, through BlockingRenderer.render
    and nt_render_device; for d also RGB24 with a pitch larger than the row -- the padding as it was -- and reversed channels"""
    n, env = route
    shown = 0
    with pytest.MonkeyPatch.context() as mp:
        for name, k in cases.CAMERAS.items():
            sc = scene(n, k, mp, env)
            for w, h in cases.SIZES:
                for which in cases.SETTINGS:
                    apply(sc, n, name, w, h, which)
                    want = cases.expected(n, name, w, h, which)["rgb"]
                    label = "n%d%s %s %dx%d setting %s" % (n, " force-var" if env else "", name, w, h, which)
                    f = sup.fmt_of(w, h, fx.RGBF32)
                    got = as_rgb(sup.render_host(sc, f), w, h)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (label, "fp32 host", _differ(got, want))
                    status, img = sup.render_device(sc, f)
                    got = as_rgb(img, w, h)
                    assert status == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (label, "fp32 device", _differ(got, want))
                    f = sup.fmt_of(w, h, fx.RGBX8)
                    packed = sx.pack(want, fx.RGBX8)
                    img = sup.render_host(sc, f)
                    assert np.array_equal(img, packed), (label, "rgbx8 host", int((img != packed).sum()))
                    status, img = sup.render_device(sc, f)
                    assert status == 0 and np.array_equal(img, packed), (label, "rgbx8 device", int((img != packed).sum()))
                    if which == "d":
                        f = sup.fmt_of(w, h, RGB24, pitch=w * 3 + 5)
                        img = sup.render_host(sc, f, fill=0xb3)
                        assert np.array_equal(img[:, :w * 3], sx.pack(want, RGB24)) and (img[:, w * 3:] == 0xb3).all(), (label, "rgb24, padded")
                        status, img = sup.render_device(sc, f, fill=0xb3)
                        assert status == 0 and np.array_equal(img[:, :w * 3], sx.pack(want, RGB24)) and (img[:, w * 3:] == 0xb3).all(), label
                        f = sup.fmt_of(w, h, RGB24, rev=True)
                        img = sup.render_host(sc, f)
                        assert np.array_equal(img, sx.pack(want, RGB24, True)), (label, "rgb24, reversed")
                        status, img = sup.render_device(sc, f)
                        assert status == 0 and np.array_equal(img, sx.pack(want, RGB24, True)), (label, "rgb24, reversed, device")
                    shown += 1
    assert shown == len(cases.CAMERAS) * len(cases.SIZES) * len(cases.SETTINGS)


# ------------------------------------------------------------------ 2. the neutral settings
@pytest.mark.parametrize("route", cases.ROUTES, ids=cases.route_id)
def test_neutral_settings_give_the_plain_frame_and_with_lines_the_face_line_frame(route):
    """no table, no tint and fog_strength = 0 -- or only a table equal to the default, or both: the bytes of the render without the
    setting, in RGBX8 and the plain fp32 format"""
    n, env = route
    neutral = (dict(near=0.5, far=3.0, color=(1.0, 0.0, 1.0), strength=0.0, background=True), dict(colors=cases.default_table(n)),
               dict(colors=cases.default_table(n), far=2.0, strength=0.0))
    with pytest.MonkeyPatch.context() as mp:
        for name in ("faces", "diagonal", "nothing"):
            for w, h in cases.SIZES[1:]:
                sc = scene(n, cases.CAMERAS[name], mp, env)
                for lines in (None, dict(color=cases.LINE_COLOR, strength=cases.LINE_STRENGTH)):
                    sc.set_face_shading(None)
                    if lines:
                        sc.set_face_lines(**lines)
                    assert sc.face_shading is None
                    fmts = [sup.fmt_of(w, h, fx.RGBX8), sup.fmt_of(w, h, fx.RGBF32)]
                    plain = [sup.render_host(sc, f) for f in fmts]
                    for kw in neutral:
                        sc.set_face_shading(**kw)
                        assert sc.face_shading is not None
                        for f, want in zip(fmts, plain):
                            label = (cases.route_id(route), name, w, h, bool(lines), sorted(kw))
                            assert np.array_equal(sup.render_host(sc, f), want), label
                            status, img = sup.render_device(sc, f)
                            assert status == 0 and np.array_equal(img, want), label
                if name != "nothing":
                    sc.set_face_shading(None)
                    sc.set_face_lines(None)
                    assert not np.array_equal(sup.render_host(sc, fmts[0]), plain[0])          # (the lines show: two different comparisons)


# ------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("route", [(6, {}), (6, {"NTRACER_FORCE_VAR": "1"}), (6, {"NTRACER_FORCE_VAR": "1", "NTRACER_CHUNK_FRAMES": "2"}), (25, {})],
                         ids=lambda r: "n%d%s" % (r[0], "".join("-" + k[8:].lower() for k in sorted(r[1]))))
def test_three_cameras_in_one_call_equal_three_single_renders(route):
    """nt_render_table_device and nt_render_frames_device with a frame_stride larger than a frame: each frame is its single-frame
    render, the first of them the rule's, no two equal, the gap as it was -- with lines (setting e of the first view) and without"""
    import torch
    n, env = route
    nf = 3
    names = ("faces", "diagonal", "on-plane")
    cams = [bc.camera(n, cases.CAMERAS[name]) for name in names]
    origins, axes = np.ascontiguousarray(np.stack([c[0] for c in cams])), np.ascontiguousarray(np.stack([c[1] for c in cams]))
    w, h = cases.SIZES[2]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, cases.CAMERAS[names[0]], mp, env)
        for which in ("d", "e"):
            apply(sc, n, names[0], w, h, which)
            for chans in (fx.RGBX8, fx.RGBF32):
                fmt = sup.fmt_of(w, h, chans)
                singles = []
                for o, a in cams:
                    sc._set_camera_arrays(o, a)
                    singles.append(sup.render_host(sc, fmt))
                singles = np.stack(singles)
                assert np.array_equal(singles[0], sx.pack(cases.expected(n, names[0], w, h, which)["rgb"], chans))
                for i in range(nf):
                    for j in range(i):
                        assert not np.array_equal(singles[i], singles[j])
                table = CameraTable(n, origins, axes)
                frame_bytes = fmt.pitch * h + 64
                buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
                assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
                torch.cuda.synchronize()
                got = buf.cpu().numpy().reshape(nf, frame_bytes)
                assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (route, which, "table")
                assert (got[:, fmt.pitch * h:] == 0x3D).all()
                buf.fill_(0x3D)
                fst = fmt._as_struct()
                _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, nf, origins.ctypes.data_as(_lib.f32p),
                                                              axes.ctypes.data_as(_lib.f32p), C.byref(fst), None,
                                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                got = buf.cpu().numpy().reshape(nf, frame_bytes)
                assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (route, which, "frames")
                assert (got[:, fmt.pitch * h:] == 0x3D).all()
                # the table form refuses what the setting excludes, drawing nothing
                buf.fill_(0x3D)
                with pytest.raises(NotImplementedError, match="face lines" if which == "e" else "face shading"):
                    table.render(sc, buf, fmt, frame_bytes=frame_bytes, band_rank=0, band_world=2)
                torch.cuda.synchronize()
                assert bool((buf == 0x3D).all())


# ------------------------------------------------------------------ 4. the scratch cap of the run-time-n route, abort, capture
def _table_setting(sc, n, lines):
    sc.set_face_shading(cases.table(n), near=1.0, far=4.0, color=cases.FOG_COLOR, strength=cases.FOG_STRENGTH, background=True,
                        tint_axis=tuple(float(v) for v in cases.tint_axis(n)), tint_range=(-3.0, 3.0), tint_colors=cases.TINT_COLORS)
    if lines:
        sc.set_face_lines(cases.LINE_COLOR, cases.LINE_STRENGTH)
    else:
        sc.set_face_lines(None)


@pytest.mark.parametrize("lines", (False, True), ids=("", "lines"))
def test_a_small_scratch_cap_gives_the_same_bytes_and_a_frame_that_does_not_fit_is_refused(lines):
    """16 bytes a pixel and frame at run-time n: 256 x 160 fits a cap of 1 MiB once and not twice, 320 x 240 not at all; the fused
    kernels need no scratch and draw either"""
    import torch
    n, nf = 6, 3
    cams = [bc.camera(n, k) for k in (2, 4, 1)]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, 2, mp, {"NTRACER_FORCE_VAR": "1"})
        _table_setting(sc, n, lines)
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
        assert _lib.last_error().startswith("face shading") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        sc.set_supersampling_scratch_mb(1024)
        status, img = sup.render_device(sc, fmt, fill=0x4E)
        assert status == 0 and np.array_equal(img, fused)


@pytest.mark.parametrize("env", ENVS, ids=("", "force-var"))
def test_an_abort_word_raised_before_the_launch_leaves_the_destination_untouched(env):
    import torch
    n, name, (w, h) = 6, "faces", cases.SIZES[2]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, cases.CAMERAS[name], mp, env)
        for which in ("d", "e"):
            apply(sc, n, name, w, h, which)
            word = torch.ones(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            opts = _lib.NtRenderOpts()
            opts.device = -1
            opts.abort_device = word.data_ptr()
            fmt = sup.fmt_of(w, h, fx.RGBX8)
            status, img = sup.render_device(sc, fmt, opts=opts, fill=0x6A)
            assert status == 0 and (img == 0x6A).all()
            word.zero_()
            torch.cuda.synchronize()
            status, img = sup.render_device(sc, fmt, opts=opts, fill=0x6A)
            assert status == 0 and np.array_equal(img, sx.pack(cases.expected(n, name, w, h, which)["rgb"], fx.RGBX8))


@pytest.mark.parametrize("lines", (False, True), ids=("", "lines"))
def test_a_warm_table_render_is_capturable(lines):
    """the fused kernels allocate nothing and add no synchronisation: a table render with the setting on, captured into a graph on
    one stream and replayed, gives the direct call's bytes"""
    import torch
    n, nf, (w, h) = 6, 2, cases.SIZES[2]
    cams = [bc.camera(n, k) for k in (2, 4)]
    with pytest.MonkeyPatch.context() as mp:
        sc = scene(n, 2, mp)
        _table_setting(sc, n, lines)
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
        assert len(np.unique(ref[1].cpu().numpy())) > 16


# ------------------------------------------------------------------ 5. the calls that ignore the setting
def test_the_probes_the_rays_the_records_and_the_masks_ignore_the_setting():
    n, name, (w, h) = 6, "faces", (37, 21)
    k = cases.CAMERAS[name]
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = scene(n, k, mp), scene(n, k, mp)
        _table_setting(sc, n, True)
        plain.set_face_lines(cases.LINE_COLOR, cases.LINE_STRENGTH)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        rng = np.random.default_rng(5)
        xs, ys = rng.integers(0, w, 60), rng.integers(0, h, 60)
        assert np.array_equal(sc.colors_at(xs, ys, w, h).view(np.uint32), plain.colors_at(xs, ys, w, h).view(np.uint32))
        assert np.array_equal(sc.face_hits(w, h).records, plain.face_hits(w, h).records)
        assert np.array_equal(sc.face_line_mask(w, h), plain.face_line_mask(w, h)) and sc.face_line_mask(w, h).any()
        e = bc.expected(n, k, w, h)
        d = np.ascontiguousarray(e["dirs"].reshape(w * h, n), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(bc.camera(n, k)[0], d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
        for s in (sc, plain):
            s.set_supersampling(2)
            s.set_adaptive_supersampling(0.1)
        assert np.array_equal(sc.refinement_mask(w, h), plain.refinement_mask(w, h))
