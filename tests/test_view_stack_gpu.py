"""View stacks (Scene.set_view_stack and the renders that honour it) on the GPU against the rule.

BoxScene: the expected bytes never come from the library -- tests/view_stack_cases.py takes the colours of every sample camera
from the oracle, sums them by the rule in sequential fp32 numpy and packs them with the oracle's pack_pixel; every comparison is
byte for byte, on the fused kernel (n = 3, 6, 24), on the frames route above 24 dimensions and, at n = 6, with
set_view_stack_route("frames").  Composite scenes: the rendered bytes equal pack(sum of w_k P_k), P_k the library's own plain fp32
frame under sample camera k with the setting off, and every P_k is held to the oracle's clamped colours within the suite's 1e-5
(the existing suite never feeds these sheared cameras).

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import box_hit_cases as bc
import fixtures as fx
import primary_hit_cases as ph
import ray_color_cases as rc
import view_stack_cases as vc
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

FRAMES = {"route": "frames"}          # not an environment switch: box_scene hands it to set_view_stack_route
# (dimension, environment and route): the fused kernel, the frames route above 24 dimensions, and the frames route where the fused kernel exists
BOX_ROUTES = [(n, {}) for n in vc.BOX_FUSED_DIMS] + [(n, {}) for n in vc.BOX_FRAMES_DIMS] + [(6, FRAMES)]


def route_id(r):
    return "n%d%s" % (r[0], "-frames" if r[1] else "")


def _env(mp, env):
    sup.set_switches(mp, vc.SWITCHES, env or {})


def box_scene(n, k, mp, env=None):
    env = dict(env or {})
    route = env.pop("route", None)
    _env(mp, env)
    sc = tracern.BoxScene(n)
    sc.set_view_stack_route(route)
    sc.set_fov(bc.FOV)
    sc._set_camera_arrays(*bc.camera(n, k))
    return sc


def composite_scene(case, mp):
    _env(mp, case[1])
    n, flat, params = rc.case_scene(case)
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(params)
    sc.set_fov(ph.fov_of(case[0]))
    sc._set_camera_arrays(*vc.composite_camera(case))
    return sc


def as_rgb(img, w, h):
    """the floats of a frame in the plain fp32 x 3 format"""
    return np.ascontiguousarray(img).view(">f4").astype(np.float32).reshape(h, w, 3)


def _differ(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(axis=2))
    return "equal" if len(bad) == 0 else "%d pixels differ, first (y, x) = %r: got %r, rule %r" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _set(sc, st):
    e, focus, w = st
    sc.set_view_stack(e, focus, w)


# ------------------------------------------------------------------ 1. BoxScene against the oracle
@pytest.mark.parametrize("route", BOX_ROUTES, ids=route_id)
def test_box_frames_equal_the_rule_byte_for_byte(route):
    """every stack under both cameras at every size: the plain fp32 x 3 format as the packer clamps the sums, and RGBX8, through
    nt_render and nt_render_device; at 37 x 21 also RGB24, RGB16, reversed RGB24 and RGB24 with a padded pitch whose padding
    survives"""
    n, env = route
    with pytest.MonkeyPatch.context() as mp:
        for k in vc.BOX_CAMERAS:
            sc = box_scene(n, k, mp, env)
            for name in vc.stacks_of(n):
                _set(sc, vc.box_stack(n, k, name))
                for w, h in vc.SIZES:
                    want = vc.box_expected(n, k, name, w, h)
                    label = "%s camera %d %s %dx%d" % (route_id(route), k, name, w, h)
                    f = sup.fmt_of(w, h, fx.RGBF32)
                    got, clamped = as_rgb(sup.render_host(sc, f), w, h), vc.clamp01(want)
                    assert np.array_equal(got.view(np.uint32), clamped.view(np.uint32)), (label, "fp32 host", _differ(got, clamped))
                    f = sup.fmt_of(w, h, fx.RGBX8)
                    packed = vc.pack(want, fx.RGBX8)
                    img = sup.render_host(sc, f)
                    assert np.array_equal(img, packed), (label, "rgbx8 host", _differ(img.reshape(h, w, 4), packed.reshape(h, w, 4)))
                    status, img = sup.render_device(sc, f)
                    assert status == 0 and np.array_equal(img, packed), (label, "rgbx8 device", int((img != packed).sum()))
                    if (w, h) != vc.SHOW_SIZE:
                        continue
                    if name != "one":
                        vc.check_box_shows(n, k, name)          # (the expectation just met is not the plain frame's)
                    for fname, chans, rev in vc.FORMATS:
                        status, img = sup.render_device(sc, sup.fmt_of(w, h, chans, rev=rev))
                        assert status == 0 and np.array_equal(img, vc.pack(want, chans, rev)), (label, fname)
                    f = sup.fmt_of(w, h, vc.RGB24, pitch=w * 3 + 5)
                    for img in (sup.render_host(sc, f, fill=0xb3), sup.render_device(sc, f, fill=0xb3)[1]):
                        assert np.array_equal(img[:, :w * 3], vc.pack(want, vc.RGB24)) and (img[:, w * 3:] == 0xb3).all(), (label, "rgb24, padded")


def test_both_box_routes_give_identical_bytes_and_one_sample_is_the_plain_frame():
    n, k, (w, h) = 6, 2, vc.SIZES[3]
    with pytest.MonkeyPatch.context() as mp:
        sc = box_scene(n, k, mp)
        fmts = [sup.fmt_of(w, h, fx.RGBX8), sup.fmt_of(w, h, fx.RGBF32), sup.fmt_of(w, h, vc.RGB24)]
        plain = [sup.render_host(sc, f) for f in fmts]
        for name in vc.stacks_of(n):
            _set(sc, vc.box_stack(n, k, name))
            sc.set_view_stack_route(None)
            fused = [sup.render_device(sc, f)[1] for f in fmts]
            sc.set_view_stack_route("frames")
            assert sc.view_stack_route == "frames"
            frames = [sup.render_device(sc, f)[1] for f in fmts]
            for a, b, p in zip(fused, frames, plain):
                assert np.array_equal(a, b), name
                # K = 1 with a zero offset and weight 1: the plain render's bytes; every other stack shows
                assert np.array_equal(a, p) == (name == "one"), name
        # taking the setting off gives the plain bytes again, on either route
        sc.set_view_stack(None)
        for f, p in zip(fmts, plain):
            assert np.array_equal(sup.render_device(sc, f)[1], p)


# ------------------------------------------------------------------ 2. composite scenes
@pytest.mark.parametrize("case", vc.COMPOSITE, ids=vc.composite_id)
def test_composite_frames_equal_the_sum_of_the_plain_frames(case):
    """every stack at every size: P_k, the library's plain fp32 frame under sample camera k with the setting off, within 1e-5 of
    the oracle's clamped colours; then the render with the setting on, byte for byte pack(sum w_k P_k), in every format at 37 x 21"""
    sizes = vc.SIZES
    with pytest.MonkeyPatch.context() as mp:
        sc = composite_scene(case, mp)
        cam = vc.composite_camera(case)
        for name in vc.STACKS:
            st = vc.composite_stack(case, name)
            origins, axes = vc.composite_cameras(case, name)
            for w, h in sizes:
                label = "%s %s %dx%d" % (vc.composite_id(case), name, w, h)
                sc.set_view_stack(None)
                f32fmt = sup.fmt_of(w, h, fx.RGBF32)
                P = np.zeros((len(origins), h, w, 3), np.float32)
                for i in range(len(origins)):
                    sc._set_camera_arrays(origins[i], axes[i])
                    P[i] = as_rgb(sup.render_device(sc, f32fmt)[1], w, h)
                oracle = vc.composite_frames(case, name, w, h)
                err = float(np.abs(P.astype(np.float64) - oracle).max())
                assert err <= 1e-5, (label, "a plain frame under a sample camera is not the oracle's", err)
                want = vc.accumulate(P, st[2])
                sc._set_camera_arrays(*cam)
                _set(sc, st)
                formats = vc.FORMATS if (w, h) == vc.SHOW_SIZE else vc.FORMATS[:1]
                for fname, chans, rev in formats:
                    status, img = sup.render_device(sc, sup.fmt_of(w, h, chans, rev=rev))
                    assert status == 0 and np.array_equal(img, vc.pack(want, chans, rev)), (label, fname)
                img = sup.render_host(sc, sup.fmt_of(w, h, fx.RGBX8))
                assert np.array_equal(img, vc.pack(want, fx.RGBX8)), (label, "host")
        # K = 1 with a zero offset gives the plain render's bytes, and so does taking the setting off
        w, h = vc.SHOW_SIZE
        f = sup.fmt_of(w, h, fx.RGBX8)
        _set(sc, vc.composite_stack(case, "one"))
        one = sup.render_device(sc, f)[1]
        sc.set_view_stack(None)
        assert np.array_equal(one, sup.render_device(sc, f)[1]) and len(np.unique(one)) > 8


# ------------------------------------------------------------------ 3. frames
def _three_frames(sc, n, cams, w, h, chans, label):
    import torch
    origins, axes = np.ascontiguousarray(np.stack([c[0] for c in cams])), np.ascontiguousarray(np.stack([c[1] for c in cams]))
    nf = len(cams)
    fmt = sup.fmt_of(w, h, chans)
    singles = []
    for o, a in cams:
        sc._set_camera_arrays(o, a)
        singles.append(sup.render_host(sc, fmt))
    singles = np.stack(singles)
    for i in range(nf):
        for j in range(i):
            assert not np.array_equal(singles[i], singles[j])
    table = CameraTable(n, origins, axes)
    frame_bytes = fmt.pitch * h + 64
    buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
    assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, frame_bytes)
    assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (label, "table")
    assert (got[:, fmt.pitch * h:] == 0x3D).all()
    # a part of the table: frames 1 and 2 alone
    buf.fill_(0x3D)
    assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=1, count=2)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, frame_bytes)
    assert np.array_equal(got[:2, :fmt.pitch * h].reshape(2, h, fmt.pitch), singles[1:]) and (got[2] == 0x3D).all(), (label, "table, from frame 1")
    buf.fill_(0x3D)
    fst = fmt._as_struct()
    _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, nf, origins.ctypes.data_as(_lib.f32p),
                                                  axes.ctypes.data_as(_lib.f32p), C.byref(fst), None,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, frame_bytes)
    assert np.array_equal(got[:, :fmt.pitch * h].reshape(nf, h, fmt.pitch), singles), (label, "frames")
    assert (got[:, fmt.pitch * h:] == 0x3D).all()
    return singles


@pytest.mark.parametrize("route", [(6, {}), (6, FRAMES), (6, dict(FRAMES, NTRACER_CHUNK_FRAMES="2")), (25, {})],
                         ids=lambda r: "n%d%s" % (r[0], "".join("-" + (k[8:].lower() if k.startswith("NTRACER_") else r[1][k]) for k in sorted(r[1]))))
def test_three_box_cameras_in_one_call_equal_three_single_renders(route):
    n, env = route
    w, h = vc.SIZES[2]
    cams = [bc.camera(n, k) for k in (2, 4, 1)]
    with pytest.MonkeyPatch.context() as mp:
        sc = box_scene(n, 2, mp, env)
        for name in ("slab", "disc"):                                   # hidden offsets need every frame's own hidden axes
            _set(sc, vc.box_stack(n, 2, name))
            singles = _three_frames(sc, n, cams, w, h, fx.RGBX8, (route_id(route), name))
            assert np.array_equal(singles[0], vc.pack(vc.box_expected(n, 2, name, w, h), fx.RGBX8))


def test_three_composite_cameras_in_one_call_equal_three_single_renders():
    case = vc.COMPOSITE[0]
    w, h = vc.SIZES[2]
    with pytest.MonkeyPatch.context() as mp:
        sc = composite_scene(case, mp)
        cams = [ph.camera(case[0], k) for k in (0, 1)]
        o, a = cams[0]
        cams.append(((o + np.float32(0.1) * a[0]).astype(np.float32), a))
        for name in ("slab", "anaglyph"):
            _set(sc, vc.composite_stack(case, name))
            _three_frames(sc, sc.dimension, cams, w, h, fx.RGBX8, (case[0], name))


# ------------------------------------------------------------------ 4. the scratch cap, abort, capture
@pytest.mark.parametrize("kind", ("box", "composite"))
def test_a_small_scratch_cap_gives_the_same_bytes_and_a_frame_that_does_not_fit_is_refused(kind):
    """12 bytes a pixel and sample: at 200 x 120 the five frames of K = 5 do not fit 1 MiB, the accumulator and one sample do --
    the samples then go in chunks of consecutive k; at 320 x 240 not even those two fit"""
    with pytest.MonkeyPatch.context() as mp:
        if kind == "box":
            sc = box_scene(6, 2, mp, FRAMES)
            st = vc.box_stack(6, 2, "disc")
        else:
            sc = composite_scene(vc.COMPOSITE[0], mp)
            st = vc.composite_stack(vc.COMPOSITE[0], "disc")
        _set(sc, st)
        w, h = 200, 120
        assert 2 * w * h * 12 <= (1 << 20) < 5 * w * h * 12
        images = []
        for mib in (1024, 1):
            sc.set_supersampling_scratch_mb(mib)
            images.append([sup.render_device(sc, sup.fmt_of(w, h, chans))[1] for chans in (fx.RGBX8, fx.RGBF32)])
        for a, b in zip(*images):
            assert np.array_equal(a, b)
        assert len(np.unique(images[0][0])) > 16
        # the same through a table of two frames, chunked frame by frame
        cams = [sc.get_camera()._origin, sc.get_camera()._axes]
        import torch
        table = CameraTable(sc.dimension, np.stack([cams[0], cams[0]]), np.stack([cams[1], cams[1]]))
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        buf = torch.zeros((2 * fmt.pitch * h,), dtype=torch.uint8, device="cuda")
        assert table.render(sc, buf, fmt, frame_bytes=fmt.pitch * h, first=0, count=2)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().reshape(2, h, fmt.pitch)
        assert np.array_equal(got[0], images[0][0]) and np.array_equal(got[1], images[0][0])
        # nothing fits: refused before anything is launched
        w, h = 320, 240
        assert 2 * w * h * 12 > (1 << 20)
        status, img = sup.render_device(sc, sup.fmt_of(w, h, fx.RGBX8), fill=0x4E)
        assert status == _lib.NT_E_UNSUPPORTED and (img == 0x4E).all()
        assert _lib.last_error().startswith("a view stack") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        if kind == "box":                                               # the fused kernel needs no scratch and draws
            sc.set_view_stack_route(None)
            status, fused = sup.render_device(sc, sup.fmt_of(w, h, fx.RGBX8), fill=0x4E)
            assert status == 0 and len(np.unique(fused)) > 16
            sc.set_view_stack_route("frames")
            sc.set_supersampling_scratch_mb(1024)
            status, img = sup.render_device(sc, sup.fmt_of(w, h, fx.RGBX8), fill=0x4E)
            assert status == 0 and np.array_equal(img, fused)


@pytest.mark.parametrize("kind", ("box-fused", "box-frames", "composite"))
def test_an_abort_word_raised_before_the_launch_leaves_the_destination_untouched(kind):
    import torch
    w, h = vc.SIZES[2]
    with pytest.MonkeyPatch.context() as mp:
        if kind == "composite":
            sc = composite_scene(vc.COMPOSITE[0], mp)
            _set(sc, vc.composite_stack(vc.COMPOSITE[0], "anaglyph"))
            want = None
        else:
            sc = box_scene(6, 2, mp, FRAMES if kind == "box-frames" else None)
            _set(sc, vc.box_stack(6, 2, "anaglyph"))
            want = vc.pack(vc.box_expected(6, 2, "anaglyph", w, h), fx.RGBX8)
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
        assert status == 0 and (np.array_equal(img, want) if want is not None else np.array_equal(img, sup.render_host(sc, fmt)))


@pytest.mark.parametrize("kind", ("box-fused", "box-frames", "composite"))
def test_a_warm_table_render_is_capturable(kind):
    """after one warm-up call of the same shape a table render only enqueues: captured into a graph on one stream and replayed,
    it gives the direct call's bytes"""
    import torch
    nf, (w, h) = 2, vc.SIZES[2]
    with pytest.MonkeyPatch.context() as mp:
        if kind == "composite":
            case = vc.COMPOSITE[0]
            sc = composite_scene(case, mp)
            _set(sc, vc.composite_stack(case, "slab"))
            cams = [ph.camera(case[0], k) for k in (0, 1)]
        else:
            sc = box_scene(6, 2, mp, FRAMES if kind == "box-frames" else None)
            _set(sc, vc.box_stack(6, 2, "slab"))
            cams = [bc.camera(6, k) for k in (2, 4)]
        n = sc.dimension
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
def test_the_probes_the_records_and_the_rays_ignore_the_setting():
    w, h = vc.SHOW_SIZE
    rng = np.random.default_rng(5)
    xs, ys = rng.integers(0, w, 60), rng.integers(0, h, 60)
    with pytest.MonkeyPatch.context() as mp:
        n, k = 6, 2
        sc, plain = box_scene(n, k, mp), box_scene(n, k, mp)
        _set(sc, vc.box_stack(n, k, "disc"))
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        assert np.array_equal(sc.colors_at(xs, ys, w, h).view(np.uint32), plain.colors_at(xs, ys, w, h).view(np.uint32))
        assert np.array_equal(sc.face_hits(w, h).records, plain.face_hits(w, h).records)
        d = np.ascontiguousarray(bc.expected(n, k, w, h)["dirs"].reshape(w * h, n), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(bc.camera(n, k)[0], d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
        case = vc.COMPOSITE[0]
        sc, plain = composite_scene(case, mp), composite_scene(case, mp)
        _set(sc, vc.composite_stack(case, "disc"))
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        assert np.array_equal(sc.colors_at(xs, ys, w, h).view(np.uint32), plain.colors_at(xs, ys, w, h).view(np.uint32))
        a, b = sc.primary_hits(w, h), plain.primary_hits(w, h)
        assert np.array_equal(a.hits, b.hits)
        d = np.ascontiguousarray(ph.rays(case[0], w, h)[0].reshape(w * h, sc.dimension), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(vc.composite_camera(case)[0], d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
