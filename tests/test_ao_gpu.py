"""Ambient occlusion (scene.set_ambient_occlusion, scene.occlusion_counts, nt_ambient_occlusion*, and the renders that honour the
setting) on the GPU against the oracle.

The expected counts never come from the library: tests/ao_cases.py works them out for every pixel from the oracle's primary-hit
records and nto_kd_intersects, by the definition in include/ntracer_hip.h.  Counts must be equal, no tolerance: DESIGN.md 4.4 and
4.5 measured these walks and hit_normal as bit-equal to the oracle.  A render with the setting on must be, byte for byte, the
library's own plain fp32 x 3 frame P (pinned to the oracle by the existing suite) times f = 1 - strength * blocked / K from the
oracle's counts, packed by the oracle's pack_pixel.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import ao_cases as ao
import fixtures as fx
import ntracer_amd
import primary_hit_cases as ph
import ray_query_cases as rq
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a5a5a
PAD = 7                         # dwords behind the counts
W, H = 37, 21
STRENGTH = 0.75
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
# (name, channels, reversed): 4-, 3-, 6- and 12-byte pixels, and a reversed one
FORMATS = [("rgbx8", fx.RGBX8, False), ("rgb24", RGB24, False), ("rgb16", fx.RGB16, False), ("rgbf32", fx.RGBF32, False),
           ("rgb24-reversed", RGB24, True)]


def _scene(case, mp, k=0):
    name, env = case
    sup.set_switches(mp, ao.SWITCHES, env)
    g, n, flat = rq.scene(name)
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(ao.scene_params(name))
    sc.set_fov(ph.fov_of(name))
    sc._set_camera_arrays(*ph.camera(name, k))
    return sc


def _standard(sc, n, **kw):
    args = dict(radius=ao.RADIUS, bias=ao.BIAS)
    args.update(kw)
    sc.set_ambient_occlusion(args.pop("T", ao.table(n)), **args)


def _device_counts(sc, w, h, abort=None):
    """nt_ambient_occlusion_device on a sentinel-filled buffer with PAD dwords behind it: the raw buffer"""
    import torch
    buf = torch.full((w * h + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    opts = sup.render_opts(abort, strict_reference=sup.strict_reference())
    _lib.check(_lib.lib().nt_ambient_occlusion_device(sc._handle, w, h, C.c_void_p(buf.data_ptr()), C.byref(opts),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _assert_counts(got, want, label):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: the counts differ on %d pixels, first (y, x) = %r: got %r, oracle %r" % (
        label, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _both_forms(sc, w, h, want, label):
    got = sc.occlusion_counts(w, h)
    assert got.dtype == np.int32 and got.shape == (h, w)
    _assert_counts(got, want, label + " host")
    raw = _device_counts(sc, w, h)
    _assert_counts(raw[:w * h].reshape(h, w), want, label + " device")
    assert (raw[w * h:] == SENTINEL).all(), label + ": a dword behind the counts was written"


# ------------------------------------------------------------------ 1. counts
@pytest.mark.parametrize("case", ao.CASES, ids=ao.case_id)
def test_counts_equal_the_oracle(case):
    name, env = case
    n = rq.scene(name)[1]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, n)
        for w, h in ao.sizes(case):
            e = ao.expected(case, w, h)
            print("%s %dx%d: hit %d, blocked > 0 on %d" % (ao.case_id(case), w, h, int(e["hit"].sum()), int((e["blocked"] > 0).sum())))
            _both_forms(sc, w, h, e["blocked"], "%s %dx%d" % (ao.case_id(case), w, h))


def test_the_python_device_form_is_a_tensor_on_the_current_stream():
    import torch
    case = ("feature5_n5", {})
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, 5)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = sc.occlusion_counts(W, H, device="cuda")
        st.synchronize()
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (H, W)
        _assert_counts(got.cpu().numpy(), ao.expected(case, W, H)["blocked"], "feature5_n5 python device form")


# ------------------------------------------------------------------ 2. the routes agree
def test_the_routes_give_equal_counts():
    w, h = ao.BIG
    got = []
    for env in ({}, {"NTRACER_FORCE_VAR": "1"}, {"NTRACER_COMPOSITE_KERNEL": "2"}):
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(("cell120_n4", env), mp)
            _standard(sc, 4)
            got.append(sc.occlusion_counts(w, h))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    _assert_counts(got[0], ao.expected(("cell120_n4", {}), w, h)["blocked"], "cell120_n4 64x48")
    assert (got[0] > 0).sum() > 500


# ------------------------------------------------------------------ 3. K and the parameters
PARAMS = [
    ("K=1", ("cell120_n4", {}), (9, 7), dict(T=ao.table(4, 1))),
    ("K=5", ("cell120_n4", {}), (9, 7), dict(T=ao.table(4, 5))),
    ("K=5,rays", ("cell120_n4", {"NTRACER_FORCE_VAR": "1"}), (9, 7), dict(T=ao.table(4, 5))),
    ("radius=0.05", ("cell120_n4", {}), (W, H), dict(radius=0.05)),
    ("radius=0.05,rays", ("feature5_n5", {}), (W, H), dict(radius=0.05)),
    ("rows-of-length-2", ("cell120_n4", {}), (W, H), dict(T=(2 * ao.table(4)).astype(np.float32), radius=0.5)),
    ("bias=0", ("orthoplex5_n5", {}), (W, H), dict(bias=0.0)),
]


@pytest.mark.parametrize("label,case,size,kw", PARAMS, ids=[p[0] for p in PARAMS])
def test_k_and_the_parameters(label, case, size, kw):
    n = rq.scene(case[0])[1]
    w, h = size
    e = ao.expected(case, w, h, T=kw.get("T"), radius=kw.get("radius", ao.RADIUS), bias=kw.get("bias", ao.BIAS))
    blocked = e["blocked"]
    print(label, "hit %d, blocked > 0 on %d, histogram %s" % (int(e["hit"].sum()), int((blocked > 0).sum()), np.bincount(blocked[blocked >= 0]).tolist()))
    if label == "rows-of-length-2":
        # the radius is in units of |t_k|: half the radius with rows twice as long reaches as far as the standard parameters
        assert (blocked > 0).sum() > 150
    if label == "bias=0":
        assert (blocked > 0).sum() == 112
    if label.startswith("radius=0.05"):
        assert (blocked >= 0).sum() > 100                   # (whatever a reach that short still finds)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, n, **kw)
        _both_forms(sc, w, h, blocked, label)


# ------------------------------------------------------------------ 4. renders
def plain_colors(sc, w, h):
    """P: the library's plain fp32 x 3 frame of a scene whose setting is off, [h][w][3] float32, clamped by the packer"""
    assert sc.ambient_occlusion is None
    return sup.render_host(sc, sup.fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h, w, 3)


@pytest.mark.parametrize("name", ["feature5_n5", "cell120_n4"])
def test_renders_equal_the_plain_frame_times_the_oracles_factor(name):
    case = (name, {})
    n = rq.scene(name)[1]
    e = ao.expected(case, W, H)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        P = plain_colors(sc, W, H)
        want_rgb = ao.shade(P, e["blocked"], ao.K, STRENGTH)
        assert (want_rgb != P).any(axis=2).sum() >= 30            # the setting shows
        _standard(sc, n, strength=STRENGTH)
        for fname, chans, rev in FORMATS:
            want = sx.pack(want_rgb, chans, rev)
            fmt = sup.fmt_of(W, H, chans, rev=rev)
            img = sup.render_host(sc, fmt)
            assert np.array_equal(img, want), (name, fname, "BlockingRenderer", int((img != want).sum()))
            status, img = sup.render_device(sc, fmt)
            assert status == 0 and np.array_equal(img, want), (name, fname, "nt_render_device", int((img != want).sum()))
        # a padded pitch keeps its padding
        bpp = 3
        fmt = sup.fmt_of(W, H, RGB24, pitch=W * bpp + 5)
        buf = bytearray(b"\xb3" * (fmt.pitch * H))
        assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
        got = np.frombuffer(bytes(buf), np.uint8).reshape(H, fmt.pitch)
        assert np.array_equal(got[:, :W * bpp], sx.pack(want_rgb, RGB24)) and (got[:, W * bpp:] == 0xb3).all()


@pytest.mark.parametrize("name", ["feature5_n5", "cell120_n4"])
def test_three_frames_of_a_camera_table_equal_three_single_renders(name):
    import torch
    case = (name, {})
    n = rq.scene(name)[1]
    nf = 3
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        P = plain_colors(sc, W, H)
        _standard(sc, n, strength=STRENGTH)
        for fname, chans, rev in (FORMATS[0], FORMATS[1]):
            fmt = sup.fmt_of(W, H, chans, rev=rev)
            singles = []
            for o, a in cams:
                sc._set_camera_arrays(o, a)
                singles.append(sup.render_host(sc, fmt))
            singles = np.stack(singles)
            assert np.array_equal(singles[0], sx.pack(ao.shade(P, ao.expected(case, W, H)["blocked"], ao.K, STRENGTH), chans, rev))
            assert not np.array_equal(singles[0], singles[1])
            table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
            frame_bytes = fmt.pitch * H + 64
            buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
            assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().reshape(nf, frame_bytes)
            assert np.array_equal(got[:, :fmt.pitch * H].reshape(nf, H, fmt.pitch), singles), (name, fname)
            assert (got[:, fmt.pitch * H:] == 0x3D).all()
            # the table form refuses what the setting excludes, drawing nothing
            buf.fill_(0x3D)
            with pytest.raises(NotImplementedError, match="ambient occlusion"):
                table.render(sc, buf, fmt, frame_bytes=frame_bytes, band_rank=0, band_world=2)
            torch.cuda.synchronize()
            assert bool((buf == 0x3D).all())


# ------------------------------------------------------------------ 5. the scratch cap
@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_a_small_scratch_cap_gives_the_same_bytes(name):
    """128 x 96 pixels under a cap of 1 MiB: a frame's 32 + 8 n bytes a pixel fit once and not twice, so frames go one to a chunk;
    on the ray route what is left of the cap holds the rays of two pixel rows, so a frame is cut into 48 chunks"""
    import torch
    case = (name, {})
    n = rq.scene(name)[1]
    w, h, nf = 128, 96, 3
    per_frame = w * h * (32 + 8 * n)
    assert per_frame <= (1 << 20) - 16 < 2 * per_frame
    if name == "feature5_n5":
        assert ((1 << 20) - 16 - per_frame) // (w * ao.K * (8 * n + 32)) == 2
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, n, strength=STRENGTH)
        table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
        fmt = sup.fmt_of(w, h, RGB24)
        frame_bytes = fmt.pitch * h
        images, counts = [], []
        for mib in (1024, 1):
            sc.set_supersampling_scratch_mb(mib)
            buf = torch.zeros((nf * frame_bytes,), dtype=torch.uint8, device="cuda")
            assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=0, count=nf)
            torch.cuda.synchronize()
            images.append(buf.cpu().numpy())
            counts.append(sc.occlusion_counts(w, h))
        assert np.array_equal(images[0], images[1]) and np.array_equal(counts[0], counts[1])
        assert (counts[0] > 0).sum() > 200 and len(np.unique(images[0])) > 16
        frames = images[0].reshape(nf, -1)
        assert not np.array_equal(frames[0], frames[1])


def test_a_frame_that_does_not_fit_the_scratch_cap_is_refused_before_anything_is_launched():
    """160 x 120 pixels at n = 4 take 1 228 800 bytes: refused under a cap of 1 MiB with the destination untouched"""
    case = ("cell120_n4", {})
    w, h = 160, 120
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, 4)
        sc.set_supersampling_scratch_mb(1)
        fmt = sup.fmt_of(w, h, fx.RGBX8)
        status, img = sup.render_device(sc, fmt, fill=0x4E)
        assert status == _lib.NT_E_UNSUPPORTED and (img == 0x4E).all()
        assert _lib.last_error().startswith("ambient occlusion") and "nt_scene_set_supersampling_scratch_mb" in _lib.last_error()
        with pytest.raises(NotImplementedError, match="ambient occlusion"):
            sc.occlusion_counts(w, h)
        sc.set_supersampling_scratch_mb(1024)
        assert (sc.occlusion_counts(w, h) > 0).sum() > 1000


# ------------------------------------------------------------------ 6. neutral settings
def test_strength_zero_and_a_scene_where_nothing_blocks_give_the_plain_bytes():
    for name, kw in (("cell120_n4", dict(strength=0.0)), ("feature5_n5", dict(strength=0.0)), ("orthoplex5_n5", dict(strength=1.0))):
        case = (name, {})
        n = rq.scene(name)[1]
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp)
            plain = {f[0]: sup.render_host(sc, sup.fmt_of(W, H, f[1], rev=f[2])) for f in FORMATS}
            _standard(sc, n, **kw)
            for fname, chans, rev in FORMATS:
                assert np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, chans, rev=rev)), plain[fname]), (name, fname)
            assert len(np.unique(plain["rgbx8"])) > 8
            # and taking the setting off again is the plain render
            sc.set_ambient_occlusion(None)
            assert np.array_equal(sup.render_host(sc, sup.fmt_of(W, H, fx.RGBX8)), plain["rgbx8"])


def test_the_probes_the_hits_and_the_queries_ignore_the_setting():
    case = ("cell120_n4", {})
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = _scene(case, mp), _scene(case, mp)
        _standard(sc, 4)
        rng = np.random.default_rng(5)
        xs, ys = rng.integers(0, W, 60), rng.integers(0, H, 60)
        assert np.array_equal(sc.colors_at(xs, ys, W, H).view(np.uint32), plain.colors_at(xs, ys, W, H).view(np.uint32))
        got, want = sc.primary_hits(W, H, normals=True), plain.primary_hits(W, H, normals=True)
        assert np.array_equal(got.hits, want.hits) and np.array_equal(got.normal_dir.view(np.uint32), want.normal_dir.view(np.uint32))


def test_the_colours_of_caller_rays_and_the_ray_queries_ignore_the_setting():
    """ray_colors, render_rays, intersect_rays and occludes_rays on the view's own primary rays: the same bits with the setting on
    as on a scene without it -- and the view is one the setting would change"""
    case = ("cell120_n4", {})
    with pytest.MonkeyPatch.context() as mp:
        sc, plain = _scene(case, mp), _scene(case, mp)
        _standard(sc, 4)
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        assert not np.array_equal(sup.render_host(sc, fmt), sup.render_host(plain, fmt))
        origin, axes = ph.camera("cell120_n4", 0)
        d = np.ascontiguousarray(ph.rays("cell120_n4", W, H, 0)[0].reshape(W * H, 4), np.float32)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float32), d.shape))
        assert np.array_equal(sc.ray_colors(o, d).view(np.uint32), plain.ray_colors(o, d).view(np.uint32))
        got, want = bytearray(fmt.pitch * H), bytearray(fmt.pitch * H)
        sc.render_rays(got, fmt, o, d)
        plain.render_rays(want, fmt, o, d)
        assert got == want and len(set(want)) > 8
        for query in ("intersect_rays", "occludes_rays"):
            a, b = getattr(sc, query)(o, d), getattr(plain, query)(o, d)
            assert sorted(a) == sorted(b)
            for key in a:
                assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (query, key)


# ------------------------------------------------------------------ 7. abort
@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_an_abort_word_raised_before_the_launch_leaves_the_buffers_untouched(name):
    import torch
    case = (name, {})
    n = rq.scene(name)[1]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, n, strength=STRENGTH)
        word = torch.ones(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        raw = _device_counts(sc, W, H, abort=word)
        assert (raw == SENTINEL).all()
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word, strict_reference=sup.strict_reference()), fill=0x6A)
        assert status == 0 and (img == 0x6A).all()
        word.zero_()
        torch.cuda.synchronize()
        raw = _device_counts(sc, W, H, abort=word)
        _assert_counts(raw[:W * H].reshape(H, W), ao.expected(case, W, H)["blocked"], name + " after the abort word went down")
        status, img = sup.render_device(sc, fmt, opts=sup.render_opts(word, strict_reference=sup.strict_reference()), fill=0x6A)
        assert status == 0 and np.array_equal(img, sup.render_host(sc, fmt))


# ------------------------------------------------------------------ 8. repeat
@pytest.mark.parametrize("name", ["cell120_n4", "feature5_n5"])
def test_two_calls_in_a_row_agree_and_a_warm_table_render_is_capturable(name):
    """the second call of a shape gives the first one's results; and after a warm-up call of the same shape a table render with the
    setting on only enqueues -- no allocation, no read-back --: captured into a HIP graph on one stream and replayed, it gives
    the direct call's bytes (the way tests/test_adaptive_gpu.py sees the same claim)"""
    import torch
    case = (name, {})
    n = rq.scene(name)[1]
    nf = 2
    cams = [ph.camera(name, k) for k in range(nf)]
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        _standard(sc, n, strength=STRENGTH)
        a, b = _device_counts(sc, W, H), _device_counts(sc, W, H)
        assert np.array_equal(a, b)
        _assert_counts(b[:W * H].reshape(H, W), ao.expected(case, W, H)["blocked"], name + " second call")
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
