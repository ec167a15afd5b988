"""Supersampled rendering (scene.set_supersampling(s): s x s samples a pixel, resolved on the device) against the oracle.

The expected image never comes from the library: tests/ss_expected.py renders the oracle's s*W x s*H frame in the plain
fp32 x 3 format, sums the s*s samples of a pixel in fp32 in row-major order, divides by float(s*s) and packs with the
oracle's pack_pixel.  BoxScene must match byte for byte; CompositeScene to the project's tolerances against the oracle
(1e-5 a component in fp32, one level a channel in packed bytes)."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import oracle_binding as ob
import ss_expected as sx
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

W, H = 203, 117                 # ragged: the width is no multiple of 64, the height is odd
TOL_ORACLE = 1e-5
RGB24 = [(8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)]
RGB565 = [(5, 1, 0, 0), (6, 0, 1, 0), (5, 0, 0, 1)]
# (name, channels, reversed)
FORMATS = [("rgbx8", fx.RGBX8, False), ("rgbf32", fx.RGBF32, False), ("rgb24", RGB24, False), ("rgb565", RGB565, False),
           ("rgb16", fx.RGB16, False), ("rgb24-reversed", RGB24, True), ("rgbx8-reversed", fx.RGBX8, True)]


def box_cameras(n):
    """a dozen of fixtures.stress_cameras -- axis-aligned, grazing, permuted axes, `up` far from orthogonal, no `up`, origins
    inside the cube, on a face's plane and on two -- and the diagonal camera"""
    rng = np.random.default_rng(977 + n)
    stress = fx.stress_cameras(n, rng)
    cams = [stress[i] for i in (0, 6, 14, 21, 37, 54, 56, 58, 71, 94, 111, 127)]
    cams.append(fx.diagonal_camera(n, 1.6 * np.sqrt(n), rng))
    return cams


def composite(name, params=None):
    g = fx.load(name)
    flat = fx.flat_of(g)
    p = dict(fx.params_of(g))
    if params:
        p.update(params)
    n = int(g["origins"].shape[1])
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(p)
    o, a = g["origins"][0], g["axes"][0]
    sc._set_camera_arrays(o, a)
    return sc, ob.OracleScene(n, o, a, flat=flat, params=p), g


def assert_close_to(img, want, chans, what):
    """the project's tolerances against the oracle: 1e-5 a component for fp32 channels, one level a channel for packed bytes"""
    if chans is fx.RGBF32:
        d = np.abs(img.view(">f4").astype(np.float32) - want.view(">f4").astype(np.float32))
        print(what, "max |delta| %.3g" % float(d.max()))
        assert d.max() <= TOL_ORACLE, (what, float(d.max()))
    else:
        assert all(c[0] == 8 for c in chans)
        d = np.abs(img.astype(np.int32) - want.astype(np.int32))
        print(what, "max level delta %d, %d bytes differ" % (int(d.max()), int((d > 0).sum())))
        assert d.max() <= 1, (what, int(d.max()))


# ------------------------------------------------------------------ 1. BoxScene, byte-exact
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("n", [3, 6, 10, 16, 27])
def test_box_scene_equals_the_oracle_byte_for_byte(n, s):
    """n: the tile kernel alone (3, 6), tile + redo kernel (10), a wide template (16), run-time n (27).  Six cameras a case
    (all thirteen of the dimension over s = 2, 3, 4); every camera in fp32 x 3 and in two packed formats, every format
    with two cameras at least."""
    cams = box_cameras(n)
    sc = tracern.BoxScene(n)
    sc.set_supersampling(s)
    picks = [(3 * i + s) % len(cams) for i in range(6)]
    packed = [f for f in FORMATS if f[0] != "rgbf32"]
    for j, k in enumerate(picks):
        o, a = cams[k]
        sc._set_camera_arrays(o, a)
        mean = sx.mean_colors(ob.OracleScene(n, o, a), W, H, s)
        assert np.isfinite(mean).all() and mean.min() >= 0.0 and mean.max() <= 1.0
        todo = [("rgbf32", fx.RGBF32, False), packed[(2 * j) % len(packed)], packed[(2 * j + 1) % len(packed)]]
        for name, chans, rev in todo:
            img = sup.render_host(sc, sup.fmt_of(W, H, chans, rev=rev))
            want = sx.pack(mean, chans, rev)
            assert np.array_equal(img, want), (n, s, k, name, int((img != want).sum()))


@pytest.mark.parametrize("s,n", [(8, 6), (3, 12), (5, 4), (7, 9)])
def test_box_scene_other_factors(s, n):
    """s = 8 (the largest), 3 at another dimension (a divisor that is no power of two), 5 and 7 (sample rows in flight that
    do not divide s)"""
    cams = box_cameras(n)
    sc = tracern.BoxScene(n)
    sc.set_supersampling(s)
    for k, (name, chans, rev) in ((5, FORMATS[0]), (12, FORMATS[1]), (9, FORMATS[4])):
        o, a = cams[k]
        sc._set_camera_arrays(o, a)
        img = sup.render_host(sc, sup.fmt_of(W, H, chans, rev=rev))
        want = sx.expected(ob.OracleScene(n, o, a), W, H, s, chans, rev)
        assert np.array_equal(img, want), (n, s, k, name, int((img != want).sum()))


def test_a_wide_frame_takes_the_aligned_loads_and_an_unaligned_destination_the_byte_stores():
    """width a multiple of 64 (sample rows on 16-byte boundaries); and RGB24 into a device buffer at an odd address"""
    import torch
    n, s, w, h = 6, 2, 256, 37
    o, a = box_cameras(n)[3]
    sc = tracern.BoxScene(n)
    sc.set_supersampling(s)
    sc._set_camera_arrays(o, a)
    mean = sx.mean_colors(ob.OracleScene(n, o, a), w, h, s)
    for name, chans, rev in FORMATS:
        img = sup.render_host(sc, sup.fmt_of(w, h, chans, rev=rev))
        assert np.array_equal(img, sx.pack(mean, chans, rev)), name
    fmt = sup.fmt_of(w, h, RGB24, pitch=3 * w + 5)
    buf = torch.full((fmt.pitch * h + 16,), 0x5C, dtype=torch.uint8, device="cuda")
    dest = buf[1:1 + fmt.pitch * h]
    fst = fmt._as_struct()
    _lib.check(_lib.lib().nt_render_device(sc._handle, C.c_void_p(dest.data_ptr()), fmt.pitch * h, C.byref(fst), None,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    rows = got[1:1 + fmt.pitch * h].reshape(h, fmt.pitch)
    assert np.array_equal(rows[:, :3 * w], sx.pack(mean, RGB24))
    assert (rows[:, 3 * w:] == 0x5C).all() and got[0] == 0x5C and (got[1 + fmt.pitch * h:] == 0x5C).all()


# ------------------------------------------------------------------ 2. s = 1 is the identity
def test_factor_one_is_the_identity():
    n = 6
    o, a = box_cameras(n)[4]
    for chans in (fx.RGBX8, fx.RGBF32, fx.RGB16):
        fmt = sup.fmt_of(W, H, chans)
        plain = tracern.BoxScene(n)
        plain._set_camera_arrays(o, a)
        want = sup.render_host(plain, fmt)
        sc = tracern.BoxScene(n)
        sc._set_camera_arrays(o, a)
        sc.set_supersampling(1)
        assert np.array_equal(sup.render_host(sc, fmt), want)
        sc.set_supersampling(3)
        assert not np.array_equal(sup.render_host(sc, fmt), want)
        sc.set_supersampling(1)
        assert np.array_equal(sup.render_host(sc, fmt), want)
    plain, _, _ = composite("cell600_n4")
    sc, _, _ = composite("cell600_n4")
    for chans in (fx.RGBX8, fx.RGBF32):
        fmt = sup.fmt_of(160, 90, chans)
        want = sup.render_host(plain, fmt)
        sc.set_supersampling(1)
        assert np.array_equal(sup.render_host(sc, fmt), want)
        sc.set_supersampling(3)
        assert not np.array_equal(sup.render_host(sc, fmt), want)
        sc.set_supersampling(1)
        assert np.array_equal(sup.render_host(sc, fmt), want)


# ------------------------------------------------------------------ 3. CompositeScene
LIT = dict(shadows=1, point_light_pos=[[6.0, 5.0, -7.0, 2.0]], point_light_color=[[60.0, 55.0, 50.0]])
COMPOSITE_CASES = [("cell600_n4", None, 2), ("cell600_n4", None, 3), ("cell120_n4", LIT, 2), ("feature5_n5", None, 2),
                   ("feature11_n11", None, 2), ("lit12_n12", None, 2)]


@pytest.mark.parametrize("name,params,s", COMPOSITE_CASES, ids=["%s-s%d" % (c[0], c[2]) for c in COMPOSITE_CASES])
def test_composite_scene_within_the_projects_tolerances_of_the_oracle(name, params, s):
    """each scene on its default route: the packet kernel (cell600_n4), the two-pass route (cell120_n4 with a point light and
    shadows), the faithful kernel (feature5_n5: transparent materials, Solids; its samples reach 1.26, so clamping per sample
    shows), run-time n (feature11_n11: samples up to 2.14; lit12_n12)"""
    w, h = 160, 90
    sc, osc, _ = composite(name, params)
    sc.set_supersampling(s)
    mean = sx.mean_colors(osc, w, h, s)
    assert np.isfinite(mean).all()
    if params:
        unlit = sx.mean_colors(composite(name)[1], w, h, s)
        assert np.abs(unlit - mean).max() > 0.05            # the light and its shadows are in the picture
    for chans in (fx.RGBF32, fx.RGBX8):
        img = sup.render_host(sc, sup.fmt_of(w, h, chans))
        assert_close_to(img, sx.pack(mean, chans), chans, "%s s=%d" % (name, s))


# ------------------------------------------------------------------ 4. bands
@pytest.mark.parametrize("band_rows", [32, 8])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("which", ["box6", "cell600_n4"])
def test_bands_put_together_are_the_whole_frame(which, world, band_rows):
    s = 2
    if which == "box6":
        w, h = W, H
        o, a = box_cameras(6)[7]
        sc = tracern.BoxScene(6)
        sc._set_camera_arrays(o, a)
        sc.set_supersampling(s)
        chans = fx.RGBX8 if world != 3 else fx.RGB16
        whole = sx.expected(ob.OracleScene(6, o, a), w, h, s, chans)
    else:
        w, h = 160, 90
        sc, osc, _ = composite(which)
        sc.set_supersampling(s)
        chans = fx.RGBF32 if world != 3 else fx.RGBX8
        whole = sup.render_host(sc, sup.fmt_of(w, h, chans))
        assert_close_to(whole, sx.expected(osc, w, h, s, chans), chans, which)
    bpp = whole.shape[1] // w
    pad = 20 if band_rows == 8 else 0                     # a pitch larger than W * bpp
    fmt = sup.fmt_of(w, h, chans, pitch=w * bpp + pad)
    for compact in (True, False):
        seen = np.zeros(h, bool)
        for rank in range(world):
            rows = ntd.owned_rows(h, rank, world, band_rows)
            if compact and len(rows) == 0:
                continue                                  # (117 rows are four bands of 32: ranks 4..7 of 8 own nothing)
            nrows = len(rows) if compact else h
            buf = bytearray(b"\xb3" * (fmt.pitch * nrows))
            assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc, band_rank=rank, band_world=world, band_rows=band_rows, compact=compact)
            got = np.frombuffer(bytes(buf), np.uint8).reshape(nrows, fmt.pitch)
            mine = got[:len(rows)] if compact else got[rows]
            assert np.array_equal(mine[:, :w * bpp], whole[rows]), (which, world, band_rows, compact, rank)
            assert (got[:, w * bpp:] == 0xb3).all()                                   # pitch padding
            if not compact:
                others = np.setdiff1d(np.arange(h), rows)
                assert (got[others] == 0xb3).all()                                    # rows of other ranks
            assert not seen[rows].any()
            seen[rows] = True
        assert seen.all()


# ------------------------------------------------------------------ 5. many frames and chunking
@pytest.mark.parametrize("scratch_mb", [None, 4, 1], ids=["one-chunk", "frame-chunks", "row-chunks"])
@pytest.mark.parametrize("which", ["box6", "cell600_n4"])
def test_many_frames_equal_single_renders_whatever_the_chunking(which, scratch_mb):
    """12 frames of 203 x 117 at s = 2 hold 13.7 MB of samples, a frame 1.14 MB, a row 9744 bytes: a cap of 4 MiB cuts the
    call into chunks of three frames, one of 1 MiB cuts every frame into chunks of 107 and 10 rows"""
    import torch
    s, nf, first = 2, 12, 2
    if which == "box6":
        n, chans = 6, fx.RGBX8
        sc = tracern.BoxScene(n)
        cams = box_cameras(n)[:nf]
    else:
        n, chans = 4, fx.RGBF32
        sc, _, g = composite(which)
        cams = [(g["origins"][f], g["axes"][f]) for f in range(0, 8 * nf, 8)]
    sc.set_supersampling(s)
    fmt = sup.fmt_of(W, H, chans)
    assert sc.supersampling_scratch_mb == 1024
    singles = []
    for o, a in cams:
        sc._set_camera_arrays(o, a)
        singles.append(sup.render_host(sc, fmt))
    if which == "box6":
        assert np.array_equal(singles[5], sx.expected(ob.OracleScene(n, *cams[5]), W, H, s, chans))
    singles = np.stack(singles)
    if scratch_mb is not None:
        sc.set_supersampling_scratch_mb(scratch_mb)
    origins = np.ascontiguousarray(np.stack([c[0] for c in cams]), np.float32)
    axes = np.ascontiguousarray(np.stack([c[1] for c in cams]), np.float32)
    frame_bytes = fmt.pitch * H + 64
    fst = fmt._as_struct()
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.full((nf * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, nf, origins.ctypes.data_as(_lib.f32p),
                                                  axes.ctypes.data_as(_lib.f32p), C.byref(fst), None, C.c_void_p(stream)))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, frame_bytes)
    assert np.array_equal(got[:, :fmt.pitch * H].reshape(nf, H, fmt.pitch), singles)
    assert (got[:, fmt.pitch * H:] == 0x3D).all()
    # a strict sub-range of a camera table
    table = CameraTable(n, origins, axes)
    count = nf - first - 3
    buf.fill_(0x3D)
    assert table.render(sc, buf, fmt, frame_bytes=frame_bytes, first=first, count=count)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, frame_bytes)
    assert np.array_equal(got[:count, :fmt.pitch * H].reshape(count, H, fmt.pitch), singles[first:first + count])
    assert (got[:count, fmt.pitch * H:] == 0x3D).all() and (got[count:] == 0x3D).all()
    # the single render as well, under the same cap
    sc._set_camera_arrays(*cams[7])
    assert np.array_equal(sup.render_host(sc, fmt), singles[7])


def test_a_supersampled_table_call_is_still_capturable():
    """after a warm-up call nt_render_table_device only launches kernels, also at s = 2 and also when the call is cut into
    frame chunks: captured into a HIP graph and replayed, it gives the direct call's bytes"""
    import torch
    n, s, nf = 6, 2, 6
    st = torch.cuda.Stream()
    cams = box_cameras(n)[:nf]
    origins = np.ascontiguousarray(np.stack([c[0] for c in cams]), np.float32)
    axes = np.ascontiguousarray(np.stack([c[1] for c in cams]), np.float32)
    fmt = sup.fmt_of(W, H, fx.RGBX8)
    fst = fmt._as_struct()
    sc = tracern.BoxScene(n)
    sc.set_supersampling(s)
    sc.set_supersampling_scratch_mb(4)
    tab = CameraTable(n, origins, axes)
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
    for rep in range(2):
        fb.zero_()
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(fb, ref), rep
    del gr
    assert np.array_equal(ref[4].cpu().numpy().reshape(H, fmt.pitch), sx.expected(ob.OracleScene(n, *cams[4]), W, H, s, fx.RGBX8))


# ------------------------------------------------------------------ 6. the drop-in surface
def test_the_drop_in_call_and_the_probes():
    n = 6
    o, a = box_cameras(n)[8]
    scene = tracern.BoxScene(n)
    scene._set_camera_arrays(o, a)
    scene.set_supersampling(2)
    fmt = sup.fmt_of(W, H, fx.RGBX8)
    dest = bytearray(fmt.pitch * H)
    assert ntracer_amd.BlockingRenderer().render(dest, fmt, scene)
    osc = ob.OracleScene(n, o, a)
    assert np.array_equal(np.frombuffer(bytes(dest), np.uint8).reshape(H, fmt.pitch), sx.expected(osc, W, H, 2, fx.RGBX8))
    # the probes answer for one ray and ignore the factor
    rng = np.random.default_rng(3)
    xs, ys = rng.integers(0, W, 200), rng.integers(0, H, 200)
    want = osc.colors_at(xs, ys, W, H)
    assert np.array_equal(scene.colors_at(xs, ys, W, H).view(np.uint32), want.view(np.uint32))
    for k in range(5):
        c = scene.calculate_color(int(xs[k]), int(ys[k]), W, H)
        assert tuple(c) == tuple(float(v) for v in want[k])


# ------------------------------------------------------------------ 7. abort and statistics
def test_abort_leaves_the_destination_alone_and_statistics_count_every_sample():
    import torch
    L = _lib.lib()
    sc, _, _ = composite("cell600_n4")
    sc.set_supersampling(2)
    w, h = 160, 90
    fmt = sup.fmt_of(w, h, fx.RGBX8)
    fst = fmt._as_struct()
    # the flag is already up: NT_ABORTED, nothing drawn
    dest = (C.c_char * (fmt.pitch * h))(*([0x6A] * (fmt.pitch * h)))
    flag = C.c_int(1)
    assert L.nt_render(sc._handle, dest, fmt.pitch * h, C.byref(fst), None, C.byref(flag)) == _lib.NT_ABORTED
    assert bytes(dest) == b"\x6a" * (fmt.pitch * h)
    # an abort word that is set before the call: the blocks of both stages leave when they start
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    buf = torch.full((fmt.pitch * h,), 0x6A, dtype=torch.uint8, device="cuda")
    opts = _lib.NtRenderOpts()
    opts.device = -1
    opts.abort_device = word.data_ptr()
    torch.cuda.synchronize()
    _lib.check(L.nt_render_device(sc._handle, C.c_void_p(buf.data_ptr()), fmt.pitch * h, C.byref(fst), C.byref(opts),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((buf == 0x6A).all())
    word.zero_()
    torch.cuda.synchronize()
    _lib.check(L.nt_render_device(sc._handle, C.c_void_p(buf.data_ptr()), fmt.pitch * h, C.byref(fst), C.byref(opts),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().reshape(h, fmt.pitch), sup.render_host(sc, fmt))
    # cell600_n4 is opaque, unlit and reflects nothing: one ray a sample
    sup.render_host(sc, fmt, collect_stats=True)
    st = sc.last_stats()
    assert st["rays"] == 4 * w * h and st["shadow_rays"] == 0, st
    sc.set_supersampling(1)
    sup.render_host(sc, fmt, collect_stats=True)
    assert sc.last_stats()["rays"] == w * h


# ------------------------------------------------------------------ 8. limits
def test_the_samples_of_one_row_must_fit_the_scratch_buffer():
    """The limit is on the row, not on the frame: 12 * s * s * W bytes within the cap set by set_supersampling_scratch_mb.  With a
    cap of 1 MiB and s = 2 that is W <= 21845: the first width beyond it is refused before anything is launched, the
    largest within it renders -- in chunks of one row -- and equals the oracle."""
    n, s, h = 4, 2, 3
    w_ok = (1 << 20) // (12 * s * s)
    assert 12 * s * s * w_ok <= 1 << 20 < 12 * s * s * (w_ok + 1) and w_ok == 21845
    o, a = box_cameras(n)[1]
    sc = tracern.BoxScene(n)
    sc._set_camera_arrays(o, a)
    sc.set_supersampling(s)
    sc.set_supersampling_scratch_mb(1)
    L = _lib.lib()
    fmt = sup.fmt_of(w_ok + 1, h, fx.RGBX8)
    fst = fmt._as_struct()
    dest = (C.c_char * (fmt.pitch * h))(*([0x4E] * (fmt.pitch * h)))
    assert L.nt_render(sc._handle, dest, fmt.pitch * h, C.byref(fst), None, None) == _lib.NT_E_UNSUPPORTED
    assert "nt_scene_set_supersampling_scratch_mb" in _lib.last_error() and "1 MiB" in _lib.last_error()
    assert bytes(dest) == b"\x4e" * (fmt.pitch * h)
    with pytest.raises(NotImplementedError):
        sup.render_host(sc, fmt)
    img = sup.render_host(sc, sup.fmt_of(w_ok, h, fx.RGBX8))
    want = sx.expected(ob.OracleScene(n, o, a), w_ok, h, s, fx.RGBX8)
    assert np.array_equal(img, want), int((img != want).sum())
    # the refused width is fine without supersampling, and with a larger cap
    sc.set_supersampling(1)
    sup.render_host(sc, fmt)
    sc.set_supersampling(s)
    sc.set_supersampling_scratch_mb(2)
    img = sup.render_host(sc, fmt)
    assert np.array_equal(img, sx.expected(ob.OracleScene(n, o, a), w_ok + 1, h, s, fx.RGBX8))
