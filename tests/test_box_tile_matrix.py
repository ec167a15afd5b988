"""Every BoxScene tile-kernel variant against the oracle: box_tile_kernel<N, F32, ROWS, WAVES> for N = 3..24, each block
shape nt_box_tile_geom picks (fixtures.BOX_TILE_SHAPES, pinned to the C++ by tests/test_box_tile_shapes.py), both fused
formats (packed RGB, three fp32 channels), both splits of box_redo_kernel (N >= 9, packed RGB), with and without lead
frames, whole frames and one rank's bands -- and the run-time-n kernels at n = 25, 33, 63, 64.

Each case launches every frame of the shape through nt_render_frames_device and again through a camera table
(nt_render_table_device, first = 3).  Frame f is seen from camera (3 f) mod K of K = 11 stress cameras, so frames 16
apart (the lead of the middle columns) never share one; the oracle renders the K frames once per format and every frame of both
launches is compared with its camera's oracle frame byte for byte, on the device.  The destination is filled with a
sentinel first, has padded pitches, a frame stride larger than a frame and guard bytes around it: every byte outside the
pixels must still hold the sentinel afterwards.  One scene per dimension serves all of its cases, so its row tables and
scratch buffers are reused across launch geometries; an RGB16 frame (the cull and general kernels, which leave the shared
scratch dirty) is rendered and checked before each nt_render_frames_device launch."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import oracle_binding as ob
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

K = 11                      # distinct cameras a case (3 f mod K: K must not divide 48)
FIRST = 3                   # the camera table's entries before the launch's first frame
SENTINEL = 0xA7
GUARD = 4096                # bytes of sentinel before the first frame and after the last
FRAME_TAIL = 256            # frame stride = rows * pitch + FRAME_TAIL
FORMATS = (("rgbx8", fx.RGBX8), ("rgbf32", fx.RGBF32))
RUN_TIME_N = (25, 33, 63, 64)


def cam_of(f):
    return (3 * f) % K


def cameras(n):
    """K cameras: eight of fixtures.stress_cameras -- axis-aligned at the edges' distance, grazing, `up` far from orthogonal
    at three distances, no `up` at all, origins on the plane of one face and of two -- and three diagonal ones (every
    coordinate of the origin equal: near-ties between faces), at the soak's distance 2.5 and 1.6 and 1.2 a coordinate.
    (A build with a narrower stretch-code margin, -DNT_BOX_MARGIN=5e-7f, fails fp32 cases of every N on the last one.)"""
    rng = np.random.default_rng(5150 + n)
    stress = fx.stress_cameras(n, rng)
    cams = [stress[i] for i in (6, 21, 54, 56, 58, 71, 94, 111)]
    cams += [fx.diagonal_camera(n, dist, rng) for dist in (2.5, 1.6 * np.sqrt(n), 1.2 * np.sqrt(n))]
    assert len(cams) == K
    return cams


_scenes = {}
_oracle = {}
_rgb16_cam = itertools.count()


def scene(n):
    if n not in _scenes:
        _scenes.clear()
        _oracle.clear()
        _scenes[n] = (tracern.BoxScene(n), cameras(n))
    return _scenes[n]


def oracle_frames(n, cams, w, h, name, chans):
    """the K oracle frames of a (dimension, size, format) on the device: (K, h, w * bpp) bytes"""
    import torch
    key = (n, w, h, name)
    if key not in _oracle:
        osc = ob.OracleScene(n, cams[0][0], cams[0][1])
        frames = []
        for o, a in cams:
            osc.set_camera(o, a)
            frames.append(osc.render(w, h, chans, threads=sup.worker_threads()))
        _oracle[key] = torch.from_numpy(np.stack(frames)).cuda()
    return _oracle[key]


def check_rgb16_frame(sc, n, cams, k):
    """a frame the fused kernels do not take: the cull and general kernels write the scratch the fused path shares"""
    w, h = 200, 72
    o, a = cams[k]
    sc._set_camera_arrays(o, a)
    fmt = ntracer_amd.ImageFormat(w, h, [ntracer_amd.Channel(*c) for c in fx.RGB16])
    buf = bytearray(fmt.pitch * h)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
    got = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
    ref = ob.OracleScene(n, o, a).render(w, h, fx.RGB16, threads=sup.worker_threads())
    assert np.array_equal(got, ref), (n, "rgb16", k, int((got != ref).sum()))


def run_case(n, w, h, nf, pad, label, band=None):
    """both formats x both entry points of one launch shape; returns the list of failures"""
    import torch
    sc, cams = scene(n)
    seq = [cam_of(f) for f in range(-FIRST, nf)]
    # frames 16 apart (the middle columns' lead) and neighbouring frames never share a camera; the K cameras are distinct
    assert all(seq[i] != seq[i + 16] for i in range(len(seq) - 16)) and all(seq[i] != seq[i + 1] for i in range(len(seq) - 1))
    assert all(not (np.array_equal(cams[i][0], cams[j][0]) and np.array_equal(cams[i][1], cams[j][1])) for i in range(K) for j in range(i))
    so = np.ascontiguousarray(np.stack([cams[k][0] for k in seq]), np.float32)
    sa = np.ascontiguousarray(np.stack([cams[k][1] for k in seq]), np.float32)
    table = CameraTable(n, so, sa)
    fo, fa = np.ascontiguousarray(so[FIRST:]), np.ascontiguousarray(sa[FIRST:])
    if band is None:
        rows, opts, tkw = np.arange(h), None, {}
    else:
        rank, world, band_rows = band
        rows = ntd.owned_rows(h, rank, world, band_rows)
        opts = _lib.NtRenderOpts()
        opts.device, opts.band_rank, opts.band_world, opts.band_rows, opts.compact = -1, rank, world, band_rows, 1
        tkw = dict(band_rank=rank, band_world=world, band_rows=band_rows, compact=True)
    failures = []
    for name, chans in FORMATS:
        bpp = 4 if name == "rgbx8" else 12
        pitch = w * bpp + pad
        fmt = ntracer_amd.ImageFormat(w, h, [ntracer_amd.Channel(*c) for c in chans], pitch)
        fst = fmt._as_struct()
        ref = oracle_frames(n, cams, w, h, name, chans)
        if band is not None:
            ref = ref.index_select(1, torch.from_numpy(rows).cuda())
        frame_bytes = len(rows) * pitch + FRAME_TAIL
        buf = torch.empty(GUARD + nf * frame_bytes + GUARD, dtype=torch.uint8, device="cuda")
        dest = buf[GUARD:GUARD + nf * frame_bytes]
        for entry in ("frames", "table"):
            if entry == "frames":
                check_rgb16_frame(sc, n, cams, next(_rgb16_cam) % K)
            buf.fill_(SENTINEL)
            stream = torch.cuda.current_stream().cuda_stream
            if entry == "frames":
                _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, nf, fo.ctypes.data_as(_lib.f32p),
                                                              fa.ctypes.data_as(_lib.f32p), C.byref(fst), C.byref(opts) if opts is not None else None,
                                                              C.c_void_p(stream)))
            else:
                assert table.render(sc, dest, fmt, frame_bytes=frame_bytes, first=FIRST, count=nf, **tkw)
            torch.cuda.synchronize()
            pix = dest.view(nf, frame_bytes)[:, :len(rows) * pitch].view(nf, len(rows), pitch)[:, :, :w * bpp]
            bad = 0
            for f in range(nf):
                k = cam_of(f)
                if torch.equal(pix[f], ref[k]):
                    continue
                bad += 1
                if bad <= 3:
                    g, r = pix[f].cpu().numpy(), ref[k].cpu().numpy()
                    ys, xs = np.nonzero(g != r)
                    failures.append("n=%d %s %s %s: frame %d (camera %d) differs from the oracle in %d bytes, first at x=%d y=%d"
                                    % (n, label, name, entry, f, k, len(ys), xs[0] // bpp, rows[ys[0]]))
            if bad > 3:
                failures.append("n=%d %s %s %s: %d frames of %d differ" % (n, label, name, entry, bad, nf))
            pix.fill_(SENTINEL)
            stray = int(torch.count_nonzero(buf != SENTINEL))
            if stray:
                off = int(torch.nonzero(buf != SENTINEL)[0, 0]) - GUARD
                failures.append("n=%d %s %s %s: %d bytes written outside the pixels, first at offset %d from the first frame"
                                % (n, label, name, entry, stray, off))
        del buf, dest, pix
    return failures


CASES = [(n, i) for n in range(3, 25) for i in range(len(fx.BOX_TILE_SHAPES) + 1)]


def _case_id(c):
    n, i = c
    if i == len(fx.BOX_TILE_SHAPES):
        return "n%d-band" % n
    w, h, f = fx.BOX_TILE_SHAPES[i][:3]
    return "n%d-%dx%dx%d" % (n, w, h, f)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_box_tile_kernel_matrix_equals_the_oracle(case):
    n, i = case
    if i < len(fx.BOX_TILE_SHAPES):
        w, h, nf, geom, split, pad = fx.BOX_TILE_SHAPES[i]
        failures = run_case(n, w, h, nf, pad, "%dx%dx%d (%dx%d, split %d)" % (w, h, nf, geom[0], geom[1], split))
    else:
        w, h, nf, rank, world, band_rows, geom, split = fx.BOX_TILE_BAND
        failures = run_case(n, w, h, nf, 0, "%dx%dx%d rank %d/%d (%dx%d, split %d)" % (w, h, nf, rank, world, geom[0], geom[1], split),
                            band=(rank, world, band_rows))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", RUN_TIME_N)
def test_run_time_n_box_kernels_equal_the_oracle(n):
    """beyond N = 24: box_rows_kernel_var (packed RGB; at n = 64 it needs more than 64 KB of LDS, n = 63 exactly 64 KB) and
    box_kernel_var (fp32), same launches and checks as the fixed-N matrix"""
    failures = run_case(n, 1920, 1080, 40, 64, "1920x1080x40")
    assert not failures, "\n".join(failures)
