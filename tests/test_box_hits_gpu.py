"""BoxScene hit buffers (BoxScene.face_hits, nt_box_hits*) on the GPU against the oracle.

The expected records never come from the library: tests/box_hit_cases.py works them out for every pixel from the oracle's
primary_dir, by the rule in include/ntracer_hip.h, and test_box_hits_host.py holds the colour each one stands for against the
oracle's own bit for bit.  Records must be equal exactly -- dist bit for bit, item, lane, every pixel -- with no tolerance: the
kernels do the reference's arithmetic in the reference's order, which is BoxScene's standing of parity.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import box_hit_cases as bc
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd.render import CameraTable

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
PAD = 5                         # records behind a frame


def scene(n, k):
    sc = tracern.BoxScene(n)
    sc.set_fov(bc.FOV)
    sc._set_camera_arrays(*bc.camera(n, k))
    return sc


def _assert_records(got, want, label):
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d records differ, first at pixel %d: got %r (dist %r), oracle %r (dist %r)" % (
        label, len(bad), len(want), bad[0], got[bad[0]].tolist(), got[bad[0], :1].view(np.float32)[0], want[bad[0]].tolist(),
        want[bad[0], :1].view(np.float32)[0])


def _device_records(sc, w, h, abort=None):
    """nt_box_hits_device on a sentinel-filled buffer with PAD records behind it: the raw buffer"""
    import torch
    buf = torch.full((w * h + PAD, 4), SENTINEL, dtype=torch.int32, device="cuda")
    opts = _lib.NtRenderOpts()
    opts.device = -1
    if abort is not None:
        opts.abort_device = abort.data_ptr()
    _lib.check(_lib.lib().nt_box_hits_device(sc._handle, w, h, C.c_void_p(buf.data_ptr()), C.byref(opts),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _both_forms(n, label_env=""):
    for v in bc.views(n):
        _, k, (w, h) = v
        label = bc.view_id(v) + label_env
        want = bc.records(n, k, w, h)
        sc = scene(n, k)
        fh = sc.face_hits(w, h)
        _assert_records(fh.records, want, label + " host")
        e = bc.expected(n, k, w, h)
        assert np.array_equal(fh.dist.view(np.uint32), e["dist"].view(np.uint32)) and np.array_equal(fh.axis, e["item"])
        assert np.array_equal(fh.side, e["lane"]) and np.array_equal(fh.hit, e["item"] >= 0)
        raw = _device_records(sc, w, h)
        _assert_records(raw[:w * h], want, label + " device")
        assert (raw[w * h:] == SENTINEL).all(), label + ": a record behind the frame was written"


# ------------------------------------------------------------------ 1. every case, both forms
@pytest.mark.parametrize("n", bc.DIMS)
def test_records_equal_the_oracle(n):
    with pytest.MonkeyPatch.context() as mp:
        sup.set_switches(mp, ("NTRACER_FORCE_VAR",), {})
        _both_forms(n)


@pytest.mark.parametrize("n", (6, 10))
def test_records_equal_the_oracle_on_the_run_time_n_kernel(n):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NTRACER_FORCE_VAR", "1")
        _both_forms(n, " NTRACER_FORCE_VAR=1")


# ------------------------------------------------------------------ 2. camera tables
TABLE_CASES = [(3, {}), (6, {}), (6, {"NTRACER_FORCE_VAR": "1"}), (24, {}), (25, {}), (64, {})]


@pytest.mark.parametrize("n,env", TABLE_CASES, ids=["n%d%s" % (n, "-force-var" if e else "") for n, e in TABLE_CASES])
def test_three_frames_of_a_camera_table_with_a_padded_stride(n, env):
    import torch
    ks = (2, 4, 0, 1)                                   # a table of four; frames 1..3 of it
    cams = [bc.camera(n, k) for k in ks]
    table = CameraTable(n, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    with pytest.MonkeyPatch.context() as mp:
        sup.set_switches(mp, ("NTRACER_FORCE_VAR",), env)
        sc = scene(n, 3)                                # the scene's own camera sees nothing: the table's are what counts
        for w, h in ((37, 21), bc.BIG):
            stride = w * h + PAD
            out = torch.full((3 * stride, 4), SENTINEL, dtype=torch.int32, device="cuda")
            fh = sc.face_hits(w, h, out=out, table=table, first=1, count=3, frame_stride=stride)
            torch.cuda.synchronize()
            assert fh.records is out and fh.frames == 3 and tuple(fh.axis.shape) == (3, h, w) and fh.dist.dtype == torch.float32
            got = out.cpu().numpy().reshape(3, stride, 4)
            for f, k in enumerate(ks[1:]):
                _assert_records(got[f, :w * h], bc.records(n, k, w, h), "n%d table frame %d (%s) %dx%d" % (n, f, bc.CAMERA_NAMES[k], w, h))
                assert np.array_equal(fh.axis[f].cpu().numpy(), bc.expected(n, k, w, h)["item"])
            assert (got[:, w * h:] == SENTINEL).all(), "records between the frames were written"
            assert not np.array_equal(got[0, :w * h], got[1, :w * h])
            nrm = fh.normal(w // 2, h // 2, frame=1)    # frame 1: one face everywhere
            e = bc.expected(n, 0, w, h)
            axis, side = int(e["item"][h // 2, w // 2]), int(e["lane"][h // 2, w // 2])
            assert list(nrm) == [(1.0 if side else -1.0) if j == axis else 0.0 for j in range(n)]


def test_the_table_form_validates_its_table():
    import torch
    L = _lib.lib()
    n = 5
    sc = scene(6, 2)
    cams = [bc.camera(6, k) for k in (0, 2)]
    table = CameraTable(6, np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    other = CameraTable(n, np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None])
    w, h = 9, 7
    out = torch.full((2 * (w * h + PAD), 4), SENTINEL, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda tab, stride, first, count: L.nt_box_hits_table_device(sc._handle, w, h, C.c_void_p(out.data_ptr()), stride, tab, first, count,
                                                                        None, stream)
    assert call(other._h, w * h, 0, 1) == _lib.NT_E_INVALID and "dimensions" in _lib.last_error()
    for first, count in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
        assert call(table._h, w * h, first, count) == _lib.NT_E_INVALID, (first, count)
    assert call(table._h, w * h - 1, 0, 2) == _lib.NT_E_INVALID and "frame_stride_records" in _lib.last_error()
    assert call(table._h, 1 << 30, 0, 2) == _lib.NT_E_INVALID and "2^31" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(table._h, w * h + PAD, 0, 2) == 0
    torch.cuda.synchronize()
    _assert_records(out.cpu().numpy().reshape(2, w * h + PAD, 4)[1, :w * h], bc.records(6, 2, w, h), "after the refusals")


# ------------------------------------------------------------------ 3. the Python device form, abort, repeatability
def test_the_python_device_form_stays_on_the_device():
    import torch
    n, k, (w, h) = 10, 2, (37, 21)
    sc = scene(n, k)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fh = sc.face_hits(w, h, device=torch.device("cuda"))
    st.synchronize()
    assert fh.records.is_cuda and fh.dist.is_cuda and fh.dist.dtype == torch.float32 and fh.hit.dtype == torch.bool
    assert tuple(fh.dist.shape) == (h, w) and fh.frames is None
    _assert_records(fh.records.cpu().numpy(), bc.records(n, k, w, h), "python device form")
    e = bc.expected(n, k, w, h)
    y, x = [int(v[0]) for v in np.nonzero(e["item"] >= 0)]
    assert list(fh.normal(x, y)).index(1.0 if e["lane"][y, x] else -1.0) == int(e["item"][y, x])
    y, x = [int(v[0]) for v in np.nonzero(e["item"] < 0)]
    assert fh.normal(x, y) is None


def test_the_settings_the_pass_ignores():
    """one ray a pixel whatever the supersampling factor says, and no trace of the face-line setting"""
    n, k, (w, h) = 6, 2, (37, 21)
    sc = scene(n, k)
    sc.set_supersampling(3)
    sc.set_face_lines((1, 0, 0), 0.5)
    _assert_records(sc.face_hits(w, h).records, bc.records(n, k, w, h), "supersampling 3, face lines on")


@pytest.mark.parametrize("env", ({}, {"NTRACER_FORCE_VAR": "1"}), ids=("", "force-var"))
def test_an_abort_word_raised_before_the_launch_leaves_the_records_untouched(env):
    import torch
    n, k, (w, h) = 6, 2, (37, 21)
    with pytest.MonkeyPatch.context() as mp:
        sup.set_switches(mp, ("NTRACER_FORCE_VAR",), env)
        sc = scene(n, k)
        word = torch.ones(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        raw = _device_records(sc, w, h, abort=word)
        assert (raw == SENTINEL).all()
        word.zero_()
        torch.cuda.synchronize()
        raw = _device_records(sc, w, h, abort=word)
        _assert_records(raw[:w * h], bc.records(n, k, w, h), "after the abort word went down")
        assert (raw[w * h:] == SENTINEL).all()
