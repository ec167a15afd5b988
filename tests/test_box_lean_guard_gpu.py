"""box_tile_kernel's lean rows behind their per-dimension guard (ntracer_amd/csrc/nt_box.hpp: guard_clear<N>, 2^-19 at N = 3..6,
2^-18 beyond) -- on the GPU.  Every case compares whole frames with the oracle's frame of their camera, byte for byte.

Dimensions: N = 3 and 6 (the narrower guard), 8 and 10 (controls: the width they had).  Cameras: tests/test_box_lean_guard_host.py's
GPU set; asserted from its census before anything is rendered: rows with a lane between the old width and the new one and none
inside the new one (the rows whose path changes), and rows that still fail.

Formats: RGBX8, 10-10-10-2, and three fp32 channels (the control whose rows never see the guard).  Launches:
tests/test_box_edge_rows_gpu.py's -- 630 x 200 frames in 8 x 4, 16 x 3 and 64 x 1 blocks below NT_BOX_TIE_SHORTCUT_MIN_WAVES and
832 frames `overlapped` above it (64 x 1, at N = 6 the kernel with the edge rows, whose clear rows use the same guard); rank 3 of
8's bands of 630 x 1080 at 24, 328 and 1100 frames, RGBX8 -- each with the cameras staged by the call and again from a camera table.

And the build with -DNT_BOX_LEAN_GUARD_LOG2=18 against the default build, each in a fresh child process, on the same launches:
every frame equal to the first frame of its camera on the device, and those through SHA-256."""
import concurrent.futures
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import test_box_edge_rows_gpu as edge  # noqa: E402
import test_box_lean_guard_host as host  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_one_pass as top  # noqa: E402
import test_box_tie_shortcut_gpu as tie  # noqa: E402

W, H = host.W, host.H
TALL, BAND = tlg.TALL, tlg.BAND
DIMS = (3, 6, 8, 10)                    # 3, 6: 2^-19; 8, 10: 2^-18, as before
FORMATS = (("rgbx8", fx.RGBX8, 4), ("rgb10x2", tlg.RGB10X2, 4), ("rgbf32", fx.RGBF32, 12))
FRAME_LAUNCHES = edge.FRAME_LAUNCHES    # (label, frames, overlapped, block shape)
BAND_LAUNCHES = edge.BAND_LAUNCHES
PATHS = ("host cameras", "camera table")


def test_the_dimensions_lie_on_both_sides_of_the_width():
    """(no GPU)"""
    assert [host.guard_log2(n) for n in DIMS] == [19, 19, 18, 18]
    assert len(FRAME_LAUNCHES) == 4 and sorted(set(shape for _, _, _, shape in FRAME_LAUNCHES)) == [(8, 4), (16, 3), (64, 1)]
    assert len(BAND_LAUNCHES) == 3


def _render(sc, n, fmt, fo, fa, frames, rows, opts, path):
    """frames of `rows` rows each, (frames, rows, pitch) on the device, over a fill pattern"""
    import torch
    if path == PATHS[0]:
        return tlg._render(sc, fmt, fo, fa, frames, rows, opts)
    from ntracer_amd.render import CameraTable
    tab = CameraTable(n, fo, fa)
    fst = fmt._as_struct()
    frame_bytes = rows * fmt.pitch
    dest = torch.full((frames, frame_bytes), 0xA7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nt_render_table_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, tab._h, 0, frames, C.byref(fst), C.byref(opts),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    del tab
    return dest.view(frames, rows, fmt.pitch)


def render_launches(n, cams, on_frames):
    """every launch of the module at dimension n: on_frames(label, pixels (frames, rows, pitch), camera sequence, format name, bytes
    a pixel, rows of the image, band or not)"""
    sc = tracern.BoxScene(n)
    for name, chans, bpp in FORMATS:
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        assert fmt.pitch == W * bpp
        for label, frames, overlapped, _ in FRAME_LAUNCHES:
            seq, fo, fa = top._sequence(cams, frames)
            for path in PATHS:
                pix = _render(sc, n, fmt, fo, fa, frames, H, top._opts(overlapped=overlapped), path)
                on_frames("n=%d %s %s, %s" % (n, name, label, path), pix, seq, name, bpp, np.arange(H), False)
                del pix
    name, chans, bpp = FORMATS[0]
    rows = ntd.owned_rows(TALL, *BAND)
    fmt = ntracer_amd.ImageFormat(W, TALL, [ntracer_amd.Channel(*c) for c in chans])
    for frames in BAND_LAUNCHES:
        seq, fo, fa = top._sequence(cams, frames)
        for path in PATHS:
            pix = _render(sc, n, fmt, fo, fa, frames, len(rows), top._opts(band=BAND), path)
            on_frames("n=%d %s bands, %d frames, %s" % (n, name, frames, path), pix, seq, name, bpp, rows, True)
            del pix


LABELS_A_DIM = len(PATHS) * (len(FORMATS) * len(FRAME_LAUNCHES) + len(BAND_LAUNCHES))


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_lean_rows_equal_the_oracle(n):
    import torch
    host.check_census(n, gpu=True)
    cams = list(host.gpu_cameras(n))
    refs = {}

    def reference(name, band):
        if (name, band) not in refs:
            chans = {f[0]: f[1] for f in FORMATS}[name]
            ref = tie._oracle_frames(n, cams, TALL if band else H, chans)
            refs[(name, band)] = ref.index_select(1, torch.from_numpy(ntd.owned_rows(TALL, *BAND)).cuda()) if band else ref
        return refs[(name, band)]
    failures, seen = [], []

    def compare(label, pix, seq, name, bpp, rows, band):
        seen.append(label)
        failures.extend(top._differences(label, pix, reference(name, band), seq, cams, rows, bpp))
    render_launches(n, cams, compare)
    assert len(seen) == LABELS_A_DIM
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------- the build with the old width everywhere
CHILD = r"""
import hashlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_box_lean_guard_gpu as t
out = {}
def keep(label, pix, seq, name, bpp, rows, band):
    order = torch.tensor(seq, device="cuda")
    first = [seq.index(k) for k in sorted(set(seq))]
    # every frame equals the first frame of its camera (on the device); those go through SHA-256
    firsts = pix[first]
    alike = bool(torch.equal(pix, firsts.index_select(0, torch.searchsorted(torch.tensor(sorted(set(seq)), device="cuda"), order))))
    host = firsts.cpu().numpy()
    out[label] = np.array([hashlib.sha256(f.tobytes()).hexdigest() for f in host] +
                          ["alike" if alike else "frames of one camera differ", "pattern" if (host == 0xA7).all(axis=(1, 2)).any() else "rendered"])
for n in t.DIMS:
    t.render_launches(n, list(t.host.gpu_cameras(n)), keep)
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def guard_libraries(tmp_path_factory):
    """the default build and the build with the old width, linked into a temporary directory: the BoxScene units of DIMS compiled
    with -DNT_BOX_LEAN_GUARD_LOG2=18, every other object the default build's"""
    from ntracer_amd import build as ntb
    d = tmp_path_factory.mktemp("box_lean_guard_libs")
    default = ntb.build(out=str(d / "default.so"))
    tag = ntb._flag_tag()
    objs, jobs = [], []
    for name, src, extra in ntb.units():
        o = os.path.join(ntb.OBJ, "%s.%s.o" % (name, tag))
        if name in ("nt_box_%d" % n for n in DIMS):
            o = str(d / (name + ".guard18.o"))
            jobs.append([ntb.hipcc()] + ntb.FLAGS + ntb.EXTRA + extra + ["-DNT_BOX_LEAN_GUARD_LOG2=18", "-c", os.path.join(ntb.CSRC, src), "-o", o])
        objs.append(o)
    assert len(jobs) == len(DIMS)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(subprocess.check_call, jobs))
    old = str(d / "guard18.so")
    subprocess.check_call([ntb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", old])
    return default, old, d


@pytest.mark.gpu
def test_the_build_with_the_old_width_renders_the_same_bytes(guard_libraries):
    default, old, d = guard_libraries
    for n in DIMS:
        host.check_census(n, gpu=True)
    outs = []
    for name, lib in (("default", default), ("guard18", old)):
        out = os.path.join(str(d), name + ".npz")
        env = dict(os.environ, NTRACER_HIP_LIB=lib)
        subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, check=True, timeout=600)
        outs.append(dict(np.load(out)))
    labels = sorted(outs[0])
    assert labels == sorted(outs[1]) and len(labels) == len(DIMS) * LABELS_A_DIM
    for label in labels:
        a, b = outs[0][label], outs[1][label]
        assert a[-1] == "rendered" and b[-1] == "rendered", label
        assert a[-2] == "alike" and b[-2] == "alike", label
        assert np.array_equal(a, b), label
        assert len(set(a[:-2])) == len(host.gpu_cameras(int(label.split()[0][2:]))), label
