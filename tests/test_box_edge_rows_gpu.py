"""box_tile_kernel's edge rows (ntracer_amd/csrc/nt_box.hpp, NT_BOX_EDGE_ROWS; packed RGB, N = 6, the 64 x 1 kernel of large launches): rows
sorted ray by ray whose stretch has two coordinates in C are classified on those two axes, set by set, and stored through the
lean rows' quotient.  Every case compares whole frames with the oracle's frame of their camera, byte for byte.

Cameras: tests/test_box_edge_rows_host.py's, in N = 6 and, as controls whose kernels do not have the path, N = 7, 5 and 8.
Asserted from the census before anything is rendered: edge rows with T on the lower axis of C, on the upper one and on both,
with and without an unclear lane, and clear rows whose guard must fail.

Launches: tests/test_box_tie_shortcut_gpu.py's.  630 x 200 frames in the three launches of tests/test_box_lean_groups.py (8 x 4,
16 x 3 and 64 x 1 blocks: below NT_BOX_TIE_SHORTCUT_MIN_WAVES, the kernels without the near-tie short cut and without edge
rows) and 832 frames `overlapped` (64 x 1, above it: the kernel with both), RGBX8 and 10-10-10-2; rank 3 of 8's bands of 630 x 1080 at 24, 328 (64 x 1,
below) and 1100 frames (64 x 1, above), RGBX8.

And the build with -DNT_BOX_EDGE_ROWS=0 against the default build, each in a fresh child process, on the same launches at N = 6,
frame by frame through SHA-256."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ntracer_amd
from ntracer_amd import tracern
from ntracer_amd import distributed as ntd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import test_box_edge_rows_host as host  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_one_pass as top  # noqa: E402
import test_box_tie_shortcut_gpu as tie  # noqa: E402

W, H = host.W, host.H
TALL, BAND = host.TALL, host.BAND
FORMATS = tie.FORMATS
FRAME_LAUNCHES = tlg.LAUNCHES + (("%d frames, overlapped" % tie.BIG_FRAMES, tie.BIG_FRAMES, 1, (64, 1)), )
BAND_LAUNCHES = tie.BAND_FRAMES + (tie.BIG_BAND_FRAMES, )


def test_the_launches_lie_on_both_sides_of_the_short_cut_s_threshold():
    """(no GPU) 64 x 1 launches below and above NT_BOX_TIE_SHORTCUT_MIN_WAVES, on whole frames and on the bands"""
    own = len(ntd.owned_rows(TALL, *BAND))
    waves = lambda rows, frames: top.COLS * top.stride_of(rows) * frames
    below = [f for _, f, _, shape in tlg.LAUNCHES if shape == (64, 1)]
    assert below and all(waves(H, f) < tie.MIN_WAVES for f in below) and waves(H, tie.BIG_FRAMES) >= tie.MIN_WAVES
    assert waves(own, max(tie.BAND_FRAMES)) < tie.MIN_WAVES <= waves(own, tie.BIG_BAND_FRAMES)


def render_launches(n, cams, on_frames):
    """every launch of the module at dimension n: on_frames(label, pixels (frames, rows, pitch), camera sequence, format name,
    rows of the image, band or not)"""
    sc = tracern.BoxScene(n)
    for name, chans in FORMATS:
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        assert fmt.pitch == W * 4
        for label, frames, overlapped, _ in FRAME_LAUNCHES:
            seq, fo, fa = top._sequence(cams, frames)
            pix = tlg._render(sc, fmt, fo, fa, frames, H, top._opts(overlapped=overlapped))
            on_frames("n=%d %s %s" % (n, name, label), pix, seq, name, np.arange(H), False)
            del pix
    name, chans = FORMATS[0]
    rows = ntd.owned_rows(TALL, *BAND)
    fmt = ntracer_amd.ImageFormat(W, TALL, [ntracer_amd.Channel(*c) for c in chans])
    for frames in BAND_LAUNCHES:
        seq, fo, fa = top._sequence(cams, frames)
        pix = tlg._render(sc, fmt, fo, fa, frames, len(rows), top._opts(band=BAND))
        on_frames("n=%d %s bands, %d frames" % (n, name, frames), pix, seq, name, rows, True)
        del pix


@pytest.mark.gpu
@pytest.mark.parametrize("n", host.SETS_DIMS + host.CONTROL_DIMS)
def test_edge_rows_equal_the_oracle(n):
    import torch
    host.check_census(n)
    cams = list(host.cameras(n))
    refs = {}

    def reference(name, band):
        if (name, band) not in refs:
            chans = dict(FORMATS)[name]
            ref = tie._oracle_frames(n, cams, TALL if band else H, chans)
            refs[(name, band)] = ref.index_select(1, torch.from_numpy(ntd.owned_rows(TALL, *BAND)).cuda()) if band else ref
        return refs[(name, band)]
    failures = []

    def compare(label, pix, seq, name, rows, band):
        failures.extend(top._differences(label, pix, reference(name, band), seq, cams, rows, 4))
    render_launches(n, cams, compare)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------- the build without the edge rows
CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_box_edge_rows_gpu as t
out = {}
def keep(label, pix, seq, name, rows, band):
    host = pix.cpu().numpy()
    out[label] = np.array([hashlib.sha256(f.tobytes()).hexdigest() for f in host] + ["pattern" if (host == 0xA7).all(axis=(1, 2)).any() else "rendered"])
for n in t.host.EDGE_DIMS:
    t.render_launches(n, list(t.host.cameras(n)), keep)
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def edge_libraries(tmp_path_factory):
    """the default build and the build without the edge rows, linked into a temporary directory: the BoxScene(6) unit
    compiled with -DNT_BOX_EDGE_ROWS=0, every other object the default build's"""
    from ntracer_amd import build as ntb
    d = tmp_path_factory.mktemp("box_edge_rows_libs")
    default = ntb.build(out=str(d / "default.so"))
    tag = ntb._flag_tag()
    objs = []
    for name, src, extra in ntb.units():
        o = os.path.join(ntb.OBJ, "%s.%s.o" % (name, tag))
        if name in ("nt_box_%d" % n for n in host.EDGE_DIMS):
            o = str(d / (name + ".noedge.o"))
            subprocess.check_call([ntb.hipcc()] + ntb.FLAGS + ntb.EXTRA + extra + ["-DNT_BOX_EDGE_ROWS=0", "-c", os.path.join(ntb.CSRC, src), "-o", o])
        objs.append(o)
    without = str(d / "noedge.so")
    subprocess.check_call([ntb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", without])
    return default, without, d


def compare_libraries(default, without, d):
    """render_launches under each library in a child process of its own; one SHA-256 a frame, and whether any frame kept the fill pattern"""
    outs = []
    for name, lib in (("default", default), ("noedge", without)):
        out = os.path.join(str(d), name + ".npz")
        env = dict(os.environ, NTRACER_HIP_LIB=lib)
        subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, check=True, timeout=600)
        outs.append(dict(np.load(out)))
    labels = sorted(outs[0])
    assert labels == sorted(outs[1]) and len(labels) == len(host.EDGE_DIMS) * (len(FORMATS) * len(FRAME_LAUNCHES) + len(BAND_LAUNCHES))
    for label in labels:
        a, b = outs[0][label], outs[1][label]
        assert a[-1] == "rendered" and b[-1] == "rendered", label
        assert np.array_equal(a, b), label
        assert len(set(a[:-1])) == len(host.cameras(6)), label


@pytest.mark.gpu
def test_the_build_without_edge_rows_renders_the_same_bytes(edge_libraries):
    for n in host.EDGE_DIMS:
        host.check_census(n)
    compare_libraries(*edge_libraries)
