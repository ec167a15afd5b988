"""box_tile_kernel's near-tie rows whose stretch carries the "sure hit" bit (ntracer_amd/csrc/nt_box.hpp, NT_BOX_SETS_SURE;
packed RGB, N = 6 and 8): stored from the smallest and the largest |dir_i| over T when both give the same bytes, without the
reference's square root and divisions.  Every case compares whole frames with the oracle's frame of their camera, byte for byte.

Cameras: tests/test_box_tie_shortcut_host.py's -- the bench's rotation at frames 48, 112 (flagged rows), 64, 96 (tie sets with
an axis at |o| >= 7: not flagged), frame 48 from 1.15 times the distance (tie axes beyond the limit of 4.5: not flagged) and
frames 52 and 108 (flagged rows that fall back) -- in N = 6 and 8 and, as controls in which neither the bit nor the branch
exists, N = 5, 7 and 10.  Asserted from the census before
anything is rendered: flagged near-tie rows, unflagged ones, and flagged rows in which some ray's candidate pixels differ (the
wave falls back to the reference's arithmetic) -- on the frames and on the rank's bands.

Launches.  The short cut is in box_tile_kernel<N, false, 64, 1, true>, which launch_box_fixed takes for 64 x 1 launches of
NT_BOX_TIE_SHORTCUT_MIN_WAVES sixty-four-row waves or more (read from the header below): 832 frames of 630 x 200 -- ragged on
both sides, 40 waves a frame -- and 1100 frames of rank 3 of 8's bands of 630 x 1080 (30 waves a frame), both `overlapped`.
Below that, and in the other block shapes, the kernel without runs: tests/test_box_lean_groups.py's three launches of 630 x 200
frames (8 x 4, 16 x 3 and 64 x 1 blocks, pinned there without a GPU) and the bands at the two frame counts of
tests/test_box_one_pass.py (8 x 4 and 64 x 1).  RGBX8 and 10-10-10-2 (the generic packer) on the frames, RGBX8 on the bands.

And the build with -DNT_BOX_TIE_SHORTCUT=0 against the default build, each in a fresh child process, on 1664 frames of 630 x 128
(64 x 1, two waves a strip: 33 280 waves) at N = 6, frame by frame through SHA-256."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import oracle_binding as ob
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_one_pass as top  # noqa: E402
import test_box_tie_shortcut_host as host  # noqa: E402

W, H = tlg.W, tlg.H                     # 630 x 200
TALL, BAND = tlg.TALL, tlg.BAND
BAND_FRAMES = top.BAND_FRAMES           # 24: 8 x 4; 328: 64 x 1
MIN_WAVES = int(re.search(r"#define NT_BOX_TIE_SHORTCUT_MIN_WAVES (\d+)", open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_box.hpp")).read()).group(1))
BIG_FRAMES, BIG_BAND_FRAMES, BIG_128_FRAMES = 832, 1100, 1664       # launches that take the kernel with the short cut
SHORTCUT_DIMS = (6, 8)                  # NT_BOX_TIE_SHORTCUT_MIN_N .. _MAX_N without 7 (nt_inst_box.hip)
CONTROL_DIMS = (5, 7, 10)
FORMATS = (("rgbx8", fx.RGBX8), ("rgb10x2", tlg.RGB10X2))


@functools.lru_cache(maxsize=None)
def row_census(n, h, band):
    """near-tie stretch-rows of the cameras in a 630 x h frame (band: the rank's rows of it): flagged, unflagged, and flagged ones
    in which some ray's candidate pixels differ, per format"""
    rows = ntd.owned_rows(h, *BAND) if band else None
    ys = np.arange(h) if rows is None else rows
    out = {"flagged": 0, "unflagged": 0, "differ-rgbx8": 0, "differ-rgb10x2": 0}
    for _, o, a in host.cameras(n):
        code, sets, sure = census.stretch_sure_hit(o, a, W, h, rows=rows)
        tie = code == 14
        out["flagged"] += int((tie & sure).sum())
        out["unflagged"] += int((tie & ~sure).sum())
        for r, col in zip(*np.nonzero(tie & sure)):
            for name, chans in FORMATS:
                out["differ-" + name] += int(host.candidates_differ(o, a, W, h, int(ys[r]), int(col), int(sets[r, col]), chans))
    return out


def check_census(n):
    frames, bands = row_census(n, H, False), row_census(n, TALL, True)
    assert frames["unflagged"] >= 100 and bands["unflagged"] >= 20, (n, frames, bands)
    if n in SHORTCUT_DIMS:
        assert frames["flagged"] >= 100 and bands["flagged"] >= 20, (n, frames, bands)
        assert frames["differ-rgbx8"] >= 5 and frames["differ-rgb10x2"] >= 5 and bands["differ-rgbx8"] >= 1, (n, frames, bands)
        # ... and rows that do not fall back
        assert frames["differ-rgbx8"] < frames["flagged"] // 2 and frames["differ-rgb10x2"] < frames["flagged"], (n, frames)


@pytest.mark.parametrize("n", SHORTCUT_DIMS + CONTROL_DIMS)
def test_cameras_show_flagged_unflagged_and_fall_back_rows(n):
    """(no GPU) what the GPU tests below rely on"""
    check_census(n)


def test_the_big_launches_reach_the_kernel_with_the_short_cut():
    """(no GPU) waves of a 64 x 1 launch = column strips x ceil(rows / 64) x frames, against the header's threshold"""
    own = len(ntd.owned_rows(TALL, *BAND))
    assert own == 136 and MIN_WAVES == 32768
    assert top.COLS * top.stride_of(H) * BIG_FRAMES >= MIN_WAVES > top.COLS * top.stride_of(H) * max(f for _, f, _, _ in tlg.LAUNCHES)
    assert top.COLS * top.stride_of(own) * BIG_BAND_FRAMES >= MIN_WAVES > top.COLS * top.stride_of(own) * max(BAND_FRAMES)
    assert top.COLS * top.stride_of(top.SHAPE1[1]) * BIG_128_FRAMES >= MIN_WAVES


def _oracle_frames(n, cams, h, chans):
    import torch
    osc = ob.OracleScene(n, cams[0][1], cams[0][2])
    frames = []
    for _, o, a in cams:
        osc.set_camera(o, a)
        frames.append(osc.render(W, h, chans, threads=sup.worker_threads()))
    return torch.from_numpy(np.stack(frames)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHORTCUT_DIMS + CONTROL_DIMS)
def test_near_tie_rows_equal_the_oracle(n):
    import torch
    check_census(n)
    cams = list(host.cameras(n))
    sc = tracern.BoxScene(n)
    failures = []
    for name, chans in FORMATS:
        ref = _oracle_frames(n, cams, H, chans)
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        assert fmt.pitch == W * 4
        for label, frames, overlapped, _ in tlg.LAUNCHES + (("%d frames, overlapped" % BIG_FRAMES, BIG_FRAMES, 1, (64, 1)), ):
            seq, fo, fa = top._sequence(cams, frames)
            pix = tlg._render(sc, fmt, fo, fa, frames, H, top._opts(overlapped=overlapped))
            failures += top._differences("n=%d %s %s" % (n, name, label), pix, ref, seq, cams, np.arange(H), 4)
            del pix
        del ref
    # one rank's bands of a tall image
    name, chans = FORMATS[0]
    rows = ntd.owned_rows(TALL, *BAND)
    ref = _oracle_frames(n, cams, TALL, chans).index_select(1, torch.from_numpy(rows).cuda())
    fmt = ntracer_amd.ImageFormat(W, TALL, [ntracer_amd.Channel(*c) for c in chans])
    for frames in BAND_FRAMES + (BIG_BAND_FRAMES, ):
        seq, fo, fa = top._sequence(cams, frames)
        pix = tlg._render(sc, fmt, fo, fa, frames, len(rows), top._opts(band=BAND))
        failures += top._differences("n=%d %s bands, %d frames" % (n, name, frames), pix, ref, seq, cams, rows, 4)
        del pix
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------- the build without the short cut
CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import ntracer_amd, fixtures as fx
from ntracer_amd import tracern
import test_box_tie_shortcut_gpu as t
h, frames = t.top.SHAPE1[1], t.BIG_128_FRAMES
cams = list(t.host.cameras(6))
seq, fo, fa = t.top._sequence(cams, frames)
fmt = ntracer_amd.ImageFormat(t.W, h, [ntracer_amd.Channel(*c) for c in fx.RGBX8])
pix = t.tlg._render(tracern.BoxScene(6), fmt, fo, fa, frames, h, t.top._opts())
host = pix.cpu().numpy()
np.save(sys.argv[3], np.array([hashlib.sha256(f.tobytes()).hexdigest() for f in host] + ["pattern" if (host == 0xA7).all(axis=(1, 2)).any() else "rendered"]))
"""


@pytest.fixture(scope="module")
def shortcut_libraries(tmp_path_factory):
    """the default build and the build without the bit and the branch, linked into a temporary directory: the BoxScene(6) unit
    compiled with -DNT_BOX_TIE_SHORTCUT=0, every other object the default build's"""
    from ntracer_amd import build as ntb
    d = tmp_path_factory.mktemp("box_tie_shortcut_libs")
    default = ntb.build(out=str(d / "default.so"))
    tag = ntb._flag_tag()
    objs = []
    for name, src, extra in ntb.units():
        o = os.path.join(ntb.OBJ, "%s.%s.o" % (name, tag))
        if name == "nt_box_6":
            o = str(d / "nt_box_6.noshortcut.o")
            subprocess.check_call([ntb.hipcc()] + ntb.FLAGS + ntb.EXTRA + extra + ["-DNT_BOX_TIE_SHORTCUT=0", "-c", os.path.join(ntb.CSRC, src), "-o", o])
        objs.append(o)
    without = str(d / "noshortcut.so")
    subprocess.check_call([ntb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", without])
    return default, without, d


@pytest.mark.gpu
def test_the_build_without_the_short_cut_renders_the_same_bytes(shortcut_libraries):
    default, without, d = shortcut_libraries
    h, frames = top.SHAPE1[1], BIG_128_FRAMES
    # (630 x 128: flagged near-tie rows there too)
    flagged = sum(int(((code == 14) & sure).sum()) for code, _, sure in (census.stretch_sure_hit(o, a, W, h) for _, o, a in host.cameras(6)))
    assert flagged >= 100, flagged
    outs = []
    for name, lib in (("default", default), ("noshortcut", without)):
        out = str(d / (name + ".npy"))
        env = dict(os.environ, NTRACER_HIP_LIB=lib)
        subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, check=True, timeout=600)
        outs.append(np.load(out))
    # one SHA-256 a frame, and whether any frame kept the fill pattern
    assert outs[0].shape == (frames + 1, ) and outs[0][-1] == "rendered"
    assert np.array_equal(outs[0], outs[1])
    assert len(set(outs[0][:-1])) == len(host.cameras(6))
