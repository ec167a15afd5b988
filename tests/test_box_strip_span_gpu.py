"""box_tile_kernel's span test (ntracer_amd/csrc/nt_box.hpp, NT_BOX_STRIP_SPAN): a wave whose column strip lies outside the span
of its frame's camera (nt_box_span.hpp; a camera table carries one a frame) goes around its stretch codes and renders its rows
as culled rows.  Every frame is compared byte for byte with the oracle's frame of its camera and, through SHA-256 (one frame a
camera, the others compared with it on the device), with the frame of the build with -DNT_BOX_STRIP_SPAN=0 (a fresh child process).

Cameras: tests/test_box_strip_span_host.py's boundary cameras of a 630-wide frame -- sx_hi and sx_lo a quarter of a pixel either
side of a strip's first and last pixel, asserted from strip_span before anything is rendered --, the bench's cameras 0, 48 and
112 (n = 6), a camera inside the cube and one with the cube behind it (both frames all background, asserted), and a far, an edge-on, a diagonal and an
on-a-face camera of tests/test_box_lean_groups.py.  N = 3, 6, 8 and 10 (box_redo_kernel).  Width 630: ten strips, the last clamps.

Launches, all through a camera table (the block shapes are pinned below without a GPU):
    630 x 200   24 frames (8 x 4), 240 frames (16 x 3), 240 frames overlapped (64 x 1: 50 valid slots a wave)
    630 x 128   416 frames (16 x 4), 416 frames overlapped (64 x 1: all 64 slots valid)
    N = 6, 8    832 frames of 630 x 200 and 1664 of 630 x 128, overlapped: the kernel with the near-tie short cut
    rank 3 of 8's 8-row bands of 630 x 1080 (136 rows): 24 frames (8 x 4), 328 frames overlapped (64 x 1) and not (16 x 3)
RGBX8 everywhere; 10-10-10-2 and three fp32 channels on the 240-frame overlapped launch and on both 416-frame ones.
And the same cameras through nt_render_frames_device (host cameras: no span), through one-frame table calls and through the
scene's own camera (the kernel-argument path): the same bytes."""
import concurrent.futures
import ctypes as C
import functools
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import box_sets_census as census  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402
import test_box_one_pass as top  # noqa: E402
import test_box_strip_span_host as host  # noqa: E402
import test_box_tie_shortcut_gpu as tts  # noqa: E402

W, H, H128 = 630, 200, 128
TALL, BAND = tlg.TALL, tlg.BAND
DIMS = host.DIMS
TIE_DIMS = (6, 8)
RGBX8, RGB10X2, RGBF32 = ("rgbx8", fx.RGBX8, 4), ("rgb10x2", tlg.RGB10X2, 4), ("rgbf32", fx.RGBF32, 12)
OTHERS = ("far-1", "edge-on-0", "diagonal-1", "on-a-face")


@functools.lru_cache(maxsize=None)
def cameras(n):
    cams = [c for c in host.cameras(n) if c[0].endswith("-630") or c[0] in ("inside-cube", "cube-behind") or c[0] in OTHERS or
            c[0] in tuple("bench-%d" % k for k in host.BENCH)]
    assert len(cams) == (13 if n == 6 else 10), [c[0] for c in cams]
    return cams


def launches(n):
    """(label, image height, frames, overlapped, band, formats, block shape)"""
    out = [("200 rows, 24 frames", H, 24, 0, None, (RGBX8, ), (8, 4)),
           ("200 rows, 240 frames", H, 240, 0, None, (RGBX8, ), (16, 3)),
           ("200 rows, 240 frames, overlapped", H, 240, 1, None, (RGBX8, RGB10X2, RGBF32), (64, 1)),
           ("128 rows, 416 frames", H128, 416, 0, None, (RGBX8, RGB10X2, RGBF32), (16, 4)),
           ("128 rows, 416 frames, overlapped", H128, 416, 1, None, (RGBX8, RGB10X2, RGBF32), (64, 1)),
           ("bands, 24 frames", TALL, 24, 1, BAND, (RGBX8, ), (8, 4)),
           ("bands, 328 frames, overlapped", TALL, 328, 1, BAND, (RGBX8, ), (64, 1)),
           ("bands, 328 frames", TALL, 328, 0, BAND, (RGBX8, ), (16, 3))]
    if n in TIE_DIMS:
        out += [("200 rows, 832 frames, overlapped", H, tts.BIG_FRAMES, 1, None, (RGBX8, ), (64, 1)),
                ("128 rows, 1664 frames, overlapped", H128, tts.BIG_128_FRAMES, 1, None, (RGBX8, ), (64, 1))]
    return out


def check_cameras(n):
    """what the GPU tests rely on, from strip_span: the boundary cameras sit where their names say, the two background cameras get
    the statements they should, and the frames have strips the span clears as well as strips it keeps"""
    host.check_boundaries(n, W)
    assert host._kind(*census.strip_span(*host.inside_camera(n))) == "none"
    assert host._kind(*census.strip_span(*host.behind_camera(n))) == "empty"
    out = kept = 0
    for _, o, a in cameras(n):
        k = census.strips_kept(o, a, W)
        out += int((~k).sum())
        kept += int(k.sum())
    assert out >= 30 and kept >= 30, (n, out, kept)


@pytest.mark.parametrize("n", DIMS)
def test_cameras_sit_at_strip_boundaries(n):
    """(no GPU)"""
    check_cameras(n)


def test_launches_take_the_block_shapes_named(tmp_path):
    """(no GPU) nt_box_tile_geom for every launch above; the tie launches reach NT_BOX_TIE_SHORTCUT_MIN_WAVES"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "box_strip_span_geom_probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ntracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "box_lean_groups_probe.cpp"), "-o", exe])
    own = len(ntd.owned_rows(TALL, *BAND))
    ls = launches(6)
    quads = [(W, own if band else h, frames, ov) for _, h, frames, ov, band, _, _ in ls]
    out = subprocess.check_output([exe] + [str(v) for q in quads for v in q]).decode().split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert got == [l[6] for l in ls], got
    assert top.COLS * top.stride_of(H) * tts.BIG_FRAMES >= tts.MIN_WAVES and top.COLS * top.stride_of(H128) * tts.BIG_128_FRAMES >= tts.MIN_WAVES
    assert top.COLS * top.stride_of(H128) * 416 < tts.MIN_WAVES


# ---------------------------------------------------------------------------------------------------------------- GPU
def _table_render(sc, n, fmt, fo, fa, frames, rows, opts, first=0, count=None):
    import torch
    tab = ntracer_amd.render.CameraTable(n, fo, fa, device=torch.cuda.current_device())
    count = frames if count is None else count
    fst = fmt._as_struct()
    frame_bytes = rows * fmt.pitch
    dest = torch.full((count, frame_bytes), 0xA7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nt_render_table_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, tab._h, first, count, C.byref(fst),
                                                 C.byref(opts) if opts is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    del tab
    return dest.view(count, rows, fmt.pitch)


def render_launch(sc, n, launch, fmt_entry):
    """the frames of one launch in one format through a camera table: (pixels on the device, camera of every frame, rows)"""
    label, h, frames, ov, band, _, _ = launch
    name, chans, bpp = fmt_entry
    cams = cameras(n)
    seq, fo, fa = top._sequence(cams, frames)
    fmt = ntracer_amd.ImageFormat(W, h, [ntracer_amd.Channel(*c) for c in chans])
    assert fmt.pitch == W * bpp
    rows = ntd.owned_rows(h, *band) if band else np.arange(h)
    pix = _table_render(sc, n, fmt, fo, fa, frames, len(rows), top._opts(overlapped=ov, band=band))
    return pix, seq, rows


def frame_hashes(pix, seq):
    """a SHA-256 for every camera's first frame, and whether every other frame of the camera has that frame's bytes (compared on
    the device: the long launches are half a gigabyte)"""
    import torch
    first = {}
    for f, k in enumerate(seq):
        first.setdefault(k, f)
    same = torch.equal(pix, pix.index_select(0, torch.tensor([first[k] for k in seq], device="cuda")))
    host_pix = pix.index_select(0, torch.tensor(sorted(first.values()), device="cuda")).cpu().numpy()
    return [hashlib.sha256(f.tobytes()).hexdigest() for f in host_pix] + ["uniform" if same else "frames of one camera differ"]


def all_hashes(dims):
    """{"n <n> <launch> <format>": [a hash a frame]}: what the child process of the other build writes, and what this build is held to"""
    out = {}
    for n in dims:
        sc = tracern.BoxScene(n)
        for launch in launches(n):
            for fmt_entry in launch[5]:
                pix, seq, _ = render_launch(sc, n, launch, fmt_entry)
                out["n %d %s %s" % (n, launch[0], fmt_entry[0])] = frame_hashes(pix, seq)
                del pix
    return out


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import test_box_strip_span_gpu as t
json.dump(t.all_hashes(t.DIMS), open(sys.argv[3], "w"))
"""


@pytest.fixture(scope="module")
def span_libraries(tmp_path_factory):
    """the default build and the build without the span test, linked into a temporary directory: the BoxScene
    units of DIMS compiled with -DNT_BOX_STRIP_SPAN=0, every other object the default build's"""
    from ntracer_amd import build as ntb
    d = tmp_path_factory.mktemp("box_strip_span_libs")
    default = ntb.build(out=str(d / "default.so"))
    tag = ntb._flag_tag()
    objs, jobs = [], []
    for name, src, extra in ntb.units():
        o = os.path.join(ntb.OBJ, "%s.%s.o" % (name, tag))
        if name in tuple("nt_box_%d" % n for n in DIMS):
            o = str(d / (name + ".nospan.o"))
            jobs.append([ntb.hipcc()] + ntb.FLAGS + ntb.EXTRA + extra + ["-DNT_BOX_STRIP_SPAN=0", "-c", os.path.join(ntb.CSRC, src), "-o", o])
        objs.append(o)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(subprocess.check_call, jobs))
    without = str(d / "nospan.so")
    subprocess.check_call([ntb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", without])
    return default, without, d


@pytest.fixture(scope="module")
def nospan_hashes(span_libraries):
    default, without, d = span_libraries
    out = str(d / "nospan.json")
    subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=dict(os.environ, NTRACER_HIP_LIB=without), check=True, timeout=600)
    return json.load(open(out))


def _reference(n, h, fmt_entry, rows):
    import torch
    name, chans, _ = fmt_entry
    ref = top.oracle_frames(n, "strip-span", cameras(n), h, name, chans)
    return ref if len(rows) == h else ref.index_select(1, torch.from_numpy(rows).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_frames_equal_the_oracle_and_the_build_without_the_span(n, nospan_hashes):
    check_cameras(n)
    cams = cameras(n)
    sc = tracern.BoxScene(n)
    failures = []
    for launch in launches(n):
        for fmt_entry in launch[5]:
            label = "n %d %s %s" % (n, launch[0], fmt_entry[0])
            pix, seq, rows = render_launch(sc, n, launch, fmt_entry)
            failures += top._differences(label, pix, _reference(n, launch[1], fmt_entry, rows), seq, cams, rows, fmt_entry[2])
            mine = frame_hashes(pix, seq)
            assert mine[-1] == "uniform" and len(set(mine[:-1])) >= len(cams) - 1, label          # (inside and behind may coincide)
            if mine != nospan_hashes[label]:
                failures.append(label + ": not the bytes of the build with -DNT_BOX_STRIP_SPAN=0")
            del pix
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_background_cameras_and_the_other_camera_paths(n):
    """the inside and behind cameras' frames are all background; host cameras, one-frame table calls and the scene's own camera
    give the table path's bytes (each against the oracle)"""
    import torch
    cams = cameras(n)
    sc = tracern.BoxScene(n)
    names = [c[0] for c in cams]
    for name in ("inside-cube", "cube-behind"):
        _, o, a = cams[names.index(name)]
        assert not host.oracle_hits(n, o, a, W, H).any(), name
    failures = []
    for fmt_entry in (RGBX8, RGBF32):
        name, chans, bpp = fmt_entry
        ref = _reference(n, H, fmt_entry, np.arange(H))
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        # host cameras, the 64 x 1 launch
        seq, fo, fa = top._sequence(cams, 240)
        pix = tlg._render(sc, fmt, fo, fa, 240, H, top._opts(overlapped=1))
        failures += top._differences("n %d host cameras %s" % (n, name), pix, ref, seq, cams, np.arange(H), bpp)
        del pix
        # one frame of a table at a time (first = k), and the scene's own camera
        every = list(range(len(cams)))
        _, fo, fa = top._sequence(cams, len(cams))
        order = tlg.frame_order(len(cams), len(cams))
        for k in every:
            pix = _table_render(sc, n, fmt, fo, fa, len(cams), H, top._opts(overlapped=0), first=k, count=1)
            failures += top._differences("n %d one-frame table call %s" % (n, name), pix, ref, [order[k]], cams, np.arange(H), bpp)
            del pix
        if fmt_entry is RGBX8:
            for k, (cname, o, a) in enumerate(cams):
                sc._set_camera_arrays(o, a)
                buf = bytearray(fmt.pitch * H)
                assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
                got = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).reshape(1, H, fmt.pitch).copy()).cuda()
                failures += top._differences("n %d the scene's own camera" % n, got, ref, [k], cams, np.arange(H), bpp)
    assert not failures, "\n".join(failures)
