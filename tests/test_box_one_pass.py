"""box_tile_kernel's 64 x 1 shape (ntracer_amd/csrc/nt_box.hpp): one wave a block works out the stretch codes of its own 64 rows,
keeps code and tie sets of slot s in lane s -- no LDS -- and renders all 64 rows in ONE pass of the row phase: masks of 64 row
bits, a slot's code and sets through v_readlane_b32, the one-face rows face by face.  Every GPU case compares whole frames
with the oracle's frame of their camera, byte for byte.

The 64 x 1 shape at small sizes: nt_render_opts.overlapped = 1, launches of at least 64 rows and 8 192 sixty-four-row waves
(nt_box_tile_geom, pinned below without a GPU).  Width 630: ten column strips, the last one with lanes past x = 629.

    shape 1   630 x 128, 416 frames   two waves a strip, stride 2: all 64 slots of both waves are valid -- bit 32 and up of
                                      every mask, v_readlane_b32 of lanes >= 32
    shape 2   630 x 200, 240 frames   four waves a strip, 50 valid slots each: the group at slots 48..51 is cut by `valid`,
                                      slots 52..63 store nothing
    shape 3   rank 3 of 8's bands of 630 x 1080 (136 rows, unevenly spaced, compact buffer), overlapped: at the 24 frames
              tests/test_box_lean_groups.py renders them with -- which nt_box_tile_geom gives 8 x 4, pinned below -- and at 328
              frames, the fewest it gives 64 x 1 (three waves a strip, stride 3; slots 46..63 of the last do not exist)

N = 3, 6, 8 (one kernel a call), 10 (the redo bitmap: the marked row's index from a slot >= 16) and 22 (no groups of four); RGBX8
everywhere, three fp32 channels and 10-10-10-2 at N = 6 on shape 1.  That the cameras -- tests/test_box_lean_groups.py's and one that
looks at an edge from the plane of symmetry of its two faces (near-tie stretches with valid sets at every N <= 8) -- put
every kind of row and group into slots >= 32 is asserted before anything is rendered, and by a test of its own that needs no
GPU: tools/box_sets_census.py's stretch_codes restates the codes wave, and slot s of wave w is row w + stride * s.

Further: a camera whose `up` is not orthogonal to `forward` (no lane passes bu^2 <= bb uu / 16: every lean row of all 64 slots
goes ray by ray); the abort word raised before the launch (shape 2: the framebuffer keeps its pattern); and the build with
-DNT_BOX_PASS_ROWS=16 -- the same driver run four times over sixteen rows -- against the default build, each in a fresh child
process, on shape 1 at N = 6."""
import ctypes as C
import functools
import os
import shutil
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
import test_box_classify_sets as tcs  # noqa: E402
import test_box_lean_groups as tlg  # noqa: E402

W = 630
COLS = (W + 63) // 64
TALL = 1080
BAND = (3, 8, 8)            # rank, world, band_rows: 136 owned rows of 1080
# (label, image height, frames): whole frames, nt_render_opts::overlapped = 1
SHAPE1 = ("630 x 128", 128, 416)
SHAPE2 = ("630 x 200", 200, 240)
BAND_FRAMES = (tlg.BAND_FRAMES, 328)
DIMS = (3, 6, 8, 10, 22)
F = np.float32


def edge_tie_camera(n):
    """looks at the edge between the faces x_0 = -1 and x_1 = +1 from the plane of symmetry between them, `right` across all the
    other coordinates (a coordinate no ray moves along has no sign, and the stretch no valid sets): on the image's middle row
    every ray enters both slabs at the same time"""
    o, axes = tlg.edge_on_camera(n, 5.0, 1.0)
    right = np.zeros(n, np.float32)
    right[2:] = 0.25
    right[2] = 1.0
    axes[0] = right / np.linalg.norm(right)
    return o, np.ascontiguousarray(axes)


def cameras(n):
    """tests/test_box_lean_groups.py's, and near-tie stretches (code 14) with valid sets at every dimension: of a 128-row frame
    the middle row is slot 32 of its wave"""
    return tlg.cameras(n) + [("edge-tie", ) + edge_tie_camera(n)]


def stride_of(count):
    """waves of a column strip = the stride between a wave's rows (nt_api.cpp: tiles * waves a block, one wave a block)"""
    return (count + 63) // 64


def slot_rows(count):
    """[wave][slot] -> row of a 64 x 1 launch of `count` rows; rows >= count do not exist"""
    il = stride_of(count)
    return np.arange(il)[:, None] + il * np.arange(64)[None, :]


def lean_ok(axes, h):
    """tests/test_box_lean_groups.py's, for a frame of any height: per column strip, every lane passes bu^2 <= bb * uu / 16"""
    right, up, fwd = (np.asarray(axes, np.float64)[k] for k in range(3))
    half_w, _, fovI = census.screen(W, h)
    x = np.minimum(np.arange(COLS * 64), W - 1)
    sx = (fovI * (x.astype(F) - half_w)).astype(F).astype(np.float64)
    base = fwd[None, :] + right[None, :] * sx[:, None]
    bb, bu, uu = (base * base).sum(1), (base * up[None, :]).sum(1), float((up * up).sum())
    return (bu * bu <= bb * uu * 0.0625).reshape(COLS, 64)


def guard_fails(axes, h, maxval=255.0):
    """tests/test_box_lean_groups.py's, for a frame of any height: [h][COLS], the culled-row quotient of some lane of the
    stretch lies within half the guard's width of a rounding boundary -- the row's guard fails whatever the device's rounding"""
    right, up, fwd = (np.asarray(axes, np.float32)[k] for k in range(3))
    half_w, half_h, fovI = census.screen(W, h)
    x = np.minimum(np.arange(COLS * 64), W - 1)
    sx = (fovI * (x.astype(F) - half_w)).astype(F).astype(np.float64)
    sy = (fovI * (np.arange(h).astype(F) - half_h)).astype(F).astype(np.float64)
    base = (fwd[None, :] + (right[None, :] * sx[:, None].astype(F)).astype(F)).astype(F).astype(np.float64)
    d = base[None, :, :] - up.astype(np.float64)[None, None, :] * sy[:, None, None]
    t = maxval * np.abs(d[:, :, 0]) / np.sqrt((d * d).sum(2))
    near = np.abs((t - np.floor(t)) - 0.5) < 0.5 * (t + 1.0) * 2.0 ** -18
    return near.reshape(h, COLS, 64).any(2)


@functools.lru_cache(maxsize=None)
def upper_half_census(n, h):
    """what the cameras of dimension n put into slots 32..63 of the waves of a 64 x 1 launch of whole 630 x h frames"""
    out = {"culled-group": 0, "one-face-group": 0, "ray-by-ray": 0, "near-tie": 0, "near-tie-with-sets": 0, "culled-with-failing-guard": 0,
           "waves-with-two-faces": 0, "mixed-face-groups": 0, "cut-groups": 0, "slots-that-do-not-exist": 0}
    rows_of = slot_rows(h)
    for _, o, a in cameras(n):
        code, sets = census.stretch_codes(o, a, W, h)
        lean = lean_ok(a, h).all(1)
        fails = guard_fails(a, h)
        for rows in rows_of:
            valid = rows < h
            out["slots-that-do-not-exist"] += int((~valid[32:]).sum())
            for col in np.nonzero(lean)[0]:
                r = np.minimum(rows, h - 1)
                c = np.where(valid, code[r, col], 99).astype(np.int64)
                face = (c >= 1) & (c <= 13)
                out["waves-with-two-faces"] += int(len(set(c[face])) >= 2)
                out["ray-by-ray"] += int((c[32:] == 15).sum())
                out["near-tie"] += int((c[32:] == 14).sum())
                out["near-tie-with-sets"] += int(((c[32:] == 14) & ((sets[r[32:], col] >> np.uint32(31)) != 0)).sum())
                out["culled-with-failing-guard"] += int(((c[32:] == 0) & fails[r[32:], col]).sum())
                for g in range(0, 64, 4):
                    cg = c[g:g + 4]
                    if face[g:g + 4].all() and len(set(cg)) >= 2:
                        out["mixed-face-groups"] += 1
                    if g < 32:
                        continue
                    if 0 < int((cg != 99).sum()) < 4:
                        out["cut-groups"] += 1
                    out["culled-group"] += int((cg == 0).all())
                    out["one-face-group"] += int(face[g:g + 4].all() and len(set(cg)) == 1)
    return out


def check_upper_half(n):
    c = upper_half_census(n, SHAPE1[1])
    assert c["slots-that-do-not-exist"] == 0, (n, c)                  # shape 1: all 64 slots of both waves
    for kind in ("culled-group", "one-face-group", "ray-by-ray", "culled-with-failing-guard", "waves-with-two-faces", "mixed-face-groups"):
        assert c[kind] >= 1, (n, kind, c)
    if n <= 8:                                                        # (NT_BOX_SETS_MAX_N: beyond, no stretch has sets)
        assert c["near-tie-with-sets"] >= 1, (n, c)
    else:                                                             # the redo bitmap, marked from a slot >= 16 (here: >= 32)
        assert c["near-tie"] >= 1, (n, c)
    c = upper_half_census(n, SHAPE2[1])
    # shape 2: 50 valid slots a wave -- the group at slots 48..51 is cut, slots 52..63 do not exist
    assert c["cut-groups"] >= 1 and c["slots-that-do-not-exist"] >= 1, (n, c)
    for kind in ("culled-group", "one-face-group", "ray-by-ray"):
        assert c[kind] >= 1, (n, kind, c)


@pytest.mark.parametrize("n", DIMS)
def test_cameras_fill_the_upper_slots_of_a_wave(n):
    """(no GPU) what the GPU tests below rely on"""
    check_upper_half(n)


def skew_cameras(n):
    """three of tests/test_box_lean_groups.py's cameras away from the cube -- culled rows and rows of one face, two faces to a
    wave -- with `forward` added to `up`: bu = base . up is then about 1, bb * uu / 16 about 1/8"""
    out = []
    for name, o, a in tlg.cameras(n):
        if name in ("far-1", "edge-on-0", "edge-on-1"):
            a = np.array(a, np.float32)
            a[1] = a[1] + a[2]
            out.append(("skew-" + name, o, np.ascontiguousarray(a)))
    return out


def test_a_skewed_up_axis_keeps_every_lane_off_the_quadratic():
    """(no GPU) bu^2 <= bb * uu / 16 fails in every lane of every strip: no wave of those frames takes the lean loops"""
    cams = skew_cameras(6)
    assert len(cams) == 3
    culled = faces = 0
    for name, o, a in cams:
        assert not lean_ok(a, SHAPE1[1]).any(), name
        # ... and the rows the lean loops would have taken are there, in slots >= 32 too
        code, _ = census.stretch_codes(o, a, W, SHAPE1[1])
        upper = code[slot_rows(SHAPE1[1])[:, 32:].reshape(-1)]
        culled += int((upper == 0).sum())
        faces += int(((upper >= 1) & (upper <= 13)).sum())
    assert culled >= 100 and faces >= 100, (culled, faces)


def test_launches_land_on_the_one_wave_shape(tmp_path):
    """(no GPU) nt_box_tile_geom (nt_device.hpp) for the launches below, and the slot-to-row map the census assumes"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "box_one_pass_probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ntracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "box_lean_groups_probe.cpp"), "-o", exe])
    own = len(ntd.owned_rows(TALL, *BAND))
    assert own == 136
    quads = [(W, SHAPE1[1], SHAPE1[2], 1), (W, SHAPE2[1], SHAPE2[2], 1), (W, own, BAND_FRAMES[0], 1), (W, own, BAND_FRAMES[1], 1),
             (W, own, BAND_FRAMES[1] - 1, 1)]
    out = subprocess.check_output([exe] + [str(v) for q in quads for v in q]).decode().split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert got == [(64, 1), (64, 1), (8, 4), (64, 1), (8, 4)], got
    # at least 8 192 sixty-four-row waves where the shape is 64 x 1
    for count, frames in ((SHAPE1[1], SHAPE1[2]), (SHAPE2[1], SHAPE2[2]), (own, BAND_FRAMES[1])):
        assert count >= 64 and COLS * stride_of(count) * frames >= 8192, (count, frames)
    src = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_api.cpp")).read()
    assert "(tg.row_count + tile_rows - 1) / tile_rows * geom.waves" in src
    assert (stride_of(SHAPE1[1]), stride_of(SHAPE2[1]), stride_of(own)) == (2, 4, 3)


# ---------------------------------------------------------------------------------------------------------------- GPU
_ORACLE = {}


def oracle_frames(n, cams_key, cams, h, chans_key, chans):
    """the oracle's W x h frames of `cams` on the device, (K, h, pitch): rendered once a module"""
    import torch
    key = (n, cams_key, h, chans_key)
    if key not in _ORACLE:
        osc = ob.OracleScene(n, cams[0][1], cams[0][2])
        frames = []
        for _, o, a in cams:
            osc.set_camera(o, a)
            frames.append(osc.render(W, h, chans, threads=sup.worker_threads()))
        _ORACLE[key] = torch.from_numpy(np.stack(frames)).cuda()
    return _ORACLE[key]


def _opts(overlapped=1, band=None, abort=None):
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world, opts.overlapped = -1, 1, overlapped
    if band is not None:
        opts.band_rank, opts.band_world, opts.band_rows, opts.compact = band[0], band[1], band[2], 1
    if abort is not None:
        opts.abort_device = abort.data_ptr()
    return opts


def _sequence(cams, frames):
    seq = tlg.frame_order(len(cams), frames)
    return (seq, np.ascontiguousarray(np.stack([cams[k][1] for k in seq]), np.float32),
            np.ascontiguousarray(np.stack([cams[k][2] for k in seq]), np.float32))


def _differences(label, pix, ref, seq, cams, rows, bpp):
    import torch
    want = ref.index_select(0, torch.tensor(seq, device="cuda"))
    if torch.equal(pix, want):
        return []
    out = []
    for f in range(len(seq)):
        if torch.equal(pix[f], want[f]):
            continue
        g, r = pix[f].cpu().numpy(), want[f].cpu().numpy()
        ys, xs = np.nonzero(g != r)
        out.append("%s: frame %d (camera %s) differs from the oracle in %d bytes, first at x=%d y=%d"
                   % (label, f, cams[seq[f]][0], len(ys), xs[0] // bpp, rows[ys[0]]))
        if len(out) > 6:
            break
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS)
def test_rows_rendered_in_one_pass_equal_the_oracle(n):
    import torch
    check_upper_half(n)
    cams = cameras(n)
    sc = tracern.BoxScene(n)
    failures = []
    formats = [("rgbx8", fx.RGBX8, 4)]
    for label, h, frames in (SHAPE1, SHAPE2):
        fmts = formats + ([("rgbf32", fx.RGBF32, 12), ("rgb10x2", tlg.RGB10X2, 4)] if n == 6 and h == SHAPE1[1] else [])
        seq, fo, fa = _sequence(cams, frames)
        for name, chans, bpp in fmts:
            ref = oracle_frames(n, "all", cams, h, name, chans)
            fmt = ntracer_amd.ImageFormat(W, h, [ntracer_amd.Channel(*c) for c in chans])
            assert fmt.pitch == W * bpp
            pix = tlg._render(sc, fmt, fo, fa, frames, h, _opts())
            failures += _differences("n=%d %s %s" % (n, name, label), pix, ref, seq, cams, np.arange(h), bpp)
            del pix
    # one rank's bands of a tall image: the rows of a wave are not evenly spaced
    name, chans, bpp = formats[0]
    rows = ntd.owned_rows(TALL, *BAND)
    ref = oracle_frames(n, "all", cams, TALL, name, chans).index_select(1, torch.from_numpy(rows).cuda())
    fmt = ntracer_amd.ImageFormat(W, TALL, [ntracer_amd.Channel(*c) for c in chans])
    for frames in BAND_FRAMES:
        seq, fo, fa = _sequence(cams, frames)
        pix = tlg._render(sc, fmt, fo, fa, frames, len(rows), _opts(band=BAND))
        failures += _differences("n=%d %s bands, %d frames" % (n, name, frames), pix, ref, seq, cams, rows, bpp)
        del pix
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_a_skewed_up_axis_sends_every_lean_row_ray_by_ray():
    n = 6
    label, h, frames = SHAPE1
    cams = skew_cameras(n)
    for _, _, a in cams:
        assert not lean_ok(a, h).any()
    sc = tracern.BoxScene(n)
    seq, fo, fa = _sequence(cams, frames)
    cams3 = cams
    failures = []
    for name, chans, bpp in (("rgbx8", fx.RGBX8, 4), ("rgbf32", fx.RGBF32, 12)):
        ref = oracle_frames(n, "skew-up", cams3, h, name, chans)
        fmt = ntracer_amd.ImageFormat(W, h, [ntracer_amd.Channel(*c) for c in chans])
        pix = tlg._render(sc, fmt, fo, fa, frames, h, _opts())
        failures += _differences("skewed up, %s %s" % (name, label), pix, ref, seq, cams3, np.arange(h), bpp)
        del pix
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_abort_word_raised_before_the_launch_leaves_the_frames_untouched():
    import torch
    n = 6
    label, h, frames = SHAPE2
    cams = cameras(n)
    sc = tracern.BoxScene(n)
    seq, fo, fa = _sequence(cams, frames)
    fmt = ntracer_amd.ImageFormat(W, h, [ntracer_amd.Channel(*c) for c in fx.RGBX8])
    fst = fmt._as_struct()
    word = torch.ones(16, dtype=torch.int32, device="cuda")
    opts = _opts(abort=word)
    frame_bytes = h * fmt.pitch
    pattern = (torch.arange(frames * frame_bytes, dtype=torch.int64, device="cuda") * 37 % 251).to(torch.uint8).view(frames, frame_bytes)
    dest = pattern.clone()

    def go():
        _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, frames, fo.ctypes.data_as(_lib.f32p),
                                                      fa.ctypes.data_as(_lib.f32p), C.byref(fst), C.byref(opts),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    go()
    assert torch.equal(dest, pattern)
    # ... and lowered again, the same call renders the frames
    word.zero_()
    torch.cuda.synchronize()
    go()
    ref = oracle_frames(n, "all", cams, h, "rgbx8", fx.RGBX8)
    failures = _differences("after the abort word went down", dest.view(frames, h, fmt.pitch), ref, seq, cams, np.arange(h), 4)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------- sixteen-row passes vs one pass
CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import torch
import ntracer_amd, fixtures as fx
from ntracer_amd import _lib, tracern
import test_box_one_pass as t
label, h, frames = t.SHAPE1
cams = t.cameras(6)
seq, fo, fa = t._sequence(cams, frames)
fmt = ntracer_amd.ImageFormat(t.W, h, [ntracer_amd.Channel(*c) for c in fx.RGBX8])
pix = t.tlg._render(tracern.BoxScene(6), fmt, fo, fa, frames, h, t._opts())
np.save(sys.argv[3], pix.cpu().numpy())
"""


@pytest.fixture(scope="session")
def pass_libraries(tmp_path_factory):
    """the default build and the build whose 64 x 1 kernels take their rows in sixteen-row passes, linked into a temporary
    directory: the BoxScene(6) unit compiled with -DNT_BOX_PASS_ROWS=16, every other object the default build's"""
    from ntracer_amd import build as ntb
    d = tmp_path_factory.mktemp("box_one_pass_libs")
    default = ntb.build(out=str(d / "default.so"))
    tag = ntb._flag_tag()
    objs = []
    for name, src, extra in ntb.units():
        o = os.path.join(ntb.OBJ, "%s.%s.o" % (name, tag))
        if name == "nt_box_6":
            o = str(d / "nt_box_6.pass16.o")
            subprocess.check_call([ntb.hipcc()] + ntb.FLAGS + ntb.EXTRA + extra + ["-DNT_BOX_PASS_ROWS=16", "-c", os.path.join(ntb.CSRC, src), "-o", o])
        objs.append(o)
    pass16 = str(d / "pass16.so")
    subprocess.check_call([ntb.hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", pass16])
    return default, pass16, d


@pytest.mark.gpu
def test_sixteen_row_passes_render_the_bytes_of_one_pass(pass_libraries):
    default, pass16, d = pass_libraries
    outs = []
    for name, lib in (("default", default), ("pass16", pass16)):
        out = str(d / (name + ".npy"))
        env = dict(os.environ, NTRACER_HIP_LIB=lib)
        subprocess.run([sys.executable, "-c", CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, check=True, timeout=600)
        outs.append(np.load(out))
    assert outs[0].shape == (SHAPE1[2], SHAPE1[1], W * 4)
    assert np.array_equal(outs[0], outs[1])
    # (that these bytes are the oracle's is test_rows_rendered_in_one_pass_equal_the_oracle's business; here: not the fill pattern)
    assert not (outs[0] == 0xA7).all(axis=(1, 2)).any()
