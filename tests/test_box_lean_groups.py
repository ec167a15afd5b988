"""The lean loops of box_tile_kernel (ntracer_amd/csrc/nt_box.hpp, packed RGB) take aligned groups of four slots at once: four
culled rows, or four rows of the one face K0, with one load of their four table entries and one branch on their four guards.
Groups that are mixed, cut by the last row of the launch or differ in face go through the one-row loops; a group one of whose
guards fails stores its clear rows one by one and hands the others to the ray-by-ray loop.  Every frame is compared with the
oracle's frame of its camera byte for byte.

A 630 x 200 image: the last column strip has lanes past the right edge, and 200 = 3 * 64 + 8 = 12 * 16 + 8 rows leave the last
groups of a wave cut.  Three launches for the three kinds of block shape (pinned below without a GPU) -- 24 frames (8 rows a
wave, four waves a block), 240 frames (16 rows a wave) and 240 frames of a caller with overlapped calls (64 rows a wave, one
wave a block: the bench's kernel) -- and rank 3 of 8's bands of a 630 x 1080 image, whose rows are not evenly spaced.
N = 3..8 and 10 (the route with a second kernel), and N = 22, which takes no groups (NT_BOX_LEAN_GROUPS_MAX_N = 20): every row
of its waves goes through the one-row loops, the same loops that take what the groups leave at the other dimensions.  RGBX8 and
a 10-10-10-2 format, whose fields are not bytes (the general copy of the loops; tests/fixtures.py has no such format, so it is
spelled out here).

The cameras are those of tests/test_box_classify_sets.py, for N = 6 with eight of the bench's.  That they reach every branch is
asserted before anything is rendered, and by a test of its own that needs no GPU: tools/box_sets_census.py's stretch_codes
restates the codes wave, and the slot-to-row map is the 64 x 1 launch's (a column strip's four waves deal the rows out: slot s
of wave w is row w + 4 s).  For N = 22 it is asserted instead that waves of the bands' launch hold culled, one-face and ray-by-ray
rows side by side in one half, and that every 630 x 200 launch has culled rows whose guard must fail."""
import ctypes as C
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

W, H = 630, 200
COLS = (W + 63) // 64
TALL = 1080
BAND = (3, 8, 8)            # rank, world, band_rows: 136 owned rows of 1080
BAND_FRAMES = 24
RGB10X2 = [(10, 1, 0, 0), (10, 0, 1, 0), (10, 0, 0, 1), (2, 0, 0, 0)]
FORMATS = (("rgbx8", fx.RGBX8), ("rgb10x2", RGB10X2))
DIMS = (3, 4, 5, 6, 7, 8, 10)           # dimensions whose lean loops take groups of four
NO_GROUPS = (22, )                      # ... and one beyond NT_BOX_LEAN_GROUPS_MAX_N: the one-row loops alone
# (label, frames, nt_render_opts::overlapped, block shape: rows a wave x waves a block)
LAUNCHES = (("24 frames", 24, 0, (8, 4)), ("240 frames", 240, 0, (16, 3)), ("240 frames, overlapped", 240, 1, (64, 1)))
IL = (H + 63) // 64         # the 64 x 1 launch: waves of a column strip = the stride between a wave's rows
F = np.float32


def edge_on_camera(n, dist, lift):
    """looks at the centre from above the edge between the faces x_0 = -1 and x_1 = +1, with `right` along that edge: the edge
    is a horizontal line on the screen, so that rows a few apart are one face throughout on either side of it"""
    o = np.zeros(n, np.float32)
    o[0], o[1] = -dist, lift * dist
    fwd = -o / np.linalg.norm(o)
    up = np.zeros(n, np.float32)
    up[0], up[1] = -fwd[1], fwd[0]
    axes = np.eye(n, dtype=np.float32)
    axes[0] = np.eye(n, dtype=np.float32)[2]
    axes[1], axes[2] = up, fwd
    if n > 3:
        axes[3:] = np.eye(n, dtype=np.float32)[3:]
    return o, np.ascontiguousarray(axes)


def cameras(n):
    """tests/test_box_classify_sets.py's, and cameras further from the cube -- whole groups of culled rows, of one face, and of
    one face above and another below a horizontal edge"""
    cams = tcs.cameras(n)
    rng = np.random.default_rng(4404 + n)
    cams += [("far-%d" % i, ) + tcs.looking_at_centre(n, d * v / np.linalg.norm(v), rng)
             for i, (d, v) in enumerate((d, rng.standard_normal(n)) for d in (14.0, 8.0))]
    cams += [("edge-on-%d" % i, ) + edge_on_camera(n, d, lift) for i, (d, lift) in enumerate(((5.0, 0.7), (7.0, 0.45)))]
    if n == 6:
        g = fx.load("box_n6_1920x1080")
        cams += [("bench-%d" % k, np.asarray(g["origins"][k], np.float32), np.ascontiguousarray(g["axes"][k], np.float32))
                 for k in range(0, 160, 20)]
    return cams


def frame_order(k, frames):
    """camera of every frame: neighbouring frames differ"""
    step = 2 if k % 2 else 3
    assert k % step != 0
    seq = [(step * f) % k for f in range(frames)]
    assert all(seq[i] != seq[i + 1] for i in range(frames - 1))
    return seq


def lean_ok(origin, axes):
    """per column strip: the wave takes the lean loops at all (fastsq of box_tile_kernel: bu^2 <= bb * uu / 16 in every lane)"""
    right, up, fwd = (np.asarray(axes, np.float64)[k] for k in range(3))
    half_w, _, fovI = census.screen(W, H)
    x = np.minimum(np.arange(COLS * 64), W - 1)
    sx = (fovI * (x.astype(F) - half_w)).astype(F).astype(np.float64)
    base = fwd[None, :] + right[None, :] * sx[:, None]
    bb, bu, uu = (base * base).sum(1), (base * up[None, :]).sum(1), float((up * up).sum())
    return (bu * bu <= bb * uu * 0.0625).reshape(COLS, 64).all(1)


def guard_fails(origin, axes, maxval=255.0):
    """[H][COLS]: the culled-row quotient t = maxval * |d_0| / |d| (double precision) of some lane of the stretch lies within half
    the guard's width, (t + 1) * 2^-19, of a rounding boundary k + 1/2: the row's guard fails on the device whatever its own
    rounding of t"""
    right, up, fwd = (np.asarray(axes, np.float32)[k] for k in range(3))
    half_w, half_h, fovI = census.screen(W, H)
    x = np.minimum(np.arange(COLS * 64), W - 1)
    sx = (fovI * (x.astype(F) - half_w)).astype(F).astype(np.float64)
    sy = (fovI * (np.arange(H).astype(F) - half_h)).astype(F).astype(np.float64)
    base = (fwd[None, :] + (right[None, :] * sx[:, None].astype(F)).astype(F)).astype(F).astype(np.float64)        # [x][n], as the device forms it
    d = base[None, :, :] - up.astype(np.float64)[None, None, :] * sy[:, None, None]                                 # [y][x][n]
    t = maxval * np.abs(d[:, :, 0]) / np.sqrt((d * d).sum(2))
    near = np.abs((t - np.floor(t)) - 0.5) < 0.5 * (t + 1.0) * 2.0 ** -18
    return near.reshape(H, COLS, 64).any(2)


def group_census(n):
    """what the aligned groups of four slots of the 64 x 1 launch are, over the cameras of dimension n"""
    out = {"culled": 0, "one-face": 0, "two-faces": 0, "mixed": 0, "cut": 0, "culled-with-failing-guard": 0, "failing-position": [0, 0, 0, 0]}
    slot_row = np.arange(IL)[:, None] + IL * np.arange(64)[None, :]                  # [wave][slot]
    for _, o, a in cameras(n):
        code, _ = census.stretch_codes(o, a, W, H)
        lean = lean_ok(o, a)
        fails = guard_fails(o, a)
        for w in range(IL):
            rows = slot_row[w]
            valid = rows < H
            for col in range(COLS):
                if not lean[col]:
                    continue
                c = np.where(valid, code[np.minimum(rows, H - 1), col], 99).astype(np.int64)
                for half in range(4):
                    ch = c[16 * half:16 * half + 16]
                    faces = ch[(ch >= 1) & (ch <= 13)]
                    k0 = int(faces[0]) if len(faces) else -1                            # the half's K0 + 1: its first one-face row's
                    for g in range(0, 16, 4):
                        cg = ch[g:g + 4]
                        nvalid = int((cg != 99).sum())
                        if nvalid == 0:
                            continue
                        if nvalid < 4:
                            out["cut"] += 1
                        elif (cg == 0).all():
                            out["culled"] += 1
                            f = fails[rows[16 * half + g:16 * half + g + 4], col]
                            if f.any():
                                out["culled-with-failing-guard"] += 1
                                for k in range(4):
                                    out["failing-position"][k] += int(f[k])
                        elif ((cg >= 1) & (cg <= 13)).all():
                            out["one-face" if (cg == k0).all() else "two-faces"] += 1
                        else:
                            out["mixed"] += 1
    return out


def wave_rows(rows_a_wave, waves_a_block, count):
    """[wave][slot] -> row of a launch of `count` rows with that block shape: the waves of a column strip deal the rows out
    (nt_api.cpp: the stride is tiles * waves a block); rows >= count do not exist"""
    il = (count + rows_a_wave * waves_a_block - 1) // (rows_a_wave * waves_a_block) * waves_a_block
    return np.arange(il)[:, None] + il * np.arange(rows_a_wave)[None, :]


def one_row_census(n):
    """a dimension without groups, per launch of the GPU test: the 16-row halves of a wave (8 rows a wave: its eight) that hold
    culled, one-face and ray-by-ray (code 15) rows together and, in the 630 x 200 launches, the culled rows whose guard must fail,
    over the cameras of dimension n"""
    band = ntd.owned_rows(TALL, *BAND)
    launches = [(label, shape, None) for label, _, _, shape in LAUNCHES] + [("bands", (8, 4), band)]
    out = {label: {"halves-with-all-three": 0, "culled-with-failing-guard": 0} for label, *_ in launches}
    for _, o, a in cameras(n):
        lean = lean_ok(o, a)
        fails = guard_fails(o, a)
        codes = {False: census.stretch_codes(o, a, W, H)[0], True: census.stretch_codes(o, a, W, TALL, rows=band)[0]}
        for label, (rows_a_wave, waves_a_block), owned in launches:
            code = codes[owned is not None]
            count = len(code)
            for rows in wave_rows(rows_a_wave, waves_a_block, count):
                valid = rows < count
                for col in np.nonzero(lean)[0]:
                    c = np.where(valid, code[np.minimum(rows, count - 1), col], 99).astype(np.int64)
                    if owned is None:
                        out[label]["culled-with-failing-guard"] += int(((c == 0) & fails[np.minimum(rows, H - 1), col]).sum())
                    for h0 in range(0, rows_a_wave, 16):
                        ch = c[h0:h0 + 16]
                        if (ch == 0).any() and ((ch >= 1) & (ch <= 13)).any() and (ch == 15).any():
                            out[label]["halves-with-all-three"] += 1
    return out


def check_census(n):
    if n in NO_GROUPS:
        # (a 630 x 200 frame is too flat for one column strip to show all three kinds of row: the bands of the tall image do)
        c = one_row_census(n)
        assert c["bands"]["halves-with-all-three"] >= 10, (n, c)
        assert all(c[label]["culled-with-failing-guard"] >= 1 for label, *_ in LAUNCHES), (n, c)
        return
    c = group_census(n)
    for kind in ("culled", "one-face", "two-faces", "mixed", "cut"):
        assert c[kind] >= 10, (n, kind, c)
    assert c["culled-with-failing-guard"] >= 20 and min(c["failing-position"]) >= 1, (n, c)


@pytest.mark.parametrize("n", DIMS + NO_GROUPS)
def test_cameras_reach_every_branch_of_the_group_loops(n):
    """(no GPU) what the GPU test below relies on"""
    check_census(n)


def test_launches_land_on_the_three_kinds_of_block_shape(tmp_path):
    """(no GPU) nt_box_tile_geom (nt_device.hpp) for the launches below, and the slot-to-row map the census assumes"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "box_lean_groups_probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ntracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "box_lean_groups_probe.cpp"), "-o", exe])
    own = len(ntd.owned_rows(TALL, *BAND))
    quads = [(W, H, frames, ov) for _, frames, ov, _ in LAUNCHES] + [(W, own, BAND_FRAMES, 0)]
    out = subprocess.check_output([exe] + [str(v) for q in quads for v in q]).decode().split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert got[:3] == [geom for *_, geom in LAUNCHES], got
    assert {g[0] for g in got[:3]} == {8, 16, 64}
    assert got[3] == (8, 4) and own == 136, (got, own)
    # the row table's interleave (nt_api.cpp): waves of a column strip = tiles * waves a block; one wave a block in the 64 x 1 launch
    src = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_api.cpp")).read()
    assert "(tg.row_count + tile_rows - 1) / tile_rows * geom.waves" in src
    assert IL == (H + 63) // 64 * 1 == 4


def _render(sc, fmt, fo, fa, frames, rows, opts):
    import torch
    fst = fmt._as_struct()
    frame_bytes = rows * fmt.pitch
    dest = torch.full((frames, frame_bytes), 0xA7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, frames, fo.ctypes.data_as(_lib.f32p),
                                                  fa.ctypes.data_as(_lib.f32p), C.byref(fst), C.byref(opts) if opts is not None else None,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return dest.view(frames, rows, fmt.pitch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", DIMS + NO_GROUPS)
def test_rows_rendered_in_groups_equal_the_oracle(n):
    import torch
    check_census(n)
    cams = cameras(n)
    K = len(cams)
    sc = tracern.BoxScene(n)
    osc = ob.OracleScene(n, cams[0][1], cams[0][2])
    failures = []

    def compare(label, pix, ref, seq, rows):
        want = ref.index_select(0, torch.tensor(seq, device="cuda"))
        if torch.equal(pix, want):
            return
        for f in range(len(seq)):
            if torch.equal(pix[f], want[f]):
                continue
            g, r = pix[f].cpu().numpy(), want[f].cpu().numpy()
            ys, xs = np.nonzero(g != r)
            failures.append("n=%d %s: frame %d (camera %s) differs from the oracle in %d bytes, first at x=%d y=%d"
                            % (n, label, f, cams[seq[f]][0], len(ys), xs[0] // 4, rows[ys[0]]))
            if len(failures) > 12:
                break

    def oracle_frames(w, h, chans):
        frames = []
        for _, o, a in cams:
            osc.set_camera(o, a)
            frames.append(osc.render(w, h, chans, threads=sup.worker_threads()))
        return torch.from_numpy(np.stack(frames)).cuda()             # (K, h, w * 4)

    def sequence(frames):
        seq = frame_order(K, frames)
        return (seq, np.ascontiguousarray(np.stack([cams[k][1] for k in seq]), np.float32),
                np.ascontiguousarray(np.stack([cams[k][2] for k in seq]), np.float32))

    for name, chans in FORMATS:
        ref = oracle_frames(W, H, chans)
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        assert fmt.pitch == W * 4
        for label, frames, overlapped, _ in LAUNCHES:
            seq, fo, fa = sequence(frames)
            opts = _lib.NtRenderOpts()
            opts.device, opts.band_world, opts.overlapped = -1, 1, overlapped
            pix = _render(sc, fmt, fo, fa, frames, H, opts)
            compare("%s %s" % (name, label), pix, ref, seq, np.arange(H))
            del pix
        del ref
    # one rank's bands of a tall image: the rows of a wave are not evenly spaced
    name, chans = FORMATS[0]
    rows = ntd.owned_rows(TALL, *BAND)
    ref = oracle_frames(W, TALL, chans).index_select(1, torch.from_numpy(rows).cuda())
    fmt = ntracer_amd.ImageFormat(W, TALL, [ntracer_amd.Channel(*c) for c in chans])
    seq, fo, fa = sequence(BAND_FRAMES)
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_rank, opts.band_world, opts.band_rows, opts.compact = -1, BAND[0], BAND[1], BAND[2], 1
    pix = _render(sc, fmt, fo, fa, BAND_FRAMES, len(rows), opts)
    compare("%s bands" % name, pix, ref, seq, rows)
    assert not failures, "\n".join(failures)
