"""box_classify_sets (ntracer_amd/csrc/nt_box.hpp): the rows of box_tile_kernel that are sorted ray by ray (code 15) are sorted on
the stretch's sets -- the faces T that can be a ray's answer, the coordinates C one of them could fail at -- where the codes
wave found valid ones (N = 6 and 7; the other dimensions keep box_classify, and are held to the same frames).  For N = 3..8 and
both fused formats, cameras chosen with tools/box_sets_census.py (the codes wave
restated in numpy) so that every kind of such a row occurs, which the test asserts before it renders anything:

    outline rows         |T| = 1: one face, and only hit or miss at it is open
    edge rows            |T| = 2
    a vertex in view     |T| >= 3
    sets not valid       origin on the plane of a face, origin inside the cube: these rows keep box_classify
    a camera whose `up` is far from orthogonal (no quadratic |dir|^2 in the lean loops: their rows come here too)

Every frame -- 72 whole 1920 x 1080 frames, the bench's launch shape, and one rank's bands of them -- is compared with the
oracle's frame of its camera byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fixtures as fx
import ntracer_amd
import oracle_binding as ob
import support as sup
from ntracer_amd import _lib, tracern
from ntracer_amd import distributed as ntd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import box_sets_census as census  # noqa: E402

W, H, FRAMES = 1920, 1080, 72
BAND = (3, 8, 8)            # rank, world, band_rows: 136 owned rows
FORMATS = (("rgbx8", fx.RGBX8, 4), ("rgbf32", fx.RGBF32, 12))


def looking_at_centre(n, origin, rng):
    """an orthonormal camera at `origin` whose forward axis points at the cube's centre"""
    o = np.asarray(origin, np.float32)
    q, _ = np.linalg.qr(np.column_stack([-o / np.linalg.norm(o)] + [rng.standard_normal(n) for _ in range(n - 1)]))
    q = q.T
    if np.dot(q[0], -o) < 0:
        q[0] = -q[0]
    axes = np.array([q[1], q[2], q[0]] + [q[k] for k in range(3, n)], np.float32)
    return o, np.ascontiguousarray(axes)


def cameras(n):
    """(name, origin, axes): fixtures.stress_cameras' skewed-`up` and up-less orientations and an origin inside the cube, an
    origin on the plane of a face and one on the face itself, both looking at the centre, and the three diagonal cameras of tests/test_box_tile_matrix.py"""
    rng = np.random.default_rng(5150 + n)
    stress = fx.stress_cameras(n, rng)
    cams = [("skew-up-1.7", ) + stress[56], ("skew-up-3.0", ) + stress[58], ("no-up", ) + stress[71], ("inside", ) + stress[0]]
    o = np.zeros(n, np.float32)
    o[:3] = (-1.0, 0.3, -4.5)
    cams.append(("on-a-face-plane", ) + looking_at_centre(n, o, rng))
    o = np.zeros(n, np.float32)
    o[:3] = (-1.0, 0.3, -0.25)                               # ... and on the face itself: the last entry is at tau = 0
    cams.append(("on-a-face", ) + looking_at_centre(n, o, rng))
    cams += [("diagonal-%d" % i, ) + fx.diagonal_camera(n, dist, rng) for i, dist in enumerate((2.5, 1.6 * np.sqrt(n), 1.2 * np.sqrt(n)))]
    return cams


def kinds(n, rows=None):
    """per camera: how many code-15 stretch-rows of each kind the codes wave finds in rows `rows` of the frame"""
    out = {}
    for name, o, a in cameras(n):
        code, sets = census.stretch_codes(o, a, W, H, rows=rows)
        is15 = code == 15
        ok = is15 & ((sets >> np.uint32(31)) != 0)
        t, _ = census.set_sizes(sets)
        out[name] = {"outline": int((ok & (t == 1)).sum()), "edge": int((ok & (t == 2)).sum()), "vertex": int((ok & (t >= 3)).sum()),
                     "not-valid": int((is15 & ~ok).sum())}
    return out


def check_kinds(n):
    k = kinds(n)
    for kind in ("outline", "edge", "vertex"):
        assert sum(c[kind] for c in k.values()) >= 10, (n, kind, k)
    # rows without valid sets where they are expected, and nowhere valid ones there: rays that start in the cube
    assert k["inside"]["not-valid"] > 0 and k["inside"]["outline"] + k["inside"]["edge"] + k["inside"]["vertex"] == 0, (n, k["inside"])
    assert k["on-a-face"]["not-valid"] > 0, (n, k["on-a-face"])
    assert k["on-a-face-plane"]["not-valid"] > 0, (n, k["on-a-face-plane"])
    skew = [k["skew-up-1.7"], k["skew-up-3.0"]]
    assert sum(c["outline"] + c["edge"] + c["vertex"] for c in skew) >= 10, (n, skew)
    # ... and the rank's bands have rows sorted on their sets too
    kb = kinds(n, rows=ntd.owned_rows(H, *BAND))
    assert sum(c["outline"] for c in kb.values()) > 0 and sum(c["edge"] for c in kb.values()) > 0, (n, kb)


@pytest.mark.parametrize("n", range(3, 9))
def test_cameras_show_every_kind_of_ray_by_ray_row(n):
    """(no GPU) what the GPU test below relies on"""
    check_kinds(n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(3, 9))
def test_rows_sorted_on_their_sets_equal_the_oracle(n):
    import torch
    check_kinds(n)
    cams = cameras(n)
    K = len(cams)
    sc = tracern.BoxScene(n)
    seq = [(2 * f) % K for f in range(FRAMES)]              # K = 9: neighbouring frames and frames 16 apart differ
    assert all(seq[i] != seq[i + 1] for i in range(FRAMES - 1)) and all(seq[i] != seq[i + 16] for i in range(FRAMES - 16))
    fo = np.ascontiguousarray(np.stack([cams[k][1] for k in seq]), np.float32)
    fa = np.ascontiguousarray(np.stack([cams[k][2] for k in seq]), np.float32)
    failures = []
    for name, chans, bpp in FORMATS:
        osc = ob.OracleScene(n, cams[0][1], cams[0][2])
        frames = []
        for _, o, a in cams:
            osc.set_camera(o, a)
            frames.append(osc.render(W, H, chans, threads=sup.worker_threads()))
        ref_all = torch.from_numpy(np.stack(frames)).cuda()             # (K, H, W * bpp)
        fmt = ntracer_amd.ImageFormat(W, H, [ntracer_amd.Channel(*c) for c in chans])
        assert fmt.pitch == W * bpp
        fst = fmt._as_struct()
        for label, band in (("whole", None), ("bands", BAND)):
            if band is None:
                rows, opts = np.arange(H), None
            else:
                rows = ntd.owned_rows(H, *band)
                opts = _lib.NtRenderOpts()
                opts.device, opts.band_rank, opts.band_world, opts.band_rows, opts.compact = -1, band[0], band[1], band[2], 1
            ref = ref_all if band is None else ref_all.index_select(1, torch.from_numpy(rows).cuda())
            frame_bytes = len(rows) * fmt.pitch
            dest = torch.full((FRAMES, frame_bytes), 0xA7, dtype=torch.uint8, device="cuda")
            _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(dest.data_ptr()), frame_bytes, FRAMES, fo.ctypes.data_as(_lib.f32p),
                                                          fa.ctypes.data_as(_lib.f32p), C.byref(fst), C.byref(opts) if opts is not None else None,
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            pix = dest.view(FRAMES, len(rows), fmt.pitch)
            for f in range(FRAMES):
                if torch.equal(pix[f], ref[seq[f]]):
                    continue
                g, r = pix[f].cpu().numpy(), ref[seq[f]].cpu().numpy()
                ys, xs = np.nonzero(g != r)
                failures.append("n=%d %s %s: frame %d (camera %s) differs from the oracle in %d bytes, first at x=%d y=%d"
                                % (n, name, label, f, cams[seq[f]][0], len(ys), xs[0] // bpp, rows[ys[0]]))
                if len(failures) > 12:
                    break
            del dest, pix
        del ref_all
    assert not failures, "\n".join(failures)
