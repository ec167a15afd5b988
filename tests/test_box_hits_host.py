"""BoxScene hit buffers (BoxScene.face_hits, nt_box_hits*) without a GPU: that the expectations of tests/box_hit_cases.py are the
oracle's own -- the colour each expected record stands for equals nto_colors_at bit for bit on every pixel of every case --,
that the cases are not vacuous, and what the ABI and the Python surface refuse before they touch a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import box_hit_cases as bc
import ntracer_amd
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, build, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", bc.DIMS)
def test_the_restated_rule_reproduces_the_oracles_colours_bit_for_bit(n):
    """no pixel left out, NaN colours included: the comparison is on the bit patterns"""
    for _, k, (w, h) in bc.views(n):
        e = bc.expected(n, k, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        want = bc.oracle_scene(n, k).colors_at(xs.ravel(), ys.ravel(), w, h).reshape(h, w, 3)
        assert np.array_equal(want.view(np.uint32), e["colors"].view(np.uint32)), bc.view_id((n, k, (w, h)))
        # the records are of one piece
        hit = e["item"] >= 0
        assert ((e["lane"] >= 0) == hit).all() and (e["dist"][~hit] == bc.FLT_MAX).all()
        assert (e["dist"][hit] > 0).all() and (e["dist"][hit] < bc.FLT_MAX).all() and (e["item"] < n).all()
        # the outward normal looks back along the ray
        d_face = np.take_along_axis(e["dirs"], np.where(hit, e["item"], 0)[..., None], axis=2)[..., 0]
        assert (np.where(e["lane"] > 0, d_face < 0, d_face > 0) | ~hit).all()


@pytest.mark.parametrize("n", bc.DIMS)
def test_the_cases_are_not_vacuous(n):
    es = {v: bc.expected(n, v[1], *v[2]) for v in bc.views(n)}
    assert any(len(e["faces"]) >= 3 and e["counts"]["silhouette"] >= 10 and e["counts"]["edge"] >= 5 for e in es.values())
    assert any((e["item"] >= 0).all() and e["item"].size > 1 for e in es.values())
    assert any((e["item"] < 0).all() and e["item"].size > 1 for e in es.values())
    # the camera the issue names for each: one face everywhere; nothing; three to seven faces with both kinds of pairs
    w, h = bc.SIZES[-1]
    assert len(bc.expected(n, 0, w, h)["faces"]) == 1 and (bc.expected(n, 0, w, h)["item"] >= 0).all()
    assert (bc.expected(n, 3, w, h)["item"] < 0).all()
    e = bc.expected(n, 2, w, h)
    assert len(e["faces"]) >= 3 and e["counts"]["silhouette"] >= 10 and e["counts"]["edge"] >= 5
    # both sides of the cube show somewhere (at n = 3 these cameras see the faces at -1 alone), the big view spans more than one
    # tile of the fused kernel both ways, and the diagonal camera stands outside the circumsphere
    assert {l for e in es.values() for _, l in e["faces"]} == ({0, 1} if n > 3 else {0})
    assert bc.BIG[0] > 64 and bc.BIG[1] > 32
    assert float(np.linalg.norm(bc.camera(n, 4)[0].astype(np.float64))) > np.sqrt(n)
    big = bc.expected(n, 4, *bc.BIG)
    assert (big["item"][:, 63] >= 0).any() and (big["item"][:, 64] >= 0).any() and (big["item"][31] >= 0).any() and (big["item"][32] >= 0).any()


def test_the_python_surface():
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.BoxScene.face_hits).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", -1), ("out", None), ("table", None),
                      ("first", 0), ("count", None), ("frame_stride", None)]
    assert [p.name for p in list(inspect.signature(tracern.FaceHits.normal).parameters.values())[1:3]] == ["x", "y"]
    assert ntracer_amd.FaceHits is tracern.FaceHits and "FaceHits" in ntracer_amd.__all__
    assert ntracer_amd.NTracer(5).FaceHits is tracern.FaceHits
    assert hasattr(ntracer_amd.NTracer(5).BoxScene, "face_hits")
    assert not hasattr(tracern.CompositeScene, "face_hits") and not hasattr(tracern.BoxScene, "primary_hits")
    # FaceHits on records made by hand: views of the buffer, the normal of a pixel
    recs = np.zeros((6, 4), np.int32)
    recs[:, 0] = np.array([1.5, 2.5, bc.FLT_MAX, 0.25, 1.0, 3.0], np.float32).view(np.int32)
    recs[:, 1] = [0, 2, -1, 4, 1, 1]
    recs[:, 2] = [1, 0, -1, 1, 0, 1]
    fh = tracern.FaceHits(5, 3, 2, None, 6, recs)
    assert fh.dist.shape == fh.axis.shape == fh.side.shape == fh.hit.shape == (2, 3) and fh.records is recs
    assert fh.dist.dtype == np.float32 and fh.dist[0, 1] == np.float32(2.5) and fh.hit.dtype == bool
    assert fh.hit.tolist() == [[True, True, False], [True, True, True]]
    assert list(fh.normal(0, 0)) == [1, 0, 0, 0, 0] and list(fh.normal(1, 0)) == [0, 0, -1, 0, 0] and fh.normal(2, 0) is None
    assert list(fh.normal(0, 1)) == [0, 0, 0, 0, 1] and isinstance(fh.normal(0, 1), tracern.Vector)
    # frames with a padded stride
    two = np.concatenate([recs, np.full((2, 4), 7, np.int32), recs[::-1], np.full((2, 4), 7, np.int32)])
    fh = tracern.FaceHits(5, 3, 2, 2, 8, two)
    assert fh.axis.shape == (2, 2, 3) and fh.axis[1, 0, 0] == 1 and list(fh.normal(0, 0, frame=1)) == [0, 1, 0, 0, 0]


def test_the_abi_validates_before_it_touches_a_device():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_box_hits", "nt_box_hits_device", "nt_box_hits_table_device"):
        assert hasattr(raw, name), name
    box = tracern.BoxScene(4)
    g, n, flat = rq.scene("cell600_n4")
    comp = tracern.CompositeScene.from_flat(n, flat)
    out = np.full((8 * 4, 4), 77, np.int32)
    host = lambda s, w, h, p: L.nt_box_hits(s, w, h, p, -1)
    devf = lambda s, w, h, p: L.nt_box_hits_device(s, w, h, p, None, None)
    for call in (host, devf):
        assert call(box._handle, 8, 4, None) == _lib.NT_E_INVALID
        assert call(None, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
            assert call(box._handle, w, h, out.ctypes.data) == _lib.NT_E_INVALID, (w, h)
            assert _lib.last_error()
        # beyond 2^31 - 1 records (nothing of the buffer is touched: the sizes are refused first)
        assert call(box._handle, 65536, 32768, out.ctypes.data) == _lib.NT_E_INVALID
        assert "2^31" in _lib.last_error()
        # a CompositeScene has primary hits of its own
        assert call(comp._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "not a box scene" in _lib.last_error()
        # a lens, the parallel projection
        box.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED and "lens" in _lib.last_error()
        box.set_lens(None)
        box.set_parallel_projection(2.0)
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED and "parallel" in _lib.last_error()
        box.set_parallel_projection(None)
    # the table form without a table (a table of another dimension or device, a bad first / count, a small stride:
    # test_box_hits_gpu.py -- a table lives on a device)
    assert L.nt_box_hits_table_device(box._handle, 8, 4, out.ctypes.data, 32, None, 0, 1, None, None) == _lib.NT_E_INVALID
    # the options of the _device forms: every field but device and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "strict_reference", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        assert L.nt_box_hits_device(box._handle, 8, 4, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID, field
        assert "every other field must be 0" in _lib.last_error()
    assert (out == 77).all()
    # the Python form refuses what does not fit before it calls the library
    with pytest.raises(ValueError):
        box.face_hits(0, 4)
    with pytest.raises(ValueError, match="frame_stride"):
        box.face_hits(8, 4, device="cuda", frame_stride=40)
    assert not box.locked


@pytest.mark.skipif(_lib.lib().nt_device_count() > 0, reason="checks the no-GPU behaviour")
def test_without_a_gpu_the_pass_fails_loudly():
    box = tracern.BoxScene(4)
    with pytest.raises(RuntimeError, match="no HIP device"):
        box.face_hits(8, 4)
    assert not box.locked


def test_the_composite_entry_points_still_refuse_a_box_scene():
    L = _lib.lib()
    box = tracern.BoxScene(4)
    black = (C.c_float * 3)(0, 0, 0)
    out = np.zeros(8 * 4 * 4, np.int32)
    res = _lib.NtHitBuffers()
    res.hits = out.ctypes.data
    assert L.nt_scene_set_outlines(box._handle, 1, 0.9, 0.02, black, 1.0) == _lib.NT_E_INVALID
    assert L.nt_scene_set_ambient_occlusion(box._handle, 0, None, 0.0, 0.0, 0.0) == _lib.NT_E_INVALID
    assert L.nt_primary_hits(box._handle, 8, 4, C.byref(res), -1) == _lib.NT_E_INVALID
    assert L.nt_primary_hits_device(box._handle, 8, 4, C.byref(res), None, None) == _lib.NT_E_INVALID
    assert L.nt_outline_mask(box._handle, 8, 4, out.ctypes.data, None, None) == _lib.NT_E_INVALID
    assert L.nt_depth_cue_factors(box._handle, 8, 4, out.ctypes.data, None) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_outlines()
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_depth_cue()


def test_the_unit_the_dispatch_and_the_header():
    # one unit a dimension, 3..24, with the guard of its siblings; no launcher named nt_<something>_fixed<N>
    units = [(name, flags) for name, src, flags in build.units() if src == "nt_inst_boxhits.hip"]
    assert sorted(int(f[0].split("=")[1]) for _, f in units) == list(range(3, 25))
    src = sup.source("nt_inst_boxhits.hip")
    assert "#ifndef NT_INST_N\n#error" in src and "nt_box_faces<NT_INST_N>" in src and "_fixed" not in src
    assert sup.source("nt_inst_box.hip") .count("nt_boxhits") == 0 and "nt_boxhits" not in sup.source("nt_box.hpp")
    var = sup.source("nt_var.hip")
    body = var[var.index("int nt_launch_box_faces("):]
    body = body[:body.index("\n}\n")]
    assert "nt_dispatch_dim<3, NT_DEV_MAX_FIXED_BOX>(li.force_var ? 0 : li.n" in body and "box_hits_var" in body and "box_lines_var" in body
    # no switch of its own, nothing of the shared pool's list
    for name in ("nt_boxhits.hpp", "nt_inst_boxhits.hip"):
        assert "getenv" not in sup.source(name) and "asm" not in sup.source(name), name
    # the header carries the rule
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    sec = header[header.index("BoxScene hit buffers and face lines"):]
    for phrase in ("in ascending order, skipping d_i == 0", "s = d_i < 0 ? 1.0f : -1.0f;  dist = (s - o_i) / d_i;",
                   "!(fabsf((d_j * dist) + o_j) > 1.0f + ROUNDING_FUZZ)", "dist >= FLT_MAX: no hit",
                   "lane = 1 for the face at +1 and 0 for the face at -1", "FLT_MAX, -1, -1, 0", "Every pixel's record is written",
                   "An origin inside the cube sees nothing", "not a box scene", "the supersampling factor is ignored"):
        assert phrase in sec, phrase
    for fn in ("nt_box_hits", "nt_box_hits_device", "nt_box_hits_table_device"):
        assert re.search(r"\bint %s\(" % fn, sec), fn
