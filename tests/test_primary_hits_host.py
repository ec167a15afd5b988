"""Primary-hit buffers, the part that needs no GPU: the fp32 restatement of aabb_distance that the expected records rest on
(tests/primary_hit_cases.py) is pinned to the oracle's own counters; the three ABI symbols refuse what can be refused before
any device is touched; the Python signature; and the kernel routes, pinned to the C++ that picks them the way
tests/test_ray_queries_host.py pins the query routes: every hipLaunchKernelGGL of launch_hits_fixed (nt_hits.hpp) and of
nt_launch_hits (nt_var.hip) has a row in HITS_ROUTES, and every row names (scene, switches) cases that
tests/test_primary_hits_gpu.py runs."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import primary_hit_cases as ph
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern


PACKET_LEAN = [("cell600_n4", {}), ("cell600_n4", {"NTRACER_STRICT_REFERENCE": "1"}), ("simplex7_n7", {})]
PACKET_SCAL = [("simplex10_n10", {})]
# kernel instantiation as its hipLaunchKernelGGL spells it (spaces dropped) -> cases of primary_hit_cases.CASES that launch it
HITS_ROUTES = [
    ("composite_packet<N,32,false,false,true>", PACKET_LEAN),
    ("composite_packet<N,32,false,true,true>", PACKET_SCAL),
    ("packet_numerators<N>", PACKET_LEAN + PACKET_SCAL),
    ("hits_normals<N,false>", PACKET_LEAN),
    ("hits_normals<N,true>", PACKET_SCAL),
    ("hits_closest<N,false>", [("cell600_n4", {"NTRACER_COMPOSITE_KERNEL": "2"})]),
    ("hits_closest<N,true>", [("simplex10_n10", {"NTRACER_COMPOSITE_KERNEL": "2"})]),
    ("hits_closest_t<N,true>", [("feature5_n5", {})]),
    ("hits_closest_t<N,false>", [("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"})]),
    ("hits_closest_var", [("simplex10_n10", {"NTRACER_FORCE_VAR": "1"})]),
    ("hits_closest_var_t<true>", [("feature5_n5", {"NTRACER_FORCE_VAR": "1"}), ("feature11_n11", {}), ("lit12_n12", {}), ("feature16_n16", {})]),
    ("hits_closest_var_t<false>", [("feature11_n11", {"NTRACER_CLEAN_NORMALS": "1"})]),
]


def _depth(flat):
    """levels of the k-d tree"""
    best, stack = 0, [(int(flat["root"]), 1)] if int(flat["root"]) >= 0 else []
    while stack:
        node, d = stack.pop()
        best = max(best, d)
        if flat["node_axis"][node] >= 0:
            stack += [(int(c), d + 1) for c in (flat["node_left"][node], flat["node_right"][node]) if c >= 0]
    return best


def _routes(name, env):
    """the kernels a (scene, switches) pass launches when normals are asked for, by the rules of hits_enqueue (nt_api.cpp) and
    the two launchers"""
    g, n, flat = rq.scene(name)
    opaque = bool((np.asarray(flat["materials"])[:, 6] >= 1).all())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    sc = "true" if scalar else "false"
    if not opaque or (solids and not clean):
        alias = "false" if clean else "true"
        return {"hits_closest_var_t<%s>" % alias if var else "hits_closest_t<N,%s>" % alias}
    if var:
        return {"hits_closest_var"}
    if env.get("NTRACER_COMPOSITE_KERNEL", "0") == "0" and max(_depth(flat) + 1, 2) <= 32:
        return {"composite_packet<N,32,false,%s,true>" % sc, "hits_normals<N,%s>" % sc} | ({"packet_numerators<N>"} if len(flat["batch_recs"]) else set())
    return {"hits_closest<N,%s>" % sc}


def test_every_hits_launch_has_a_row_and_every_row_a_gpu_case():
    launched = sup.launches_through(sup.source("nt_hits.hpp"), "int launch_hits_fixed(") | sup.launches(sup.function_body(sup.source("nt_var.hip"), "int nt_launch_hits("))
    rows = [k for k, _ in HITS_ROUTES]
    assert len(rows) == len(set(rows)) == 12
    assert set(rows) == launched, (sorted(launched - set(rows)), sorted(set(rows) - launched))
    cases = [(name, tuple(sorted(env.items()))) for name, env in ph.CASES]
    for kernel, ways in HITS_ROUTES:
        assert ways, kernel
        for name, env in ways:
            assert (name, tuple(sorted(env.items()))) in cases, (kernel, name, env)
            assert kernel in _routes(name, env), (kernel, name, env, _routes(name, env))
    # every case lands on rows of the table
    for name, env in ph.CASES:
        assert _routes(name, env) <= set(rows), (name, env)
    # the launches stay out of the render and query launchers, whose every launch wants a row of their own matrices
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_query.hpp", "int launch_query_fixed("), ("nt_var.hip", "int nt_launch_query(")):
        names = sup.launches(sup.function_body(sup.source(src), head))
        assert not any(k.startswith("hits_") or re.match(r"composite_packet<N,32,\w+,\w+,true>", k) for k in names), (head, names)
    # and route on the switches read_switches already reads: no getenv of their own
    assert "getenv" not in sup.source("nt_hits.hpp") and "getenv" not in sup.function_body(sup.source("nt_var.hip"), "int nt_launch_hits(")


@pytest.mark.parametrize("size", [(37, 21), (64, 48)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ph.COUNTED)
def test_the_expected_records_agree_with_the_oracles_counters(name, size):
    """pixels with t0 >= 0 and pixels with an opaque hit, counted from the expected records, against aabb_enter and hits of
    nto_colors_at on the same pixels: ray_color's own decisions"""
    w, h = size
    g, n, flat = rq.scene(name)
    e = ph.expected((name, {}), w, h)
    o, axes = ph.camera(name)
    sc = ob.OracleScene(n, o, axes, ph.fov_of(name), flat=flat, params=fx.params_of(g))
    ys, xs = np.mgrid[0:h, 0:w]
    _, c = sc.colors_at(xs.ravel(), ys.ravel(), w, h, counters=True)
    enter, hit = int((e["t0"] >= 0).sum()), int((e["item"] >= 0).sum())
    assert (enter, hit) == (c["aabb_enter"], c["hits"]), (name, size, enter, hit, c)
    assert (e["item"][e["t0"] < 0] == -1).all() and not e["n_transparent"][e["t0"] < 0].any()
    # both sides of both decisions are there (every ray of the two large feature scenes enters the box)
    assert 0 < hit < enter
    assert (enter < w * h) == (name not in ("feature11_n11", "feature16_n16")), (name, enter)
    if (name, size) == ("cell600_n4", (64, 48)):
        assert (enter, hit) == (2397, 1059)
    if (name, size) == ("simplex10_n10", (37, 21)):
        assert (enter, hit) == (320, 16)


def test_the_python_signature():
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.primary_hits).parameters.values())[1:]]
    assert params[:4] == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("normals", False), ("device", -1)]
    assert all(d is not inspect.Parameter.empty for _, d in params[4:])            # whatever follows is optional
    assert {"table", "first", "count", "frame_stride"} <= {k for k, _ in params}
    assert [p.name for p in list(inspect.signature(tracern.PrimaryHits.intersection).parameters.values())[1:3]] == ["x", "y"]
    assert not hasattr(tracern.BoxScene, "primary_hits")


def _bufs(width=8, height=4, n=4, **kw):
    hits = np.zeros((width * height, 4), np.int32)
    res = _lib.NtHitBuffers()
    res.hits = hits.ctypes.data
    for k, v in kw.items():
        setattr(res, k, v)
    return res, hits


def test_the_abi_validates_before_it_touches_a_device():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_primary_hits", "nt_primary_hits_device", "nt_primary_hits_table_device"):
        assert hasattr(raw, name), name
    g, n, flat = rq.scene("cell600_n4")
    sc = tracern.CompositeScene.from_flat(n, flat)
    box = tracern.BoxScene(4)
    host = lambda s, w, h, out: L.nt_primary_hits(s, w, h, out, -1)
    devf = lambda s, w, h, out: L.nt_primary_hits_device(s, w, h, out, None, None)
    for call in (host, devf):
        res, keep = _bufs()
        assert call(sc._handle, 8, 4, None) == _lib.NT_E_INVALID
        assert call(None, 8, 4, C.byref(res)) == _lib.NT_E_INVALID
        for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
            assert call(sc._handle, w, h, C.byref(res)) == _lib.NT_E_INVALID, (w, h)
            assert _lib.last_error()
        res, keep = _bufs(hits=None)
        assert call(sc._handle, 8, 4, C.byref(res)) == _lib.NT_E_INVALID
        # beyond 2^31 - 1 records (nothing of the buffer is touched: the sizes are refused first)
        res, keep = _bufs()
        assert call(sc._handle, 65536, 32768, C.byref(res)) == _lib.NT_E_INVALID
        assert "2^31" in _lib.last_error()
        # a BoxScene has no tree
        assert call(box._handle, 8, 4, C.byref(res)) == _lib.NT_E_INVALID
        assert "not a composite scene" in _lib.last_error()
    # the table form without a table (a table of another dimension, a bad first / count: test_primary_hits_gpu.py -- a table
    # lives on a device)
    res, keep = _bufs()
    assert L.nt_primary_hits_table_device(sc._handle, 8, 4, C.byref(res), 32, None, 0, 1, None, None) == _lib.NT_E_INVALID
    # the options of the _device forms: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        res, keep = _bufs()
        assert L.nt_primary_hits_device(sc._handle, 8, 4, C.byref(res), C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the Python form refuses what does not fit before it calls the library
    with pytest.raises(ValueError):
        sc.primary_hits(0, 4)
