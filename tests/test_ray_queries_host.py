"""Ray queries, the part that needs no GPU: the Python surface of the reference (RayIntersection, KDNode.intersects /
occludes with its parameter names, defaults and errors), the four ABI symbols and their validation -- which answers before
any device is touched -- and the kernel routes of nt_launch_query, pinned to the C++ that picks them the way
tests/test_composite_routes.py pins the render routes: every hipLaunchKernelGGL of nt_launch_query (nt_var.hip) and of the
fixed-n launcher it calls (launch_query_fixed, nt_query.hpp) has a row in QUERY_ROUTES, and every row names (scene, switches)
pairs that tests/test_ray_queries_gpu.py runs."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest

import ray_query_cases as rq
import support as sup
from ntracer_amd import Material, _lib, compat, tracern
from ntracer_amd.wrapper import NTracer


# kernel instantiation as its hipLaunchKernelGGL spells it (spaces dropped) -> cases of ray_query_cases.CASES that reach it, and
# through which query.  Lean: opaque, no Solids (cell600_n4: batches alone; simplex10_n10: loose triangles too).
QUERY_ROUTES = [
    ("query_closest<N,false>", [("cell600_n4", {}, "intersect"), ("cell600_n4", {"NTRACER_STRICT_REFERENCE": "1"}, "intersect"),
                                ("simplex7_n7", {}, "intersect")]),
    ("query_closest<N,true>", [("simplex10_n10", {}, "intersect")]),
    ("query_closest_t<N,true>", [("feature5_n5", {}, "intersect")]),
    ("query_closest_t<N,false>", [("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}, "intersect")]),
    ("query_occluded<N,false>", [("cell600_n4", {}, "occludes"), ("simplex7_n7", {}, "occludes")]),
    ("query_occluded<N,true>", [("simplex10_n10", {}, "occludes")]),
    ("query_occluded_t<N>", [("feature5_n5", {}, "occludes")]),
    ("query_closest_var", [("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}, "intersect")]),
    ("query_closest_var_t<true>", [("feature5_n5", {"NTRACER_FORCE_VAR": "1"}, "intersect"), ("feature11_n11", {}, "intersect"),
                                   ("lit12_n12", {}, "intersect"), ("feature16_n16", {}, "intersect")]),
    ("query_closest_var_t<false>", [("feature11_n11", {"NTRACER_CLEAN_NORMALS": "1"}, "intersect")]),
    ("query_occluded_var", [("simplex10_n10", {"NTRACER_FORCE_VAR": "1"}, "occludes"), ("lit12_n12", {}, "occludes")]),
    ("query_occluded_var_t", [("feature5_n5", {"NTRACER_FORCE_VAR": "1"}, "occludes"), ("feature11_n11", {}, "occludes"),
                              ("feature16_n16", {}, "occludes")]),
]


def _route(name, env, query):
    """the kernel a (scene, switches, query) lands on, by the rules of query_enqueue (nt_api.cpp) and the two launchers"""
    g, n, flat = rq.scene(name)
    opaque = bool((np.asarray(flat["materials"])[:, 6] >= 1).all())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    clean = env.get("NTRACER_CLEAN_NORMALS") == "1"
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    if query == "occludes":
        if var:
            return "query_occluded_var" if opaque else "query_occluded_var_t"
        return ("query_occluded<N,%s>" % ("true" if scalar else "false")) if opaque else "query_occluded_t<N>"
    if not opaque or (solids and not clean):
        alias = "false" if clean else "true"
        return "query_closest_var_t<%s>" % alias if var else "query_closest_t<N,%s>" % alias
    return "query_closest_var" if var else "query_closest<N,%s>" % ("true" if scalar else "false")


def test_every_query_launch_has_a_row_and_every_row_a_gpu_case():
    launched = sup.launches(sup.function_body(sup.source("nt_query.hpp"), "int launch_query_fixed(")) | sup.launches(sup.function_body(sup.source("nt_var.hip"), "int nt_launch_query("))
    assert len(launched) >= 12, sorted(launched)
    rows = [k for k, _ in QUERY_ROUTES]
    assert len(rows) == len(set(rows))
    assert set(rows) == launched, (sorted(launched - set(rows)), sorted(set(rows) - launched))
    cases = [(name, tuple(sorted(env.items()))) for name, env in rq.CASES]
    for kernel, ways in QUERY_ROUTES:
        assert ways, kernel
        for name, env, query in ways:
            assert (name, tuple(sorted(env.items()))) in cases, (kernel, name, env)      # the GPU test runs both queries of each case
            assert _route(name, env, query) == kernel, (kernel, name, env, query, _route(name, env, query))
    # the launches stay out of the render launchers, whose every launch wants a row of the render matrix
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite(")):
        assert not any(k.startswith("query_") for k in sup.launches(sup.function_body(sup.source(src), head)))
    # and route on the switches read_switches already reads: no getenv of their own
    assert "getenv" not in sup.source("nt_query.hpp") and "getenv" not in sup.function_body(sup.source("nt_var.hip"), "int nt_launch_query(")


def test_the_python_surface_is_the_references():
    params = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert params(tracern.KDNode.intersects) == [("origin", inspect.Parameter.empty), ("direction", inspect.Parameter.empty),
                                                 ("t_near", None), ("t_far", None), ("source", None), ("batch_index", -1)]
    assert params(tracern.KDNode.occludes) == [("origin", inspect.Parameter.empty), ("direction", inspect.Parameter.empty),
                                               ("distance", None), ("t_near", None), ("t_far", None), ("source", None), ("batch_index", -1)]
    assert issubclass(tracern.KDLeaf, tracern.KDNode) and issubclass(tracern.KDBranch, tracern.KDNode)
    assert NTracer(5).RayIntersection is tracern.RayIntersection
    names = compat.alias_reference_modules()
    try:
        assert "ntracer.tracern" in names
        for module in ("ntracer.tracern", "ntracer.tracer3", "ntracer.tracer8"):
            assert importlib.import_module(module).RayIntersection is tracern.RayIntersection
    finally:
        compat.remove_aliases()
    nt = NTracer(3)
    tri = nt.Triangle((1, -1, -1), (1, 0, 0), [(0, -0.25, 0), (0, 0, -0.25)], Material((1, 1, 1)))
    ri = tracern.RayIntersection(3.0, nt.Vector(1, 0, 0), nt.Vector(-1, 0, 0), tri)
    assert (ri.dist, ri.primitive, ri.batch_index) == (3.0, tri, -1)
    assert list(ri.origin) == [1, 0, 0] and list(ri.normal) == [-1, 0, 0]
    for attr in ("dist", "origin", "normal", "primitive", "batch_index"):
        with pytest.raises(AttributeError):
            setattr(ri, attr, 0)
    with pytest.raises(ValueError):
        tracern.RayIntersection(3.0, nt.Vector(1, 0, 0), nt.Vector(-1, 0, 0), tri, 2)
    with pytest.raises(TypeError):
        tracern.RayIntersection(3.0, nt.Vector(1, 0, 0), nt.Vector(-1, 0, 0), None)


def test_the_errors_are_the_references():
    nt = NTracer(3)
    tri = nt.Triangle((1, -1, -1), (1, 0, 0), [(0, -0.25, 0), (0, 0, -0.25)], Material((1, 1, 1)))
    leaf = nt.KDLeaf([tri])
    for call in (leaf.intersects, leaf.occludes):
        with pytest.raises(TypeError, match='"source" must be an instance of Primitive or PrimitiveBatch'):
            call((0, 0, 0), (1, 0, 0), source=3)
        with pytest.raises(TypeError, match='"origin" and "direction" must have the same dimension'):
            call((0, 0, 0), (1, 0, 0, 0))
        with pytest.raises(TypeError):
            call((0, 0, 0, 0), (1, 0, 0, 0))                 # a ray of another dimension than the node


def _args(count=2, n=4, **kw):
    o = np.zeros((max(count, 1), n), np.float32)
    hits = np.zeros((max(count, 1), 4), np.int32)
    rays = _lib.NtRayBatch()
    rays.count, rays.origins, rays.directions = count, o.ctypes.data, o.ctypes.data
    res = _lib.NtRayResults()
    res.hits = hits.ctypes.data
    for k, v in kw.items():
        setattr(rays if hasattr(rays, k) else res, k, v)
    return rays, res, (o, hits)


def test_the_abi_validates_before_it_touches_a_device():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_intersect_rays", "nt_occludes_rays", "nt_intersect_rays_device", "nt_occludes_rays_device"):
        assert hasattr(raw, name), name
    assert C.sizeof(_lib.NtRayHit) == 16
    g, n, flat = rq.scene("cell600_n4")
    sc = tracern.CompositeScene.from_flat(n, flat)
    host = [lambda r, o, f=f: f(sc._handle, r, o, -1) for f in (L.nt_intersect_rays, L.nt_occludes_rays)]
    devf = [lambda r, o, f=f: f(sc._handle, r, o, None, None) for f in (L.nt_intersect_rays_device, L.nt_occludes_rays_device)]
    scratch = np.zeros(64, np.int32)
    for call in host + devf:
        rays, res, keep = _args()
        assert call(None, C.byref(res)) == _lib.NT_E_INVALID
        assert call(C.byref(rays), None) == _lib.NT_E_INVALID
        for bad in (dict(hits=None), dict(origins=None), dict(directions=None), dict(count=-1), dict(max_transparent=-1),
                    dict(max_transparent=25), dict(transparent=scratch.ctypes.data, max_transparent=0)):
            rays, res, keep = _args(**bad)
            assert call(C.byref(rays), C.byref(res)) == _lib.NT_E_INVALID, bad
            assert _lib.last_error()
        rays, res, keep = _args(count=0)
        assert call(C.byref(rays), C.byref(res)) == _lib.NT_OK           # nothing to do: no device is asked for
    # a BoxScene has no tree
    box = tracern.BoxScene(4)
    rays, res, keep = _args()
    for f in (L.nt_intersect_rays, L.nt_occludes_rays):
        assert f(box._handle, C.byref(rays), C.byref(res), -1) == _lib.NT_E_INVALID
        assert "not a composite scene" in _lib.last_error()
    # the options of the _device forms: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        rays, res, keep = _args()
        assert L.nt_intersect_rays_device(sc._handle, C.byref(rays), C.byref(res), C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the batched Python forms refuse what does not fit before they call the library
    with pytest.raises(ValueError):
        sc.intersect_rays(np.zeros((3, 5), np.float32), np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError):
        sc.intersect_rays(np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32), max_transparent=25)
    empty = sc.intersect_rays(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))
    assert all(len(v) == 0 for v in empty.values())
