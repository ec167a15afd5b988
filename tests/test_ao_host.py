"""Ambient occlusion, the part that needs no GPU: the conditions that keep tests/test_ao_gpu.py from being vacuous, asserted on
the oracle's counts (tests/ao_cases.py); every answer the ABI gives before a device is touched; the setting's round trip;
sphere_directions; the Python signatures; and the kernel routes, pinned to the C++ that picks them the way
tests/test_primary_hits_host.py pins HITS_ROUTES: every hipLaunchKernelGGL of launch_ao_fixed (nt_ao.hpp) and of nt_launch_ao,
nt_launch_ao_expand, nt_launch_ao_reduce and nt_launch_ao_apply (nt_var.hip) has a row in AO_ROUTES, and every row names
(scene, switches) cases that tests/test_ao_gpu.py runs."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ao_cases as ao
import ntracer_amd
import ray_query_cases as rq
import support as sup
from ntracer_amd import _lib, tracern


FAST = [("cell120_n4", {}), ("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}), ("cell120_n4", {"NTRACER_COMPOSITE_KERNEL": "2"}),
        ("orthoplex5_n5", {})]
RAYS = [("cell120_n4", {"NTRACER_FORCE_VAR": "1"}), ("feature5_n5", {}), ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"}),
        ("feature5_n5", {"NTRACER_FORCE_VAR": "1"}), ("feature16_n16", {})]
# kernel instantiation as its hipLaunchKernelGGL spells it (spaces dropped) -> cases of ao_cases.CASES that launch it; ao_apply is
# launched by every render with the setting on (test_ao_gpu.py renders these two)
AO_ROUTES = [
    ("ao_kernel<N,false>", FAST),
    ("ao_kernel<N,true>", [("simplex10_n10", {})]),
    ("ao_expand", RAYS),
    ("ao_reduce", RAYS),
    ("ao_apply", [("cell120_n4", {}), ("feature5_n5", {})]),
]


def _routes(name, env):
    """the counting kernels a (scene, switches) case launches, by the rule of enqueue_ao (nt_api.cpp) and launch_ao_fixed"""
    g, n, flat = rq.scene(name)
    opaque = bool((np.asarray(flat["materials"])[:, 6] >= 1).all())
    solids, scalar = len(flat["solid_types"]) > 0, len(flat["solid_types"]) + len(flat["tri_recs"]) > 0
    var = n > 10 or env.get("NTRACER_FORCE_VAR") == "1"
    faithful = not opaque or (solids and env.get("NTRACER_CLEAN_NORMALS") != "1")
    if faithful or var:
        return {"ao_expand", "ao_reduce"}
    return {"ao_kernel<N,%s>" % ("true" if scalar else "false")}


def test_every_ao_launch_has_a_row_and_every_row_a_gpu_case():
    var = sup.source("nt_var.hip")
    launched = sup.launches(sup.function_body(sup.source("nt_ao.hpp"), "int launch_ao_fixed("))
    for head in ("int nt_launch_ao(", "int nt_launch_ao_expand(", "int nt_launch_ao_reduce(", "int nt_launch_ao_apply("):
        launched |= sup.launches(sup.function_body(var, head))
    rows = [k for k, _ in AO_ROUTES]
    assert len(rows) == len(set(rows)) == 5
    assert set(rows) == launched, (sorted(launched - set(rows)), sorted(set(rows) - launched))
    cases = [(name, tuple(sorted(env.items()))) for name, env in ao.CASES]
    for kernel, ways in AO_ROUTES:
        assert ways, kernel
        for name, env in ways:
            assert (name, tuple(sorted(env.items()))) in cases, (kernel, name, env)
            if kernel != "ao_apply":
                assert kernel in _routes(name, env), (kernel, name, env, _routes(name, env))
    # every case lands on rows of the table, and both routes have cases
    for name, env in ao.CASES:
        assert _routes(name, env) <= set(rows), (name, env)
    # the rule above is enqueue_ao's own: the terms are composite_route's, which it asks, keeping none of its own
    rule, api = sup.function_body(sup.source("nt_api.cpp"), "CompositeRoute composite_route("), sup.function_body(sup.source("nt_api.cpp"), "int enqueue_ao(")
    assert "r.var = s->n > NT_MAX_FIXED_DIM || sw.force_var;" in rule
    assert "r.faithful = !s->all_opaque || (s->n_solids > 0 && !sw.clean_normals);" in rule
    assert "const CompositeRoute rt = composite_route(s, sw);" in api and "all_opaque" not in api
    assert "const bool fast = !rt.faithful && !rt.var;" in api
    # the new launches stay out of the render, query and hits launchers, whose every launch wants a row of their own matrices
    for src, head in (("nt_composite.hpp", "int launch_composite_fixed("), ("nt_var.hip", "int nt_launch_composite("),
                      ("nt_query.hpp", "int launch_query_fixed("), ("nt_var.hip", "int nt_launch_query("),
                      ("nt_hits.hpp", "int launch_hits_fixed("), ("nt_var.hip", "int nt_launch_hits(")):
        assert not any(k.startswith("ao_") for k in sup.launches(sup.function_body(sup.source(src), head))), head
    # and route on the switches read_switches already reads: no getenv of their own
    assert "getenv" not in sup.source("nt_ao.hpp") and "getenv" not in sup.source("nt_inst_ao.hip")


# ------------------------------------------------------------------ the conditions that keep the GPU tests from being vacuous
def test_the_oracles_counts_are_not_vacuous():
    w, h = 37, 21
    e = ao.expected(("cell120_n4", {}), w, h)
    b = e["blocked"]
    hits = int(e["hit"].sum())
    print("cell120_n4: hit %d, blocked > 0 on %d, 0 < blocked < 8 on %d" % (hits, int((b > 0).sum()), int(((b > 0) & (b < 8)).sum())))
    assert (b[~e["hit"]] == -1).all() and (b[e["hit"]] >= 0).all()
    assert 2 * int((b > 0).sum()) >= hits > 0
    assert (hits, int((b > 0).sum()), int(((b > 0) & (b < 8)).sum())) == (270, 206, 200)
    assert np.bincount(b[b >= 0], minlength=9).tolist() == [64, 48, 37, 32, 33, 28, 13, 9, 6]
    for case in (("feature5_n5", {}), ("feature5_n5", {"NTRACER_CLEAN_NORMALS": "1"})):
        f = ao.expected(case, w, h)
        fb = f["blocked"]
        assert 3 * int((fb > 0).sum()) >= int(f["hit"].sum()) > 0, case
        assert (int(f["hit"].sum()), int((fb > 0).sum())) == (132, 58 if case[1] else 57)
        assert ((fb > 0) == ((fb > 0) & (fb < 8))).all()
    f = ao.expected(("feature16_n16", {}), w, h)
    assert int((f["blocked"] > 0).sum()) >= 10 and (int(f["hit"].sum()), int((f["blocked"] > 0).sum())) == (95, 15)
    # the convex control: nothing blocks with the bias, and the neighbouring facets do without it
    o = ao.expected(("orthoplex5_n5", {}), w, h)
    assert int(o["hit"].sum()) == 160 and not (o["blocked"] > 0).any()
    o0 = ao.expected(("orthoplex5_n5", {}), w, h, bias=0.0)
    assert int((o0["blocked"] > 0).sum()) == 112
    # the small views
    s = ao.expected(("cell120_n4", {"NTRACER_STRICT_REFERENCE": "1"}), 9, 7)
    assert (int(s["hit"].sum()), int((s["blocked"] > 0).sum())) == (14, 12)
    s = ao.expected(("cell120_n4", {}), 8, 8)
    assert (int(s["hit"].sum()), int((s["blocked"] > 0).sum())) == (11, 10)


@pytest.mark.parametrize("case", ao.CASES, ids=ao.case_id)
def test_no_blocking_hit_lies_at_the_radius(case):
    """dist <= radius is never decided by a last bit: no sample's hit lies within 1e-4 * radius of the radius"""
    for w, h in ao.sizes(case):
        e = ao.expected(case, w, h)
        d = e["dist"][e["item"] >= 0].astype(np.float64)
        assert not (np.abs(d - ao.RADIUS) <= 1e-4 * ao.RADIUS).any(), (case, w, h)
        # t_far = radius: the walk hands out nothing from beyond it either way
        assert ((e["item"] >= 0) & (e["dist"] <= np.float32(ao.RADIUS))).sum(axis=2)[e["hit"]].tolist() == e["blocked"][e["hit"]].tolist()


# ------------------------------------------------------------------ sphere_directions, signatures
def test_sphere_directions_is_deterministic_and_its_rows_have_unit_length():
    for n, k in ((3, 1), (4, 8), (16, 256)):
        t = ntracer_amd.sphere_directions(n, k)
        assert t.dtype == np.float32 and t.shape == (k, n) and t.flags["C_CONTIGUOUS"]
        assert np.array_equal(t, ntracer_amd.sphere_directions(n, k, seed=0))
        assert np.abs(np.sqrt((t.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 1e-6
        v = np.random.default_rng(0).standard_normal((k, n))
        assert np.array_equal(t, (v / np.sqrt((v * v).sum(axis=1))[:, None]).astype(np.float32))
    assert not np.array_equal(ntracer_amd.sphere_directions(4, 8, seed=1), ntracer_amd.sphere_directions(4, 8))
    assert ntracer_amd.sphere_directions is tracern.sphere_directions and "sphere_directions" in ntracer_amd.__all__


def test_the_python_signatures():
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.set_ambient_occlusion).parameters.values())[1:]]
    assert params == [("samples", inspect.Parameter.empty), ("radius", None), ("bias", None), ("strength", 1.0)]
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.occlusion_counts).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("device", None), ("strict_reference", None)]
    assert isinstance(inspect.getattr_static(tracern.CompositeScene, "ambient_occlusion"), property)
    params = [(p.name, p.default) for p in inspect.signature(ntracer_amd.sphere_directions).parameters.values()]
    assert params == [("n", inspect.Parameter.empty), ("count", inspect.Parameter.empty), ("seed", 0)]


# ------------------------------------------------------------------ the setting
def _scene(name="cell120_n4"):
    g, n, flat = rq.scene(name)
    return tracern.CompositeScene.from_flat(n, flat), n


def _same(a, b):
    return (a is None and b is None) or (a["count"] == b["count"] and np.array_equal(a["directions"].view(np.uint32), b["directions"].view(np.uint32))
                                         and (a["radius"], a["bias"], a["strength"]) == (b["radius"], b["bias"], b["strength"]))


def test_the_setting_round_trips_and_a_refused_set_leaves_it_as_it_was():
    L = _lib.lib()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_scene_set_ambient_occlusion", "nt_scene_get_ambient_occlusion", "nt_ambient_occlusion", "nt_ambient_occlusion_device"):
        assert hasattr(raw, name), name
    sc, n = _scene()
    assert sc.ambient_occlusion is None
    # a table with awkward bits: denormals, negative zero beside a non-zero component, large and tiny values
    t = np.array([[1e-42, -0.0, 3.0, -2.5], [0.0, 0.0, 0.0, -1e-30], [1e30, 1.0, -1.0, 7.0]], np.float32)
    sc.set_ambient_occlusion(t, 0.75, bias=0.125, strength=0.3)
    a = sc.ambient_occlusion
    assert a["count"] == 3 and a["directions"].dtype == np.float32 and a["directions"].shape == (3, n)
    assert np.array_equal(a["directions"].view(np.uint32), t.view(np.uint32))
    assert (a["radius"], a["bias"], a["strength"]) == (0.75, 0.125, float(np.float32(0.3)))
    # the ABI's getter through whichever pointers are given
    count, radius = C.c_int(-1), C.c_float(-1)
    assert L.nt_scene_get_ambient_occlusion(sc._handle, C.byref(count), None, C.byref(radius), None, None) == 0
    assert (count.value, radius.value) == (3, 0.75)
    assert L.nt_scene_get_ambient_occlusion(None, C.byref(count), None, None, None, None) == _lib.NT_E_INVALID
    # an int: sphere_directions(n, K); bias None: 1e-3 * radius
    sc.set_ambient_occlusion(8, 2.0)
    a = sc.ambient_occlusion
    assert np.array_equal(a["directions"], ntracer_amd.sphere_directions(n, 8)) and a["radius"] == 2.0 and a["strength"] == 1.0
    assert a["bias"] == float(np.float32(2e-3))
    # every refusal leaves it as it was
    keep = sc.ambient_occlusion
    good = ntracer_amd.sphere_directions(n, 4)
    ptr = lambda arr: arr.ctypes.data_as(_lib.f32p)
    bad_rows = []
    for v in (np.nan, np.inf, -np.inf):
        r = good.copy()
        r[2, 1] = v
        bad_rows.append(r)
    r = good.copy()
    r[3] = 0.0
    r[3, 0] = -0.0
    bad_rows.append(r)
    refused = [(-1, good, 1.0, 0.0, 1.0), (257, np.zeros((257, n), np.float32) + 1, 1.0, 0.0, 1.0), (4, None, 1.0, 0.0, 1.0)]
    refused += [(4, r, 1.0, 0.0, 1.0) for r in bad_rows]
    refused += [(4, good, v, 0.0, 1.0) for v in (0.0, -1.0, np.nan, np.inf)]
    refused += [(4, good, 1.0, v, 1.0) for v in (-1e-9, np.nan, np.inf)]
    refused += [(4, good, 1.0, 0.0, v) for v in (-0.001, 1.001, np.nan)]
    for count, table, radius, bias, strength in refused:
        status = L.nt_scene_set_ambient_occlusion(sc._handle, count, None if table is None else ptr(table), radius, bias, strength)
        assert status == _lib.NT_E_INVALID, (count, radius, bias, strength)
        assert _lib.last_error()
        assert _same(sc.ambient_occlusion, keep)
    assert L.nt_scene_set_ambient_occlusion(None, 4, ptr(good), 1.0, 0.0, 1.0) == _lib.NT_E_INVALID
    for bad in (dict(samples=True, radius=1.0), dict(samples=8), dict(samples=-2, radius=1.0), dict(samples=np.zeros((2, n + 1)), radius=1.0),
                dict(samples=8, radius="1"), dict(samples=300, radius=1.0)):
        with pytest.raises(ValueError):
            sc.set_ambient_occlusion(**bad)
        assert _same(sc.ambient_occlusion, keep)
    # the limits are in: K = 1 and K = 256, bias 0, strength 0 and 1
    sc.set_ambient_occlusion(1, 1e-20, bias=0.0, strength=0.0)
    assert sc.ambient_occlusion["count"] == 1 and sc.ambient_occlusion["bias"] == 0.0
    sc.set_ambient_occlusion(256, 1e20)
    assert sc.ambient_occlusion["count"] == 256
    # locked while a render holds the scene, as nt_scene_set_camera
    assert L.nt_scene_lock(sc._handle) == 0
    keep = sc.ambient_occlusion
    assert L.nt_scene_set_ambient_occlusion(sc._handle, 4, ptr(good), 1.0, 0.0, 1.0) == _lib.NT_E_LOCKED
    assert L.nt_scene_set_ambient_occlusion(sc._handle, 0, None, 0.0, 0.0, 0.0) == _lib.NT_E_LOCKED
    with pytest.raises(_lib.LockedError):
        sc.set_ambient_occlusion(4, 1.0)
    assert _same(sc.ambient_occlusion, keep)
    assert L.nt_scene_unlock(sc._handle) == 0
    # off: None or 0, whatever else is passed
    sc.set_ambient_occlusion(0)
    assert sc.ambient_occlusion is None
    sc.set_ambient_occlusion(4, 1.0)
    sc.set_ambient_occlusion(None)
    assert sc.ambient_occlusion is None
    # a BoxScene has no tree
    box = tracern.BoxScene(4)
    assert L.nt_scene_set_ambient_occlusion(box._handle, 4, ptr(good), 1.0, 0.0, 1.0) == _lib.NT_E_INVALID
    assert L.nt_scene_set_ambient_occlusion(box._handle, 0, None, 0.0, 0.0, 0.0) == _lib.NT_E_INVALID
    with pytest.raises(ValueError, match="BoxScene"):
        box.set_ambient_occlusion(4, 1.0)
    assert box.ambient_occlusion is None


def test_the_buffer_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    sc, n = _scene()
    box = tracern.BoxScene(4)
    out = np.full(8 * 4, 77, np.int32)
    host = lambda s, w, h, p: L.nt_ambient_occlusion(s, w, h, p, None)
    devf = lambda s, w, h, p: L.nt_ambient_occlusion_device(s, w, h, p, None, None)
    for call in (host, devf):
        # the setting is off
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "off" in _lib.last_error()
        sc.set_ambient_occlusion(8, 1.0)
        assert call(None, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert call(sc._handle, 8, 4, None) == _lib.NT_E_INVALID
        for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
            assert call(sc._handle, w, h, out.ctypes.data) == _lib.NT_E_INVALID, (w, h)
        assert call(box._handle, 8, 4, out.ctypes.data) == _lib.NT_E_INVALID
        assert "not a composite scene" in _lib.last_error()
        # the primary-hit pass is refused under a lens and under the parallel projection
        sc.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        sc.set_lens(None)
        sc.set_parallel_projection(2.0)
        assert call(sc._handle, 8, 4, out.ctypes.data) == _lib.NT_E_UNSUPPORTED
        sc.set_parallel_projection(None)
        sc.set_ambient_occlusion(None)
    assert (out == 77).all()
    sc.set_ambient_occlusion(8, 1.0)
    # the options of the _device form: every field but device, strict_reference and abort_device must be 0
    for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
        opts = _lib.NtRenderOpts()
        opts.device = -1
        setattr(opts, field, 1)
        assert L.nt_ambient_occlusion_device(sc._handle, 8, 4, out.ctypes.data, C.byref(opts), None) == _lib.NT_E_INVALID, field
    # the Python forms
    with pytest.raises(ValueError):
        sc.occlusion_counts(0, 4)
    with pytest.raises(ValueError, match="not a composite scene"):
        box.occlusion_counts(8, 4)
    sc.set_ambient_occlusion(None)
    with pytest.raises(ValueError, match="off"):
        sc.occlusion_counts(8, 4)


def test_the_renders_refuse_what_the_setting_excludes_before_they_touch_a_device():
    """nt_render, nt_render_device, nt_render_frames_device and a camera table's render: NT_E_UNSUPPORTED with a message that
    starts "ambient occlusion", the destination as it was (the table form needs a device to make its table: test_ao_gpu.py)"""
    L = _lib.lib()
    sc, n = _scene()
    sc.set_ambient_occlusion(8, 1.0)
    w, h = 8, 4
    fmt = sup.fmt_of(w, h)
    fst = fmt._as_struct()
    size = fmt.pitch * h
    dest = (C.c_char * size)(*([0x4E] * size))
    origins, axes = np.zeros((1, n), np.float32), np.eye(n, dtype=np.float32)[None].copy()

    def forms(opts):
        po = None if opts is None else C.byref(opts)
        return [L.nt_render(sc._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_device(sc._handle, dest, size, C.byref(fst), po, None),
                L.nt_render_frames_device(sc._handle, dest, size, 1, origins.ctypes.data_as(_lib.f32p), axes.ctypes.data_as(_lib.f32p),
                                          C.byref(fst), po, None)]

    def refused(opts, word):
        for status in forms(opts):
            assert status == _lib.NT_E_UNSUPPORTED, (word, status, _lib.last_error())
            assert _lib.last_error().startswith("ambient occlusion") and word in _lib.last_error(), _lib.last_error()
        assert bytes(dest) == b"\x4e" * size

    # a supersampling factor, adaptive or not
    sc.set_supersampling(2)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(0.1)
    refused(None, "supersampling")
    sc.set_adaptive_supersampling(None)
    sc.set_supersampling(1)
    # bands
    opts = _lib.NtRenderOpts()
    opts.device, opts.band_world = -1, 2
    refused(opts, "band")
    # statistics
    opts = _lib.NtRenderOpts()
    opts.device, opts.collect_stats = -1, 1
    refused(opts, "collect_stats")
    # a lens, the parallel projection
    sc.set_lens(tracern.Lens.pinhole(w, h, 0.8))
    refused(None, "lens")
    sc.set_lens(None)
    sc.set_parallel_projection(2.0)
    refused(None, "parallel")
    sc.set_parallel_projection(None)
    with pytest.raises(NotImplementedError, match="ambient occlusion"):
        sc.set_supersampling(3)
        ntracer_amd.BlockingRenderer().render(bytearray(size), fmt, sc)
    # each of them in the setting's own words, which tests/view_setting_refusals.py has byte for byte and
    # tests/test_view_setting_refusals.py holds every render form to; the sixth, the row range, is a guard for callers inside
    # nt_api.cpp (the entry points hand over whole images unless band_world > 1, which is refused first), so it can only be
    # read, not reached: the same test reads it
    import view_setting_refusals as vr
    words = [m for (setting, _), m in vr.RENDER_REFUSALS.items() if setting == "ao"]
    assert len(words) == 5 and all(m.startswith("ambient occlusion is not available") for m in words)
