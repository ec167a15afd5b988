"""Hit layers, the part that needs no GPU: the reference of tests/layer_cases.py pinned to xray_cases (whose nearest t
test_xray_host.py pins to the oracle), the conditions that keep tests/test_hit_layers_gpu.py from being vacuous, the ABI, and every
answer the entry points give before a device is touched -- the messages written down here as literals."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import layer_cases as lc
import xray_cases as xc
from ntracer_amd import _lib, tracern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)

REFUSALS = {
    "null": "NULL argument",
    "size": "invalid view size",
    "layers": "the hit layers take 1 to 8 layers (%d)",
    "box": "not a composite scene",
    "clip": "clip planes are set: the hit layers is not available under them",
    "projection": "the hit layers are not available while a lens or the parallel projection is set",
    "records1": "1 layers of 65536 x 65536 pixels are beyond 2^31 - 1 records",
    "records8": "8 layers of 32768 x 32768 pixels are beyond 2^31 - 1 records",
    "options": "the hit layers read device, strict_reference and abort_device of their options: every other field must be 0",
}
SIMPLEX_VIEWS = [v for v in lc.VIEWS if not v[0].startswith("feature")]


# ------------------------------------------------------------------ the reference, and the conditions on the inputs
@pytest.mark.parametrize("name,w,h", lc.VIEWS, ids=lambda v: str(v))
def test_layer_0_is_the_nearest_crossing_and_the_count_is_the_crossing_count(name, w, h):
    r = xc.reference(name, w, h)
    ls = lc.lists(name, w, h)
    e = lc.expected(name, w, h, 1)
    assert np.array_equal(e["count"], r["count"])
    # xc.reference's `nearest` is of the simplices: the first entry of the list that is no Solid (every list here is kept whole
    # where it holds a Solid: the feature scenes cross 3 primitives at the most)
    simplex = ~ls["solid"] & np.isfinite(ls["t"])
    assert (ls["count"][ls["solid"].any(axis=1)] <= lc.KEPT).all()
    first = np.where(simplex.any(axis=1), ls["t"][np.arange(len(simplex)), simplex.argmax(axis=1)], xc.FLT_MAX).astype(np.float32)
    assert np.array_equal(bits(first), bits(r["nearest"]))
    if not ls["solid"].any():
        assert np.array_equal(bits(e["dist"][0]), bits(r["nearest"]))
    # the order is the rule's: keys strictly ascending along every list
    t, item, lane = ls["t"], ls["item"].astype(np.int64), ls["lane"].astype(np.int64)
    both = np.isfinite(t[:, 1:])
    lt = (t[:, :-1] < t[:, 1:]) | ((t[:, :-1] == t[:, 1:]) & ((item[:, :-1] < item[:, 1:]) | ((item[:, :-1] == item[:, 1:]) & (lane[:, :-1] < lane[:, 1:]))))
    assert lt[both].all()
    assert (np.isfinite(t).sum(axis=1) == np.minimum(ls["count"], lc.KEPT)).all()


def test_the_120_cell_cuts_its_lists_ties_and_nearly_ties():
    ls = lc.lists("cell120_n4", 37, 21)
    t, item, lane = ls["t"][:, :9], ls["item"][:, :9], ls["lane"][:, :9]
    there = np.isfinite(t[:, 1:])
    cut = int((ls["count"] > 8).sum())
    tied = (t[:, 1:] == t[:, :-1]) & there
    assert ((item[:, 1:] != item[:, :-1]) | (lane[:, 1:] != lane[:, :-1]))[tied].all()          # between distinct primitives
    with np.errstate(invalid="ignore"):
        close = ((t[:, 1:] - t[:, :-1]) <= 1e-4 * t[:, :-1]) & there
    ties, closes = int(tied.any(axis=1).sum()), int(close.any(axis=1).sum())
    print("more than 8 crossings: %d rays; bit-equal t among the first nine: %d rays; within 1e-4: %d rays" % (cut, ties, closes))
    assert cut >= 100              # (measured: 122)
    assert ties >= 5               # (measured: 11)
    assert closes > 100            # (measured: 130)


@pytest.mark.parametrize("name,w,h", [v for v in SIMPLEX_VIEWS if v[0] != "cell120_n4"], ids=lambda v: str(v))
def test_every_other_simplex_view_counts_0_or_2_and_has_no_ties(name, w, h):
    ls = lc.lists(name, w, h)
    assert set(ls["count"].tolist()) <= {0, 2}
    assert not ((ls["t"][:, 1:] == ls["t"][:, :-1]) & np.isfinite(ls["t"][:, 1:])).any()
    if w * h > 64:
        assert ls["count"].max() == 2


@pytest.mark.parametrize("name,w,h,layers", lc.PACKET + lc.GENERAL, ids=lambda v: str(v))
def test_at_most_one_ray_in_a_hundred_is_left_out(name, w, h, layers):
    e = lc.expected(name, w, h, layers)
    assert (~e["compared"]).sum() <= 0.01 * w * h, int((~e["compared"]).sum())


def test_the_solid_scenes_put_solids_into_the_layers():
    for name in ("feature5_n5", "feature11_n11", "feature16_n16"):
        e = lc.expected(name, 37, 21, 2)
        assert (e["solid"] & e["compared"][None]).sum() >= 10, name


# ------------------------------------------------------------------ the ABI
def test_the_exported_symbols_and_the_python_signature():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("nt_hit_layers", "nt_hit_layers_device"):
        assert hasattr(raw, name), name
    L = _lib.lib()
    assert L.nt_hit_layers.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(_lib.NtRenderOpts)]
    assert L.nt_hit_layers_device.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(_lib.NtRenderOpts), C.c_void_p]
    header = open(os.path.join(ROOT, "include", "ntracer_hip.h")).read()
    for decl in ("#define NT_LAYERS_MAX 8",
                 "int nt_hit_layers(nt_scene_t *s, int width, int height, int layers, nt_ray_hit *records, const nt_render_opts *opts);",
                 "int nt_hit_layers_device(nt_scene_t *s, int width, int height, int layers, void *records_dev, const nt_render_opts *opts, void *hip_stream);"):
        assert decl in header, decl
    params = [(p.name, p.default) for p in list(inspect.signature(tracern.CompositeScene.hit_layers).parameters.values())[1:]]
    assert params == [("width", inspect.Parameter.empty), ("height", inspect.Parameter.empty), ("layers", 4), ("device", None)]
    assert callable(tracern.HitLayers.primitive)


# ------------------------------------------------------------------ refusals
def test_both_forms_validate_before_they_touch_a_device():
    L = _lib.lib()
    n, flat, _, _, _ = xc.scene("cell120_n4")
    sc = tracern.CompositeScene.from_flat(n, flat)
    box = tracern.BoxScene(4)
    out = np.full(8 * 4 * 2 * 4, 77, np.int32)
    host = lambda s, w, h, k, p, o=None: L.nt_hit_layers(s, w, h, k, p, o)
    devf = lambda s, w, h, k, p, o=None: L.nt_hit_layers_device(s, w, h, k, p, o, None)

    def refused(status, code, key, *args):
        assert status == code, (key, status, _lib.last_error())
        assert _lib.last_error() == (REFUSALS[key] % args if args else REFUSALS[key])

    for on in (False, True):                 # the calls are answered with X-ray on: the same refusals, nothing about X-ray
        if on:
            sc.set_xray()
        for call in (host, devf):
            refused(call(None, 8, 4, 2, out.ctypes.data), _lib.NT_E_INVALID, "null")
            refused(call(sc._handle, 8, 4, 2, None), _lib.NT_E_INVALID, "null")
            for w, h in ((0, 4), (8, 0), (-1, 4), (8, -3)):
                refused(call(sc._handle, w, h, 2, out.ctypes.data), _lib.NT_E_INVALID, "size")
            for k in (0, -1, 9):
                refused(call(sc._handle, 8, 4, k, out.ctypes.data), _lib.NT_E_INVALID, "layers", k)
            refused(call(box._handle, 8, 4, 2, out.ctypes.data), _lib.NT_E_INVALID, "box")
            refused(call(sc._handle, 65536, 65536, 1, out.ctypes.data), _lib.NT_E_INVALID, "records1")
            refused(call(sc._handle, 32768, 32768, 8, out.ctypes.data), _lib.NT_E_INVALID, "records8")
            sc.set_clip_planes([((1,) + (0,) * (n - 1), 0.5)])
            refused(call(sc._handle, 8, 4, 2, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "clip")
            sc.set_clip_planes(None)
            sc.set_lens(tracern.Lens.pinhole(8, 4, 0.8))
            refused(call(sc._handle, 8, 4, 2, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "projection")
            sc.set_lens(None)
            sc.set_parallel_projection(2.0)
            refused(call(sc._handle, 8, 4, 2, out.ctypes.data), _lib.NT_E_UNSUPPORTED, "projection")
            sc.set_parallel_projection(None)
        for field in ("band_rank", "band_world", "band_rows", "compact", "collect_stats", "overlapped"):
            opts = _lib.NtRenderOpts()
            opts.device = -1
            setattr(opts, field, 1)
            refused(devf(sc._handle, 8, 4, 2, out.ctypes.data, C.byref(opts)), _lib.NT_E_INVALID, "options")
    assert (out == 77).all()


def test_the_python_method_refuses_before_the_library_is_called():
    n, flat, _, _, _ = xc.scene("cell600_n4")
    sc = tracern.CompositeScene.from_flat(n, flat)
    for layers in (0, -1, 9, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="layers must be an int in 1..8"):
            sc.hit_layers(8, 4, layers)
    with pytest.raises(ValueError):
        sc.hit_layers(0, 4)
    with pytest.raises(ValueError):
        sc.hit_layers(8, -1, 2)
    with pytest.raises(ValueError, match="not a composite scene"):
        tracern.BoxScene(4).hit_layers(8, 4)
