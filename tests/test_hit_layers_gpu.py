"""Hit layers on the GPU against tests/layer_cases.py: the records of nt_hit_layers (host form) and _device (a torch tensor) on the
packet walk and on the general route, the packet walk without numerators and tile order, the forced general route against the
packet's bytes, and the cross-checks with primary_hits and crossing_counts.

On every compared ray (layer_cases.expected: ordinary in xray_cases, no Solid among its first layers + 1 within 1e-4 * max(1, t) of
a neighbour) count, item and lane are equal and dist is equal bit for bit, but for a Solid's dist, which lies within
1e-5 * max(1, t).  test_hit_layers_host.py holds every view to at most 1 % of rays left out.  One reference a scene and size, kept.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import layer_cases as lc
import xray_cases as xc
import support as sup
from ntracer_amd import _lib, tracern

pytestmark = pytest.mark.gpu

SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL", "NTRACER_NUMERATORS",
            "NTRACER_TILE_ORDER", "NTRACER_FRAME_MAJOR", "NTRACER_CHUNK_FRAMES")
VAR = {"NTRACER_FORCE_VAR": "1"}
W, H = 37, 21
ids = lambda cases: ["%s-%dx%d-%d" % c for c in cases]


def _scene(name, mp, env=None):
    sup.set_switches(mp, SWITCHES, env or {})
    n, flat, params, fov, cam = xc.scene(name)
    sc = tracern.CompositeScene.from_flat(n, flat)
    if params is not None:
        sc.set_params_flat(params)
    sc.set_fov(fov)
    sc._set_camera_arrays(*cam(0))
    return sc


def _both_forms(sc, name, w, h, layers, label):
    """the host form's records, held to the reference; the device form's must be the same bytes"""
    import torch
    got = sc.hit_layers(w, h, layers)
    lc.assert_records(got.records, name, w, h, layers, label + " host form")
    dev = sc.hit_layers(w, h, layers, device="cuda")
    torch.cuda.synchronize()
    assert dev.records.is_cuda and dev.records.dtype == torch.int32 and tuple(dev.records.shape) == (layers, h, w, 4)
    assert np.array_equal(dev.records.cpu().numpy(), got.records), label + ": the device form differs from the host form"
    return got


@pytest.mark.parametrize("name,w,h,layers", lc.PACKET, ids=ids(lc.PACKET))
def test_records_on_the_packet_walk(name, w, h, layers):
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        got = _both_forms(sc, name, w, h, layers, name)
        # the fields are views of the records
        assert np.array_equal(got.dist.view(np.int32), got.records[..., 0]) and got.dist.dtype == np.float32
        assert np.array_equal(got.item, got.records[..., 1]) and np.array_equal(got.lane, got.records[..., 2])
        assert np.array_equal(got.count, got.records[0, :, :, 3]) and np.array_equal(got.cut, got.count > layers)
        none = got.item < 0
        assert np.array_equal(got.kind[~none], got.item[~none] & 3) and np.array_equal(got.index[~none], got.item[~none] >> 2)
        assert (got.kind[none] == -1).all() and (got.index[none] == -1).all() and (got.lane[none] == -1).all()
        assert (got.dist[none] == xc.FLT_MAX).all()
        # a layer is there exactly below the pixel's count
        assert np.array_equal(~none, np.arange(layers)[:, None, None] < got.count[None])
        if name == xc.BUILT:
            # the repeated facet of the padded batch is no layer
            assert set(got.count.ravel().tolist()) == {0, 2}
            assert none[2:].all() and not none[:2][:, got.count == 2].any()


def test_the_packet_walk_without_numerators_and_tile_order_writes_the_same_bytes():
    with pytest.MonkeyPatch.context() as mp:
        want = _scene("cell120_n4", mp).hit_layers(W, H, 8).records
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell120_n4", mp, {"NTRACER_NUMERATORS": "0", "NTRACER_TILE_ORDER": "0"})
        got = sc.hit_layers(W, H, 8).records
    lc.assert_records(got, "cell120_n4", W, H, 8, "cell120_n4 plain launch")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name,w,h,layers", lc.GENERAL, ids=ids(lc.GENERAL))
def test_records_on_the_general_route(name, w, h, layers):
    """(the Solids of these scenes: a sphere's dist is the float64 evaluation rounded once, which is what brings feature16_n16
    inside 1e-5 * max(1, t) -- the Solid's own fp32 quadratic lies up to 2.51e-05 from float64 on this view)"""
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        _both_forms(sc, name, w, h, layers, name)


@pytest.mark.parametrize("name,w,h,layers", lc.FORCED, ids=ids(lc.FORCED))
def test_the_general_route_writes_the_packet_walks_bytes(name, w, h, layers):
    with pytest.MonkeyPatch.context() as mp:
        packet = _scene(name, mp).hit_layers(w, h, layers).records
    with pytest.MonkeyPatch.context() as mp:
        forced = _both_forms(_scene(name, mp, VAR), name, w, h, layers, name + " FORCE_VAR").records
    assert np.array_equal(packet, forced)


@pytest.mark.parametrize("name", ["cell600_n4", "cell120_n4"])
def test_layer_0_is_the_primary_hit_and_the_count_is_the_crossing_count(name):
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        one = sc.hit_layers(W, H, 1)
        hits = sc.primary_hits(W, H)
        assert (hits.dist < xc.FLT_MAX).sum() > 100
        assert np.array_equal(one.dist[0].view(np.int32), np.ascontiguousarray(hits.dist).view(np.int32))
        assert np.array_equal(one.count, sc.crossing_counts(W, H))
        if name == "cell600_n4":
            two = sc.hit_layers(W, H, 2)
            ys, xs = np.nonzero(two.count == 2)
            assert len(ys) > 100
            y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
            obj, lane = two.primitive(x, y, 1)
            assert isinstance(obj, tracern.TriangleBatch) and 0 <= lane <= 3
            assert obj is sc._object_of(0, int(two.index[1, y, x])) and lane == int(two.lane[1, y, x])
            ys, xs = np.nonzero(two.count == 0)
            assert two.primitive(int(xs[0]), int(ys[0]), 0) is None


@pytest.mark.parametrize("name", ["feature5_n5", "feature16_n16"])
def test_a_cube_layer_carries_the_bits_of_the_primary_hit(name):
    """A Solid cube's dist is the Solid's own fp32 test, the one a render runs: where the nearest opaque hit is the cube of layer
    0, the same bits.  (A sphere's is evaluated in float64, nt_layer_list.hpp, and is held to the float64 reference instead.)"""
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        one = sc.hit_layers(W, H, 1)
        hits = sc.primary_hits(W, H)
        types = np.asarray(xc.scene(name)[1]["solid_types"]).reshape(-1)
        same = (one.kind[0] == 2) & (np.asarray(hits.item) == one.item[0])
        cube = same & (types[np.where(same, one.index[0], 0)] == 1)
        print("%s: layer 0 is the Solid of the primary hit on %d pixels, %d of them a cube's" % (name, int(same.sum()), int(cube.sum())))
        assert cube.sum() >= 10
        assert np.array_equal(one.dist[0].view(np.int32)[cube], np.ascontiguousarray(hits.dist).view(np.int32)[cube])


def test_the_device_form_on_another_stream_leaves_the_plane_behind_alone():
    import torch
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell120_n4", mp)
        layers = 3
        want = sc.hit_layers(W, H, layers).records
        buf = torch.full((layers + 1, H, W, 4), 0x3D3D3D3D, dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        opts = _lib.NtRenderOpts()
        opts.device = torch.cuda.current_device()
        with torch.cuda.stream(stream):
            _lib.check(_lib.lib().nt_hit_layers_device(sc._handle, W, H, layers, C.c_void_p(buf.data_ptr()), C.byref(opts), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:layers], want)
        assert (got[layers] == 0x3D3D3D3D).all()


def test_two_calls_of_different_layers_on_one_scene_each_answer_their_own():
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell120_n4", mp)
        for layers in (8, 2, 3):
            lc.assert_records(sc.hit_layers(W, H, layers).records, "cell120_n4", W, H, layers, "cell120_n4 after another call")
