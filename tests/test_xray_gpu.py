"""X-ray views on the GPU against tests/xray_cases.py: the counts of nt_crossing_counts (host form) and _device (a torch tensor)
on the packet walk and on the general route, the colours of a render with the setting on, two cameras in one call, and the
setting off again.

Counts are equal on every ray that is neither fuzzed nor unsafe, and differ on the others by at most the number of fuzzed or unsafe
primitives of that ray.  A colour channel of an ordinary ray lies within (k + 2) * 2^-23 * max(1, max B) of the float64
expectation, k the ray's count: k fp32 multiplications of relative error <= 2^-24 each, doubled for the unspecified order.  Into
RGBX8 every byte is within 1 of oracle_binding.pack_pixel of the expectation, the project's rule for composite frames.
test_xray_host.py holds every view to at most 1 % of such rays.  One reference a scene and size, kept (xray_cases.reference).

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import xray_cases as xc
import support as sup
from ntracer_amd import _lib, tracern

pytestmark = pytest.mark.gpu

SWITCHES = ("NTRACER_STRICT_REFERENCE", "NTRACER_CLEAN_NORMALS", "NTRACER_FORCE_VAR", "NTRACER_COMPOSITE_KERNEL", "NTRACER_NUMERATORS",
            "NTRACER_TILE_ORDER", "NTRACER_FRAME_MAJOR", "NTRACER_CHUNK_FRAMES")
VAR = {"NTRACER_FORCE_VAR": "1"}
W, H = 37, 21


def _scene(name, mp, env=None, k=0):
    sup.set_switches(mp, SWITCHES, env or {})
    n, flat, params, fov, cam = xc.scene(name)
    sc = tracern.CompositeScene.from_flat(n, flat)
    if params is not None:
        sc.set_params_flat(params)
    sc.set_fov(fov)
    sc._set_camera_arrays(*cam(k))
    return sc


def _assert_counts(got, name, w, h, label, k=0):
    r = xc.reference(name, w, h, k)
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == (h, w), label
    diff = np.abs(got.ravel().astype(np.int64) - r["count"])
    print("%s %dx%d: counts up to %d, %d rays differ (allowed on %d)" % (label, w, h, int(got.max()), int((diff != 0).sum()), int((~r["ordinary"]).sum())))
    bad = np.nonzero(r["ordinary"] & (diff != 0))[0]
    assert len(bad) == 0, "%s: %d ordinary rays differ, first ray %d: got %d, expected %d" % (
        label, len(bad), bad[0], got.ravel()[bad[0]], r["count"][bad[0]])
    assert (diff <= r["odd"]).all(), "%s: a fuzzed or unsafe ray is off by more than its fuzzed and unsafe primitives" % label


def _both_forms(sc, name, w, h, label):
    import torch
    got = sc.crossing_counts(w, h)
    _assert_counts(got, name, w, h, label + " host form")
    dev = sc.crossing_counts(w, h, device="cuda")
    torch.cuda.synchronize()
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (h, w)
    _assert_counts(dev.cpu().numpy(), name, w, h, label + " device form")
    return got


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("name,sizes", xc.PACKET, ids=[c[0] for c in xc.PACKET])
def test_counts_on_the_packet_walk(name, sizes):
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        for w, h in sizes:
            _both_forms(sc, name, w, h, name)
        # the setting has no say in a count
        sc.set_xray(0.3, 1.0)
        w, h = sizes[-1]
        _assert_counts(sc.crossing_counts(w, h), name, w, h, name + " with the setting on")


def test_the_packet_walk_without_numerators_and_tile_order_counts_the_same():
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell120_n4", mp, {"NTRACER_NUMERATORS": "0", "NTRACER_TILE_ORDER": "0"})
        _assert_counts(sc.crossing_counts(W, H), "cell120_n4", W, H, "cell120_n4 plain launch")


@pytest.mark.parametrize("name,sizes", xc.GENERAL, ids=[c[0] for c in xc.GENERAL])
def test_counts_on_the_general_route(name, sizes):
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        for w, h in sizes:
            _both_forms(sc, name, w, h, name)


@pytest.mark.parametrize("name,sizes", xc.FORCED, ids=[c[0] for c in xc.FORCED])
def test_the_general_route_counts_what_the_packet_walk_counts(name, sizes):
    for w, h in sizes:
        with pytest.MonkeyPatch.context() as mp:
            packet = _scene(name, mp).crossing_counts(w, h)
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(name, mp, VAR)
            forced = _both_forms(sc, name, w, h, name + " FORCE_VAR")
        assert np.array_equal(packet, forced)


# ------------------------------------------------------------------ renders
def colours_of(sc, w, h):
    return sup.render_host(sc, sup.fmt_of(w, h, fx.RGBF32)).view(">f4").astype(np.float32).reshape(h * w, 3)


def _assert_colours(got, name, a, t, label):
    r = xc.reference(name, W, H)
    want = np.clip(xc.expected_colour(name, W, H, a, t), 0.0, 1.0)
    bound = xc.colour_bound(name, W, H)
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    o = r["ordinary"]
    print("%s: largest error %.3g on ordinary rays, %.3g of its bound" % (label, err[o].max(), (err[o] / bound[o]).max()))
    assert (err[o] <= bound[o]).all(), "%s: %d ordinary rays beyond the bound, worst %g of it" % (label, int((err[o] > bound[o]).sum()), (err[o] / bound[o]).max())
    assert (got >= 0).all() and (got <= 1).all()
    return want


@pytest.mark.parametrize("name", xc.COLOURED)
@pytest.mark.parametrize("tint", [1.0, 0.0])
def test_colours_against_the_float64_expectation(name, tint):
    a = 0.3
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(name, mp)
        sc.set_xray(a, tint)
        r = xc.reference(name, W, H)
        got = colours_of(sc, W, H)
        want = _assert_colours(got, name, a, tint, "%s tint %g" % (name, tint))
        assert np.abs(got - r["B"]).max() > 0.05                            # the crossings show
        # RGBX8: every byte within 1 of the oracle's packing of the expectation
        rgbx = sup.render_host(sc, sup.fmt_of(W, H, fx.RGBX8)).reshape(H * W, 4).astype(np.int32)
        packed = np.array([list(ob.pack_pixel(want[i].astype(np.float32), fx.RGBX8)) for i in range(H * W)], np.int32)
        o = r["ordinary"]
        assert np.abs(rgbx - packed)[o].max() <= 1
        if tint == 0.0:
            # the grey X-ray: B * (1 - a)^count with the count of the same view
            counts = sc.crossing_counts(W, H).ravel()
            grey = r["B"].astype(np.float64) * ((1.0 - float(np.float32(a))) ** counts)[:, None]
            bound = (counts + 2) * 2.0 ** -23 * max(1.0, float(r["B"].max()))
            # (1.0f - 0.3f is rounded once more than 1 - float(0.3f): half an ulp of T a crossing, inside the doubled bound)
            assert (np.abs(got.astype(np.float64) - np.clip(grey, 0, 1)).max(axis=1) <= bound).all()


def test_the_general_route_draws_what_the_packet_walk_draws():
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell120_n4", mp, VAR)
        sc.set_xray(0.3, 1.0)
        _assert_colours(colours_of(sc, W, H), "cell120_n4", 0.3, 1.0, "cell120_n4 FORCE_VAR")


def test_two_cameras_in_one_call_equal_their_single_renders():
    """nt_render_frames_device, golden cameras 0 and 1 of the 600-cell: the seen set is cleared between tiles and frames"""
    import torch
    name = "cell600_n4"
    for env in ({}, {"NTRACER_FRAME_MAJOR": "0"}, {"NTRACER_CHUNK_FRAMES": "1"}, VAR):
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(name, mp, env)
            sc.set_xray(0.3, 1.0)
            fmt = sup.fmt_of(W, H, fx.RGBX8)
            cams = [xc.scene(name)[4](k) for k in range(2)]
            singles = []
            for o, axes in cams:
                sc._set_camera_arrays(o, axes)
                singles.append(sup.render_host(sc, fmt))
            assert not np.array_equal(singles[0], singles[1])
            frame_bytes = fmt.pitch * H + 64
            buf = torch.full((2 * frame_bytes,), 0x3D, dtype=torch.uint8, device="cuda")
            origins = np.ascontiguousarray([c[0] for c in cams], np.float32)
            axes = np.ascontiguousarray([c[1] for c in cams], np.float32)
            fst = fmt._as_struct()
            _lib.check(_lib.lib().nt_render_frames_device(sc._handle, C.c_void_p(buf.data_ptr()), frame_bytes, 2, origins.ctypes.data_as(_lib.f32p),
                                                          axes.ctypes.data_as(_lib.f32p), C.byref(fst), None,
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            got = buf.cpu().numpy().reshape(2, frame_bytes)
            for f in range(2):
                assert np.array_equal(got[f, :fmt.pitch * H].reshape(H, fmt.pitch), singles[f]), (env, f)
            assert (got[:, fmt.pitch * H:] == 0x3D).all()


def test_the_setting_off_again_leaves_the_plain_render_as_it_was():
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene("cell600_n4", mp)
        fmt = sup.fmt_of(W, H, fx.RGBX8)
        before = sup.render_host(sc, fmt)
        sc.set_xray(0.3, 1.0)
        xray = sup.render_host(sc, fmt)
        assert not np.array_equal(before, xray)
        sc.set_xray(None)
        assert np.array_equal(sup.render_host(sc, fmt), before)
