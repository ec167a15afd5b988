"""Colours of caller-supplied rays (nt_ray_colors / nt_render_rays and their _device forms; Scene.ray_colors / render_rays)
against the oracle: every ray of every case is compared, none is left out.

The expected colour of a ray is the oracle's colour of the centre pixel of a 2 x 2 view through a camera at the ray's origin
that looks along it (ray_color_cases.CentrePixel; tests/test_ray_colors_host.py pins that method), the oracle in the GPU's
mode.  CompositeScene: every component of every ray within 1e-5, the project's composite tolerance (the arithmetic is the
oracle's except through powf).  BoxScene: array_equal.

Each test runs its GPU work once; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import oracle_binding as ob
import ray_color_cases as rc
import ray_query_cases as rq
import support as sup
import ntracer_amd
from ntracer_amd import _lib, tracern

pytestmark = pytest.mark.gpu

TOL = 1e-5
LAUNCHES = (1, 63, 64, 65, 257)         # a partial wave, a wave, a partial block, more than one block
f32 = np.float32

# the cases that also go through nt_ray_colors_device: two a family (fixed n / run-time n, opaque / transparent)
DEVICE_CASES = {rc.case_id(c) for c in (("cell600_n4", {}, "lit"), ("simplex10_n10", {}, ""), ("feature5_n5", {}, ""), ("feature5_n5", rc.CLEAN, ""),
                                        ("simplex10_n10", rc.VAR, ""), ("feature5_n5", rc.VAR, "transparent_reflective"),
                                        ("feature11_n11", {}, ""), ("feature11_n11", rc.CLEAN, ""))}
DEVICE_BOX = (6, 24, 25, 40)


def _scene(case, mp):
    name, env, variant = case
    sup.set_switches(mp, rc.SWITCHES, env)
    n, flat, params = rc.case_scene(case)
    sc = tracern.CompositeScene.from_flat(n, flat)
    sc.set_params_flat(params)
    return sc


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(sup.cuda_device())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_composite_colours_equal_the_oracle(case):
    rc.check_floors(case)
    r = rc.rays(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        got = sc.ray_colors(r.origins, r.directions)
        assert got.shape == r.ref.shape and got.dtype == f32
        err = np.abs(got.astype(np.float64) - r.ref).max(axis=1)
        print("%s: %d rays, worst difference %g; per slice %s" % (rc.case_id(case), len(err), err.max(),
                                                                  {k: float(err[sl].max()) for k, sl in r.slices.items()}))
        bad = np.nonzero(~(err <= TOL))[0]
        assert len(bad) == 0, "%s: %d rays beyond %g, first %d: got %r, oracle %r" % (rc.case_id(case), len(bad), TOL, bad[0], got[bad[0]], r.ref[bad[0]])
        assert len(np.unique(r.ref, axis=0)) > 50                       # (colours, not one background)
        if rc.case_id(case) in DEVICE_CASES:
            import torch
            dgot = sc.ray_colors(_dev(r.origins), _dev(r.directions))
            torch.cuda.synchronize()
            assert dgot.device.type == "cuda" and tuple(dgot.shape) == got.shape
            assert np.array_equal(_bits(dgot.cpu().numpy()), _bits(got)), rc.case_id(case)


@pytest.mark.parametrize("n", rc.BOX_DIMS)
def test_box_colours_equal_the_oracle(n):
    r = rc.box_rays(n)
    assert r.hits >= rc.MIN_BOX_HITS, (n, r.hits)
    sc = tracern.BoxScene(n)
    got = sc.ray_colors(r.origins, r.directions)
    bad = np.nonzero((got.view(np.uint32) != r.ref.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, "BoxScene(%d): %d rays differ, first %d: got %r, oracle %r" % (n, len(bad), bad[0], got[bad[0]], r.ref[bad[0]])
    assert np.array_equal(got, r.ref)
    if n in DEVICE_BOX:
        import torch
        dgot = sc.ray_colors(_dev(r.origins), _dev(r.directions))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dgot.cpu().numpy()), _bits(got))


def test_launch_sizes():
    """prefixes of the ray set in launches of a partial wave, a wave, a partial block and more than one block: the same
    colours as the same rays have in the full launch"""
    for case in (("cell600_n4", {}, "lit"), ("feature5_n5", {}, ""), ("feature11_n11", {}, "")):
        r = rc.rays(case)
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp)
            full = sc.ray_colors(r.origins, r.directions)
            for k in LAUNCHES:
                assert np.array_equal(_bits(sc.ray_colors(r.origins[:k], r.directions[:k])), _bits(full[:k])), (rc.case_id(case), k)
    for n in (6, 25):
        r = rc.box_rays(n)
        sc = tracern.BoxScene(n)
        for k in LAUNCHES:
            assert np.array_equal(sc.ray_colors(r.origins[:k], r.directions[:k]), r.ref[:k]), (n, k)


@pytest.mark.parametrize("case,count", [(("feature5_n5", {}, ""), 300000), (("feature11_n11", {}, ""), 270000)], ids=["fixed_n", "run_time_n"])
def test_capped_grid_strides(case, count):
    """the walks with the exact `checked` list keep a scratch column per resident lane, so their grid is capped -- at most
    1 024 blocks of 256 lanes, 4 096 of 64 at run-time n -- and the blocks stride: the ray set tiled on the device to more
    rays than that.  Every tile equals the first, and the first equals the oracle."""
    import torch
    r = rc.rays(case)
    m = len(r.ref)
    assert count > (1024 * 256 if case[0] == "feature5_n5" else 4096 * 64)
    reps = -(-count // m)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        o = _dev(r.origins).repeat(reps, 1)[:count].contiguous()
        d = _dev(r.directions).repeat(reps, 1)[:count].contiguous()
        got = sc.ray_colors(o, d)
        torch.cuda.synchronize()
        first = got[:m]
        whole = (count // m) * m
        assert bool((got[:whole].view(count // m, m, 3).view(torch.int32) == first.view(torch.int32)[None]).all())
        assert bool((got[whole:].view(torch.int32) == first[:count - whole].view(torch.int32)).all())
        err = np.abs(first.cpu().numpy().astype(np.float64) - r.ref)
        assert err.max() <= TOL, err.max()


def test_shared_origin_equals_an_origin_a_ray():
    """the rays of one camera with `origins` of shape [n] and of shape [count][n]: the same bits"""
    import torch
    for case in (("feature5_n5", {}, ""), ("cell600_n4", {}, "lit"), ("feature11_n11", {}, ""), ("simplex10_n10", rc.VAR, "")):
        r = rc.rays(case)
        A = r.slices["A"]
        one = np.nonzero((r.origins[A] == r.origins[0]).all(axis=1))[0]
        assert len(one) >= 100
        o, d = np.ascontiguousarray(r.origins[one]), np.ascontiguousarray(r.directions[one])
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp)
            each = sc.ray_colors(o, d)
            shared = sc.ray_colors(o[0], d)
            assert np.array_equal(_bits(each), _bits(shared)), rc.case_id(case)
            dshared = sc.ray_colors(_dev(o[0]), _dev(d))
            torch.cuda.synchronize()
            assert np.array_equal(_bits(dshared.cpu().numpy()), _bits(each)), rc.case_id(case)
            assert np.abs(each.astype(np.float64) - r.ref[one]).max() <= TOL
    for n in (6, 25):
        r = rc.box_rays(n)
        sc = tracern.BoxScene(n)
        k = r.per_camera
        assert np.array_equal(sc.ray_colors(r.origins[0], r.directions[:k]), r.ref[:k])
        assert np.array_equal(sc.ray_colors(np.ascontiguousarray(r.origins[k]), r.directions[k:2 * k]), r.ref[k:2 * k])


def _view(w, h):
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    return xs.ravel().astype(np.int32), ys.ravel().astype(np.int32)


def test_the_cameras_own_rays_give_the_cameras_own_colours():
    """the camera's unnormalised rays of a 97 x 61 view through ray_colors, and colors_at of every pixel: the same device
    function on the same inputs, so the same bits"""
    w, h = 97, 61
    xs, ys = _view(w, h)
    g, n, flat = rq.scene("feature5_n5")
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(("feature5_n5", {}, ""), mp)
        f = int(g["frames"][1])
        sc._set_camera_arrays(g["origins"][f], g["axes"][f])
        v = rc.camera_rays(g["axes"][f], xs, ys, w, h, sc.fov)
        a = sc.ray_colors(np.asarray(g["origins"][f], f32), v)
        b = sc.colors_at(xs, ys, w, h)
        assert np.array_equal(_bits(a), _bits(b))
        assert len(np.unique(b, axis=0)) > 100
    for n, cam in ((6, 17), (25, 3)):
        sc = tracern.BoxScene(n)
        if n == 6:
            gb = fx.load("box_n6_1920x1080")
            o, q = np.asarray(gb["origins"][cam], f32), np.asarray(gb["axes"][cam], f32)
        else:
            o, q = fx.stress_cameras(n, np.random.default_rng(rc.SEED))[cam]
        sc._set_camera_arrays(o, q)
        a = sc.ray_colors(o, rc.camera_rays(q, xs, ys, w, h, sc.fov))
        b = sc.colors_at(xs, ys, w, h)
        assert np.array_equal(_bits(a), _bits(b)), n
        assert (b[:, 0] != b[:, 1]).sum() >= 100, n               # rays that hit the cube


BOX_FORMATS = [(fx.RGBX8, 0, False), (fx.RGBX8, 8, False), (fx.RGB16, 0, True), (fx.RGB16, 7, False), (fx.RGBF32, 0, False),
               (fx.RGBF32, 12, True)]               # (channels, bytes of pitch padding, reversed)


@pytest.mark.parametrize("n", [6, 25])
def test_render_rays_of_a_box_scene_equals_the_oracles_render(n):
    import torch
    w, h = 97, 61
    xs, ys = _view(w, h)
    if n == 6:
        gb = fx.load("box_n6_1920x1080")
        o, q = np.asarray(gb["origins"][17], f32), np.asarray(gb["axes"][17], f32)
    else:
        o, q = fx.stress_cameras(n, np.random.default_rng(rc.SEED))[3]
    sc = tracern.BoxScene(n)
    v = rc.camera_rays(q, xs, ys, w, h, sc.fov)
    orc = ob.OracleScene(n, o, q)
    for chans, pad, rev in BOX_FORMATS:
        bpp = sum(c[0] for c in chans) // 8
        pitch = w * bpp + pad
        fmt = sup.fmt_of(w, h, chans, pitch if pad else 0, rev)
        ref = orc.render(w, h, chans, pitch=pitch if pad else 0, reversed_=rev)
        buf = bytearray(pitch * h)
        assert sc.render_rays(buf, fmt, o, v) is True
        got = np.frombuffer(bytes(buf), np.uint8).reshape(h, pitch)
        assert np.array_equal(got, ref), (n, chans, pad, rev, int((got != ref).sum()))
        # the device form: the padding keeps the caller's bytes
        dest = torch.full((h, pitch), 0xab, dtype=torch.uint8, device=sup.cuda_device())
        assert sc.render_rays(dest, fmt, _dev(o), _dev(v)) is True
        torch.cuda.synchronize()
        dgot = dest.cpu().numpy()
        assert np.array_equal(dgot[:, :w * bpp], ref[:, :w * bpp]), (n, chans, pad, rev)
        assert (dgot[:, w * bpp:] == 0xab).all()
    assert (ref != 0).any()


def test_render_rays_of_a_composite_scene_packs_its_own_colours():
    """feature5_n5 through the camera's own rays: the image is nto_pack_pixel of the GPU's own ray_colors, byte for byte, and
    lies within 1 LSB of the oracle's frame; the device form writes the same bytes"""
    import torch
    w, h = 97, 61
    xs, ys = _view(w, h)
    g, n, flat = rq.scene("feature5_n5")
    f = int(g["frames"][1])
    o, q = np.asarray(g["origins"][f], f32), np.asarray(g["axes"][f], f32)
    params = fx.params_of(g)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(("feature5_n5", {}, ""), mp)
        v = rc.camera_rays(q, xs, ys, w, h, sc.fov)
        colours = sc.ray_colors(o, v)
        orc = ob.OracleScene(n, o, q, float(g["fov"]), flat=flat, params=params)
        for chans, pad, rev in ((fx.RGBX8, 0, False), (fx.RGB16, 7, True)):
            bpp = sum(c[0] for c in chans) // 8
            pitch = w * bpp + pad
            fmt = sup.fmt_of(w, h, chans, pitch if pad else 0, rev)
            buf = bytearray(pitch * h)
            assert sc.render_rays(buf, fmt, o, v) is True
            got = np.frombuffer(bytes(buf), np.uint8).reshape(h, pitch)
            packed = np.frombuffer(b"".join(ob.pack_pixel(c, chans, rev) for c in colours), np.uint8).reshape(h, w * bpp)
            assert np.array_equal(got[:, :w * bpp], packed), (chans, int((got[:, :w * bpp] != packed).sum()))
            assert not got[:, w * bpp:].any()
            ref = orc.render(w, h, chans, pitch=pitch if pad else 0, reversed_=rev, threads=4)
            if bpp == 4:
                assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1
            else:
                words = lambda a: np.ascontiguousarray(a[:, :w * bpp]).view("<u2" if rev else ">u2").astype(int)
                assert np.abs(words(got) - words(ref)).max() <= 1
            dest = torch.zeros((h, pitch), dtype=torch.uint8, device=sup.cuda_device())
            assert sc.render_rays(dest, fmt, _dev(o), _dev(v)) is True
            torch.cuda.synchronize()
            assert np.array_equal(dest.cpu().numpy(), got)
        with pytest.raises(ValueError):
            sc.render_rays(bytearray(w * h * 4), sup.fmt_of(w, h, fx.RGBX8), _dev(o), _dev(v))       # host bytes, device rays


def test_abort_word_raised_before_the_call_nothing_is_written():
    """the pattern of test_abort_word_on_the_batched_device_path: raised, no block writes; lowered, the same call answers"""
    import torch
    dev = sup.cuda_device()
    word = torch.ones(1, dtype=torch.int32, device=dev)
    w, h = 50, 20
    fmt = sup.fmt_of(w, h, fx.RGBX8)
    fst = fmt._as_struct()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = _lib.lib()
    with pytest.MonkeyPatch.context() as mp:
        scenes = [(_scene(c, mp), rc.rays(c)) for c in (("cell600_n4", {}, "mirror"), ("feature5_n5", {}, ""), ("feature11_n11", {}, ""))]
        scenes += [(tracern.BoxScene(n), rc.box_rays(n)) for n in (6, 25)]
        for sc, r in scenes:
            count = w * h
            o, d = _dev(r.origins[:count]), _dev(r.directions[:count])
            rgb = torch.full((count, 3), 7.0, dtype=torch.float32, device=dev)
            dest = torch.full((h, fmt.pitch), 0xab, dtype=torch.uint8, device=dev)
            rays = _lib.NtRays()
            rays.count, rays.origins, rays.directions, rays.shared_origin = count, o.data_ptr(), d.data_ptr(), 0
            opts = _lib.NtRenderOpts()
            opts.device = dev.index
            opts.abort_device = word.data_ptr()

            def go():
                assert L.nt_ray_colors_device(sc._handle, C.byref(rays), rgb.data_ptr(), C.byref(opts), stream) == _lib.NT_OK
                assert L.nt_render_rays_device(sc._handle, dest.data_ptr(), dest.numel(), C.byref(fst), C.byref(rays), C.byref(opts), stream) == _lib.NT_OK
                torch.cuda.synchronize()
            word.fill_(1)
            torch.cuda.synchronize()
            go()
            assert bool((rgb == 7.0).all()) and bool((dest == 0xab).all())
            word.fill_(0)
            torch.cuda.synchronize()
            go()
            want = sc.ray_colors(r.origins[:count], r.directions[:count])
            assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(want))
            buf = bytearray(fmt.pitch * h)
            sc.render_rays(buf, fmt, r.origins[:count], r.directions[:count])
            assert bytes(buf) == dest.cpu().numpy().tobytes()
            # every other field of the options must be 0
            opts.collect_stats = 1
            assert L.nt_ray_colors_device(sc._handle, C.byref(rays), rgb.data_ptr(), C.byref(opts), stream) == _lib.NT_E_INVALID


@pytest.mark.parametrize("name", ["feature5_n5", "feature11_n11"])
def test_a_render_after_a_ray_call_still_gives_the_golden_frame(name):
    """the `checked` and frame scratch is shared between renders and ray calls (both grow it): a golden camera's frame before
    a ray call, after a small one and after one large enough to reallocate the scratch -- the same bytes, the oracle's frame"""
    case = (name, {}, "")
    g, n, flat = rq.scene(name)
    w, h = int(g["width"]), int(g["height"])
    k = 1
    f = int(g["frames"][k])
    fmt = sup.fmt_of(w, h, fx.RGBF32)
    r = rc.rays(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        sc._set_camera_arrays(g["origins"][f], g["axes"][f])

        def frame():
            buf = bytearray(fmt.pitch * h)
            assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
            return bytes(buf)
        before = frame()
        small = sc.ray_colors(r.origins[:100], r.directions[:100])
        assert frame() == before
        reps = 120
        big = sc.ray_colors(np.concatenate([r.origins] * reps), np.concatenate([r.directions] * reps))
        assert frame() == before
        assert np.array_equal(_bits(big[:100]), _bits(small)) and np.array_equal(_bits(big[-len(r.ref):]), _bits(big[:len(r.ref)]))
        ref = ob.OracleScene(n, g["origins"][f], g["axes"][f], float(g["fov"]), flat=flat, params=fx.params_of(g)).render(w, h, fx.RGBF32, threads=4)
        assert np.abs(np.frombuffer(before, ">f4") - ref.view(">f4").ravel()).max() <= TOL
        # ... and the reference's own colours of the golden pixels, to the tolerance and the share test_gpu_parity.py holds them to
        pix = np.frombuffer(before, ">f4").reshape(h, w, 3)[np.asarray(g["ys"]), np.asarray(g["xs"])]
        off = np.abs(pix - np.clip(g["colors"][k], 0.0, 1.0)).max(axis=1) > 1e-4
        assert off.sum() <= 0.002 * len(off), int(off.sum())


def test_an_empty_scene_gives_the_background():
    g, n, flat = rq.scene("cell600_n4")
    f = dict(flat)
    f["root"] = -1
    r = rc.rays(("cell600_n4", {}, "mirror"))
    sc = tracern.CompositeScene.from_flat(n, f)
    got = sc.ray_colors(r.origins[:300], r.directions[:300])
    want = rc.CentrePixel(n, f, fx.params_of(g)).colors(r.origins[:300], r.directions[:300])
    assert np.abs(got.astype(np.float64) - want).max() <= TOL
    assert len(np.unique(want, axis=0)) > 50
