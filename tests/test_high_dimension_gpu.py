"""The run-time-n CompositeScene kernels (csrc/nt_var.hip) against the oracle at n = 17, 33, 59, 60 and 64, below and above
the 64 KiB of LDS at which a launch needs hipFuncAttributeMaxDynamicSharedMemorySize, at the 160 KiB limit and one step past it.

The scenes, the cases and the oracle's answers are tests/high_dimension_cases.py's (their floors, the LDS arithmetic and the
route of every call: tests/test_high_dimension_host.py, on the CPU).  Every comparison is the sibling test's own, with its
constant: the frame and the probes as test_composite_matrix.run_way (TOL_ORACLE), ray_colors as test_ray_colors_gpu (TOL), the
queries by test_ray_queries_gpu's checkers, the primary hits by test_primary_hits_gpu's (bitwise), the adaptive render and its
mask as test_adaptive_gpu.  Each test prints the worst difference of every family it compares.

Each test runs its GPU work once; nothing is retried."""
import numpy as np
import pytest

import adaptive_cases as ac
import fixtures as fx
import high_dimension_cases as hd
import support as sup
import ntracer_amd
import test_composite_matrix as tcm
from ntracer_amd import tracern
from test_adaptive_gpu import TOL_ORACLE as TOL_ADAPTIVE
from test_primary_hits_gpu import _check as check_hits
from test_ray_colors_gpu import TOL as TOL_COLOURS
from test_ray_queries_gpu import QUERY_SWITCHES, _check_intersect, _check_occludes

pytestmark = pytest.mark.gpu

W, H = hd.VIEW
TOL_ORACLE = tcm.TOL_ORACLE
SENTINEL = tcm.SENTINEL
SWITCHES = sorted(set(tcm.SWITCHES) | set(QUERY_SWITCHES) | {"NTRACER_COMPOSITE_KERNEL"})
TOO_DEEP = r"scene too deep for the LDS budget \(n 64, depth 369\)"


def _scene(case, mp, flat=None):
    """the case's scene with the switches set before it is made"""
    s = hd.scene(case)
    sup.set_switches(mp, SWITCHES, hd.env_of(case))
    sc = tracern.CompositeScene.from_flat(s.n, s.flat if flat is None else flat)
    sc.set_params_flat(s.params)
    sc._set_camera_arrays(s.origin, s.axes)
    return sc


def _render(sc, w=W, h=H):
    """one RGBF32 frame into a padded, sentinel-filled host buffer: (floats as (h, w * 3), padding bytes written)"""
    fmt = tcm._fmt(w, h)
    buf = bytearray([SENTINEL]) * (fmt.pitch * h)
    assert ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
    a = np.frombuffer(bytes(buf), np.uint8).reshape(h, fmt.pitch)
    return a[:, :w * 12].copy().view(">f4"), int((a[:, w * 12:] != SENTINEL).sum())


def _check_frame(sc, case, label):
    fr = hd.frame(case)
    img, stray = _render(sc)
    assert stray == 0, "%s: %d bytes of pitch padding written" % (label, stray)
    d = np.abs(img.astype(np.float64) - fr.frame)
    worst = float(d.max())
    assert worst < TOL_ORACLE, "%s: %d floats differ from the oracle (max %g), first at %r" % (
        label, int((d >= TOL_ORACLE).sum()), worst, tuple(np.argwhere(d >= TOL_ORACLE)[0]))
    return worst


@pytest.mark.parametrize("case", hd.core_cases(), ids=hd.case_id)
def test_every_call_equals_the_oracle(case):
    """render, colors_at, ray_colors, intersect_rays, occludes_rays and primary_hits of one case: six kernels of
    high_dimension_cases.route(case, ...)"""
    s, fr, r, hh = hd.scene(case), hd.frame(case), hd.rays(case), hd.hits(case)
    label = hd.case_id(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        # ---- render and colors_at, as test_composite_matrix.run_way
        worst_frame = _check_frame(sc, case, label + " render")
        got = sc.colors_at(fr.xs, fr.ys, W, H)
        worst_probe = float(np.abs(got.astype(np.float64) - fr.probes).max())
        assert worst_probe < TOL_ORACLE, "%s: colors_at differs from the oracle by %g" % (label, worst_probe)
        # ---- ray_colors on the camera's own rays, as test_composite_colours_equal_the_oracle
        got = sc.ray_colors(r.origins, r.directions)
        assert got.shape == r.colours.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - r.colours).max(axis=1)
        bad = np.nonzero(~(err <= TOL_COLOURS))[0]
        assert len(bad) == 0, "%s: %d rays beyond %g, first %d: got %r, oracle %r" % (label, len(bad), TOL_COLOURS, bad[0], got[bad[0]], r.colours[bad[0]])
        # ---- the query kernels, as test_queries_equal_the_oracle
        count = len(r.origins)
        full = sc.intersect_rays(r.origins, r.directions, r.t_near, r.t_far, r.none, r.none, normals=True)
        worst_q = _check_intersect(full, r.closest, slice(0, count), label + " intersects")
        occ = sc.occludes_rays(r.origins, r.directions, r.distance, r.t_near, r.t_far, r.none, r.none)
        _check_occludes(occ, r.blocked, slice(0, count), label + " occludes")
        # ---- the same three calls on rays whose hidden coordinates are all non-zero (high_dimension_cases.tilted)
        t = hd.tilted(case)
        got = sc.ray_colors(t.origins, t.directions)
        terr = np.abs(got.astype(np.float64) - t.colours).max(axis=1)
        bad = np.nonzero(~(terr <= TOL_COLOURS))[0]
        assert len(bad) == 0, "%s tilted: %d rays beyond %g, first %d: got %r, oracle %r" % (label, len(bad), TOL_COLOURS, bad[0], got[bad[0]], t.colours[bad[0]])
        full = sc.intersect_rays(t.origins, t.unit, r.t_near, r.t_far, r.none, r.none, normals=True)
        worst_t = _check_intersect(full, t.closest, slice(0, count), label + " tilted intersects")
        occ = sc.occludes_rays(t.origins, t.unit, r.distance, r.t_near, r.t_far, r.none, r.none)
        _check_occludes(occ, t.blocked, slice(0, count), label + " tilted occludes")
        # ---- the primary-hit kernels, as test_hits_equal_the_oracle: bitwise
        hits = sc.primary_hits(W, H, normals=True)
        check_hits(dict(dist=hits.dist, item=hits.item, lane=hits.lane, n_transparent=hits.n_transparent, normal_origin=hits.normal_origin,
                        normal_dir=hits.normal_dir), hh.hits, label + " primary hits")
        assert not sc.locked
    print("%s (LDS %d): worst difference from the oracle: frame %g, colors_at %g (< %g), ray_colors %g, tilted %g (<= %g), query dist %g, query normals %g, "
          "tilted %g, %g (<= 1e-05), primary hits 0 (bitwise)" % (label, s.lds, worst_frame, worst_probe, TOL_ORACLE, float(err.max()), float(terr.max()),
                                                                  TOL_COLOURS, worst_q[0], worst_q[1], worst_t[0], worst_t[1]))


@pytest.mark.parametrize("case", hd.refine_cases(), ids=hd.case_id)
def test_adaptive_renders_equal_the_expected_image_and_mask(case):
    """s = 2, t = adaptive_cases.T: decided pixels within the composite tolerance of the expected image, undecided ones of either
    variant; the mask equal on the decided pixels (test_adaptive_gpu.assert_decided_close, at this view's size)"""
    e = hd.refine(case)
    label = hd.case_id(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        sc.set_supersampling(hd.REFINE_S)
        sc.set_adaptive_supersampling(ac.T)
        img, stray = _render(sc)
        assert stray == 0, label
        got = img.astype(np.float32).reshape(H, W, 3)
        want = e.image(fx.RGBF32).view(">f4").astype(np.float32).reshape(H, W, 3)
        other = e.other_image(fx.RGBF32).view(">f4").astype(np.float32).reshape(H, W, 3)
        d, d2 = np.abs(got - want).max(axis=2), np.abs(got - other).max(axis=2)
        worst = float(d[~e.undecided].max())
        print("%s: refine, decided pixels: worst difference %g (<= %g); flagged %d, undecided %d of %d" % (
            label, worst, TOL_ADAPTIVE, int(e.mask.sum()), int(e.undecided.sum()), e.mask.size))
        assert worst <= TOL_ADAPTIVE, (label, worst, int((d[~e.undecided] > TOL_ADAPTIVE).sum()))
        assert (np.minimum(d, d2)[e.undecided] <= TOL_ADAPTIVE).all(), label
        mask = sc.refinement_mask(W, H)
        assert np.array_equal(mask[~e.undecided], e.mask[~e.undecided]), (label, int((mask != e.mask)[~e.undecided].sum()))


# ------------------------------------------------------------------ the five settings at n = 64
@pytest.mark.parametrize("case", hd.SETTING_CASES, ids=hd.case_id)
def test_the_five_settings_on_their_general_routes_at_n64(case):
    """a fisheye lens, the parallel projection, ambient occlusion at K = 5, outlines and depth cues on a 9 x 7 view of a scene of
    64 dimensions -- no packet walk at run-time n: the ray route behind lens_expand / parallel_expand, the query kernels behind
    ao_expand, and the primary-hit kernels behind outline_mark and cue_factors -- each compared as its sibling test compares"""
    import ao_cases as ao
    import cue_cases as cc
    import outline_cases as oc
    import ss_expected as sx
    import test_ao_gpu as tao
    import test_depth_cue_gpu as tcue
    import test_lens_gpu as tlens
    import test_outlines_gpu as tout
    import test_parallel_gpu as tpar
    c = hd.settings(case)
    w, h = hd.SMALL_VIEW
    label = hd.case_id(case)
    fmt = sup.fmt_of(w, h, fx.RGBF32)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        sc._set_camera_arrays(c.origin, c.axes)
        P = tcue.plain_colors(sc, w, h)
        worst_plain = float(np.abs(P.astype(np.float64) - c.plain).max())
        assert worst_plain < TOL_ORACLE, (label, worst_plain)
        # ---- a fisheye lens, as test_lens_renders_equal_the_oracle_on_every_pixel
        sc.set_lens(c.lens)
        got = tlens._floats(tlens._render(sc, fmt), w, h)
        worst_lens = tlens._check((label, {}, "", "fisheye"), got, c.lens_colours)
        masked = c.lens.masked.reshape(-1)
        assert (got[masked].view(np.uint32) == 0).all()
        sc.set_lens(None)
        # ---- the parallel projection, as test_parallel_gpu compares its renders
        sc.set_parallel_projection(hd.PARALLEL_HALF_WIDTH)
        got = tlens._floats(tlens._render(sc, fmt), w, h)
        worst_parallel = tpar._check((label, {}, ""), got, c.parallel_colours)
        sc.set_parallel_projection(None)
        # ---- ambient occlusion: the counts equal, the render the plain frame shaded by them
        sc.set_ambient_occlusion(c.ao_table, radius=ao.RADIUS, bias=ao.BIAS, strength=0.75)
        tao._both_forms(sc, w, h, c.ao["blocked"], label + " ambient occlusion")
        want = sx.pack(ao.shade(P, c.ao["blocked"], hd.AO_K, 0.75), fx.RGBF32, False)
        assert np.array_equal(sup.render_host(sc, fmt), want), label + ": the render under ambient occlusion"
        sc.set_ambient_occlusion(None)
        # ---- outlines: the mask equal, the render the plain frame with the lines drawn
        tout._set(sc, oc.A)
        tout._both_forms(sc, w, h, c.outline, label + " outlines")
        want = sx.pack(oc.blend(P, c.outline, tout.COLOR, tout.STRENGTH), fx.RGBF32, False)
        assert np.array_equal(sup.render_host(sc, fmt), want), label + ": the render with outlines"
        sc.set_outlines(None)
        # ---- depth cues, the tint axis non-zero in coordinate 63: the factors bit for bit, the render their blend
        tcue._set(sc, c.cue)
        tcue._both_forms(sc, w, h, c.cue_factors, label + " depth cue")
        want = sx.pack(cc.blend(P, c.cue_factors[..., 0], c.cue_factors[..., 1], c.cue), fx.RGBF32, False)
        assert np.array_equal(sup.render_host(sc, fmt), want), label + ": the render under the depth cue"
        sc.set_depth_cue(None)
    print("%s, 9 x 7, five settings: worst difference from the oracle: plain frame %g (< %g), fisheye %g, parallel %g (<= 1e-05); "
          "occlusion counts, outline mask and cue factors equal" % (label, worst_plain, TOL_ORACLE, worst_lens, worst_parallel))


# ------------------------------------------------------------------ the limits
@pytest.mark.parametrize("case", hd.limit_cases(), ids=hd.case_id)
def test_the_deepest_scene_that_fits_equals_the_oracle(case):
    """n = 64, stack_depth 368: 163 840 bytes, 160 KiB exactly; a primary ray pushes 366 entries"""
    s, fr = hd.scene(case), hd.frame(case)
    assert s.lds == hd.LDS_LIMIT and fr.centre["branches"] == hd.MAX_DEPTH_N64 - 2
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        worst = _check_frame(sc, case, hd.case_id(case))
    print("%s (LDS %d): worst difference from the oracle: frame %g (< %g)" % (hd.case_id(case), s.lds, worst, TOL_ORACLE))


def test_one_level_deeper_is_refused_before_anything_is_launched():
    """n = 64, stack_depth 369 would take 164 096 bytes.  Every entry point is refused by var_walk_ready, on the host, before the
    first kernel of the call -- the adaptive render's base frame is the first launch of that render, and its refusal ends it --,
    the scene is unlocked and the output is as it was; after the refusals of a kind a render and a ray call on a scene that
    fits succeed."""
    n = 64
    deep = hd.wide_comb(n, hd.MAX_DEPTH_N64 + 1, [0])
    assert hd.stack_depth_of(deep) == hd.MAX_DEPTH_N64 + 1 and hd.lds_bytes(n, hd.MAX_DEPTH_N64 + 1) > hd.LDS_LIMIT
    fits = ("wide", n, 4, "lit", False)
    r = hd.rays(fits)
    count = len(r.origins)
    fmt = tcm._fmt(W, H)
    clean_buf = bytearray([SENTINEL]) * (fmt.pitch * H)

    def render(sc):
        buf = bytearray(clean_buf)
        try:
            ntracer_amd.BlockingRenderer().render(buf, fmt, sc)
        finally:
            assert buf == clean_buf, "a refused render wrote to its buffer"

    def adaptive(sc):
        sc.set_supersampling(2)
        sc.set_adaptive_supersampling(ac.T)
        try:
            render(sc)
        finally:
            sc.set_adaptive_supersampling(None)
            sc.set_supersampling(1)

    xs, ys = hd.probe_lattice()
    calls = [("render", render), ("colors_at", lambda sc: sc.colors_at(xs, ys, W, H)),
             ("ray_colors", lambda sc: sc.ray_colors(r.origins, r.directions)),
             ("intersect_rays", lambda sc: sc.intersect_rays(r.origins, r.directions, normals=True)),
             ("occludes_rays", lambda sc: sc.occludes_rays(r.origins, r.directions)),
             ("primary_hits", lambda sc: sc.primary_hits(W, H, normals=True)), ("adaptive render", adaptive)]
    # the plain kernels, the _t<true> ones and, in clean mode, the _t<false> ones
    for kind, clean in (("lit", False), ("transparent_reflective", False), ("transparent_reflective", True)):
        case = ("wide", n, 4, kind, False)
        with pytest.MonkeyPatch.context() as mp:
            sc = _scene(case, mp, tcm._scene_flat(deep, kind))
            if clean:                                                # (read at every call: composite_route)
                mp.setenv("NTRACER_CLEAN_NORMALS", "1")
            for name, call in calls:
                with pytest.raises(RuntimeError, match=TOO_DEEP):
                    call(sc)
                assert not sc.locked, (kind, name)
            # caller-supplied output stays as it was
            out = np.full((count, 3), 7.0, np.float32)
            with pytest.raises(RuntimeError, match=TOO_DEEP):
                sc.ray_colors(r.origins, r.directions, out=out)
            assert (out == 7.0).all() and not sc.locked
            # the next call, on a scene that fits, succeeds
            mp.delenv("NTRACER_CLEAN_NORMALS", raising=False)
            ok = _scene(case, mp)
            _check_frame(ok, case, hd.case_id(case) + " after the refusals")
            got = ok.ray_colors(r.origins, r.directions)
            assert np.abs(got.astype(np.float64) - hd.rays(case).colours).max() <= TOL_COLOURS
