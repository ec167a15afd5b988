"""Every compile-time dimension reaches its own launcher (csrc/nt_dispatch.hpp), in the families whose other GPU tests sample
the dimensions: BoxScene's ray colours and refine kernels at n = 3 .. 24, CompositeScene's ray colours, ray queries and
primary hits at N = 3 .. 10.  The cases and the oracle's answers are tests/dimension_sweep_cases.py's (their floors:
tests/test_dispatch.py, on the CPU); each comparison is the sibling test's own, with its constants."""
import numpy as np
import pytest

import dimension_sweep_cases as dc
import fixtures as fx
import support as sup
from ntracer_amd import tracern
from test_adaptive_gpu import box_scene
from test_primary_hits_gpu import _check as check_hits
from test_ray_colors_gpu import TOL as TOL_COLOURS
from test_ray_queries_gpu import QUERY_SWITCHES, _check_intersect, _check_occludes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", range(3, 25))
def test_box_rays_and_refine_at_every_fixed_dimension(n):
    # ---- rays_box<n>: array_equal, as test_box_colours_equal_the_oracle
    r = dc.box_rays(n)
    got = tracern.BoxScene(n).ray_colors(r.origins, r.directions)
    bad = np.nonzero((got.view(np.uint32) != r.ref.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, "BoxScene(%d): %d rays differ, first %d: got %r, oracle %r" % (n, len(bad), bad[0], got[bad[0]], r.ref[bad[0]])
    # ---- refine_box<n>: byte for byte, mask included, as test_box_scene_equals_the_expected_image_and_mask_exactly
    w, h = dc.REFINE_VIEW
    e = dc.box_refine(n)
    sc = box_scene(n, dc.BOX_CAMERA, 2, e.t)
    for chans in (fx.RGBF32, fx.RGBX8):
        img = sup.render_host(sc, sup.fmt_of(w, h, chans))
        want = e.image(chans)
        assert np.array_equal(img, want), (n, int((img != want).sum()))
    assert np.array_equal(sc.refinement_mask(w, h), e.mask), n


@pytest.mark.parametrize("n", range(3, 11))
def test_composite_rays_queries_and_hits_at_every_fixed_dimension(n, monkeypatch):
    c = dc.composite(n)
    sup.set_switches(monkeypatch, QUERY_SWITCHES + ("NTRACER_COMPOSITE_KERNEL",), {})         # the default routes: the fixed-n launchers
    sc = tracern.CompositeScene.from_flat(n, c.flat)
    sc.set_params_flat(c.params)
    sc.set_fov(c.fov)
    sc._set_camera_arrays(c.origin, c.axes)
    label = "orthoplex N=%d" % n
    # ---- rays_color<N, ...>: within the composite tolerance, as test_composite_colours_equal_the_oracle
    got = sc.ray_colors(c.origins, c.directions)
    assert got.shape == c.colours.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - c.colours).max(axis=1)
    print("%s: %d rays, worst colour difference %g" % (label, len(err), err.max()))
    bad = np.nonzero(~(err <= TOL_COLOURS))[0]
    assert len(bad) == 0, "%s: %d rays beyond %g, first %d: got %r, oracle %r" % (label, len(bad), TOL_COLOURS, bad[0], got[bad[0]], c.colours[bad[0]])
    # ---- the query kernels, as test_queries_equal_the_oracle
    count = len(c.origins)
    full = sc.intersect_rays(c.origins, c.directions, c.t_near, c.t_far, c.none, c.none, normals=True)
    worst = _check_intersect(full, c.closest, slice(0, count), label + " intersects")
    print("%s: dist error %g, normal error %g" % (label, worst[0], worst[1]))
    occ = sc.occludes_rays(c.origins, c.directions, c.distance, c.t_near, c.t_far, c.none, c.none)
    _check_occludes(occ, c.blocked, slice(0, count), label + " occludes")
    # ---- the primary-hit kernels, as test_hits_equal_the_oracle
    w, h = dc.HITS_VIEW
    hits = sc.primary_hits(w, h, normals=True)
    check_hits(dict(dist=hits.dist, item=hits.item, lane=hits.lane, n_transparent=hits.n_transparent, normal_origin=hits.normal_origin,
                    normal_dir=hits.normal_dir), c.hits, label + " primary hits")
