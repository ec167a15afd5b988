"""The far-child exit of the occlusion walks (tracer.hpp:1298) on the GPU: the batches of tests/occlusion_walk_cases.py -- gapped
trees, origins inside the slab, t_near / t_far windows, finite distances on either side of the splits and of the hits -- through
occludes_rays on each of the five occlusion query kernels, at fixed N, forced to run-time n, and at n = 11, 33, 59 and 64.
`blocked` and n_transparent must equal the oracle's on every ray; none is left out.  That the rays reach the rule, and that a walk
without it answers differently on them, is tests/test_occlusion_walk_host.py's, on the CPU.

A failure names the first differing ray: its set, what the model's walk of it met, its distance and the t of the splits and leaf
hits it was compared with.  Each test runs its GPU work once; nothing is retried."""
import numpy as np
import pytest

import occlusion_walk_cases as ow
import support as sup
from ntracer_amd import tracern
from test_ray_queries_gpu import QUERY_SWITCHES, _check_occludes

pytestmark = pytest.mark.gpu


def _scene(case, mp):
    """the case's scene with the switches set before it is made"""
    s = ow.scene(case)
    sup.set_switches(mp, QUERY_SWITCHES, ow.env_of(case))
    sc = tracern.CompositeScene.from_flat(s.n, s.flat)
    sc.set_params_flat(s.params)
    return sc


def _check(got, ref, case, label):
    b = ow.batch(case)
    assert len(got["blocked"]) == b.count and len(got["n_transparent"]) == b.count, label
    bad = np.nonzero((np.asarray(got["blocked"]) != ref["blocked"]) | (np.asarray(got["n_transparent"]) != ref["n_transparent"]))[0]
    try:
        _check_occludes(got, ref, slice(0, b.count), label)
    except AssertionError as e:
        r = int(bad[0])
        raise AssertionError("%s (%d rays differ in all); got blocked %s, n_transparent %d; as sent in the first test, %s" % (
            e, len(bad), bool(got["blocked"][r]), int(got["n_transparent"][r]), ow.describe(case, r))) from None
    assert len(bad) == 0, label


@pytest.mark.parametrize("case", [c for c, _ in ow.CASES], ids=ow.case_id)
def test_occlusion_equals_the_oracle_on_gapped_trees(case):
    b = ow.batch(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        got = sc.occludes_rays(b.origins, b.directions, b.distance, b.t_near, b.t_far, b.skip_item, b.skip_lane)
    _check(got, b.ref, case, "%s (%s)" % (ow.case_id(case), ow.route(case)))


@pytest.mark.parametrize("kernel", ow.KERNELS)
def test_the_same_rays_without_a_distance_or_a_window(kernel):
    """what the older tests feed these kernels, on the new scenes: every distance FLT_MAX, no window -- one launch a kernel"""
    case = ow.first_case_of(kernel)
    b = ow.batch(case)
    with pytest.MonkeyPatch.context() as mp:
        sc = _scene(case, mp)
        got = sc.occludes_rays(b.origins, b.directions, b.far, b.no_near, b.no_far, b.skip_item, b.skip_lane)
    _check(got, b.ref_far, case, "%s (%s), distance FLT_MAX, whole window" % (ow.case_id(case), kernel))
