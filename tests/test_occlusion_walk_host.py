"""The far-child exit of the occlusion walks, the part that needs no GPU: that the rays of tests/occlusion_walk_cases.py reach
the rule in both of its forms, and would tell a walk without it from the right one -- by the oracle and the module's model of the
walk alone.  tests/test_occlusion_walk_gpu.py sends the same batches through the kernels.

Per case the model with both rules equals the oracle on every ray, in `blocked` and in n_transparent (the per-leaf counts add up
on every ray here, the blocked ones included: a leaf's count up to its blocker is the one-leaf scene's own).  A walk "differs"
where blocked or n_transparent does, which is what the GPU test compares.  Run with -s, each case prints its census."""
import numpy as np
import pytest

import high_dimension_cases as hd
import occlusion_walk_cases as ow

MIN_RAYS = 10                   # rays taking each outcome, rays on which a walk without a rule differs, blocked, not blocked, transparent
MIN_FLIPS = 5                   # second legs whose verdict differs between 0.999 and 1.001 of the next hit's distance
CASES = [c for c, _ in ow.CASES]


@pytest.mark.parametrize("case", CASES, ids=ow.case_id)
def test_the_rays_reach_both_rules_and_the_model_equals_the_oracle(case):
    b, c = ow.batch(case), ow.census(case)
    label = ow.case_id(case)
    print("%s -> %s: %d rays (%d dropped); %s; without the descent exit %d rays differ, without the pop rule %d; blocked %d, "
          "n_transparent > 0 on %d, second legs that flip %d" % (
              label, ow.route(case), c["rays"], c["dropped"], ", ".join("%s %d" % kv for kv in zip(ow.OUTCOMES, c["outcomes"])),
              c["no_descent_exit"], c["no_pop_rule"], c["blocked"], c["transparent"], c["s_flips"]))
    # ---- the batch: 192 .. 256 rays, no whole number of waves, at most 5 % dropped for a tie, every set there
    assert 192 <= b.count <= 256 and b.count % 64, (label, b.count)
    assert b.dropped <= ow.MAX_DROPPED * b.total, (label, b.dropped, b.total)
    assert all((b.sets == s).sum() >= 10 for s in "IWSE"), label
    norm = np.sqrt((b.directions.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norm - 1).max() < 1e-6, label
    if case[0] >= 11:
        assert (b.origins[:, 3:] != 0).all() and (b.directions[:, 3:] != 0).all(), label
    # ---- set E: direction[2] exactly 0 in a filled cell, in an empty one and on a split; the origin on a split, both ways
    e = b.sets == "E"
    flat = ow.scene(case).flat
    splits = np.asarray(flat["node_split"])[np.asarray(flat["node_axis"]) >= 0]
    on_split = np.isin(b.origins[:, 2], splits)
    level = e & (b.directions[:, 2] == 0)
    cell = np.floor(b.origins[:, 2].astype(np.float64) * ow.CELLS).astype(int)
    assert (level & ~on_split & np.isin(cell, case[1])).sum() >= 2 and (level & ~on_split & ~np.isin(cell, case[1])).sum() >= 2, label
    assert (level & on_split).sum() >= 2, label
    assert (e & on_split & (b.directions[:, 2] > 0)).sum() >= 2 and (e & on_split & (b.directions[:, 2] < 0)).sum() >= 2, label
    assert not (b.directions[~e, 2] == 0).any() and not on_split[~e].any(), label
    # ---- no tie decides: no distance within 1e-4 (1 + t) of a split's or a leaf hit's t that the walk compares it with
    for r in range(b.count):
        if b.distance[r] < ow.FLT_MAX:
            for t in b.crossed[r] + b.hits[r]:
                assert abs(float(b.distance[r]) - t) > ow.TIE * (1 + abs(t)), (label, r, float(b.distance[r]), t)
    # ---- the model with both rules is the oracle
    for k in ("blocked", "n_transparent"):
        bad = np.nonzero(b.model["both"][k] != b.ref[k])[0]
        assert len(bad) == 0, "%s: the model's %s differs from the oracle's on %d rays; %s" % (label, k, len(bad), ow.describe(case, bad[0]))
    # ---- the floors
    for name, count in zip(ow.OUTCOMES, c["outcomes"]):
        assert count >= MIN_RAYS, (label, name, count)
    assert c["no_descent_exit"] >= MIN_RAYS and c["no_pop_rule"] >= MIN_RAYS, (label, c)
    assert c["blocked"] >= MIN_RAYS and c["rays"] - c["blocked"] >= MIN_RAYS, (label, c)
    if case[2] == "transparent":
        assert c["transparent"] >= MIN_RAYS, (label, c)
    else:
        assert c["transparent"] == 0, (label, c)
    assert c["s_flips"] >= MIN_FLIPS, (label, c)
    # (with every distance FLT_MAX and no window the exit is always taken: what the older tests feed these kernels)
    assert b.ref_far["blocked"].sum() >= MIN_RAYS and (b.ref_far["blocked"] != b.ref["blocked"]).sum() >= MIN_RAYS, label


def test_every_case_routes_to_the_kernel_it_claims():
    for case, kernel in ow.CASES:
        assert kernel in ow.KERNELS and ow.route(case) == kernel, (ow.case_id(case), kernel, ow.route(case))
        n, loose = case[0], case[3]
        assert len(ow.scene(case).flat["tri_recs"]) == (4 if loose else 0)
        if n > 10:
            # (high_dimension_cases.route reads the kind's materials on the full comb: the same rule at run-time n)
            assert hd.route(("wide", n, ow.TREE, case[2], False), "occludes") == kernel
    assert len(CASES) == len(set(CASES))


def test_every_kernel_meets_both_gap_patterns_and_every_native_dimension():
    for kernel in ow.KERNELS:
        mine = [c for c, k in ow.CASES if k == kernel]
        assert {c[1] for c in mine} == set(ow.PATTERNS), kernel
        if kernel in ow.VAR_KERNELS:
            native = {c[0] for c in mine if not c[4]}
            assert native == set(ow.NATIVE_DIMS), (kernel, native)
            assert {c[0] for c in mine if c[4]} == {5, 10}, kernel                  # forced to run-time n
            assert any(c[3] for c in mine), kernel                                  # loose triangles: the cut-off simplex test
        else:
            assert {c[0] for c in mine} == {4, 10} and not any(c[4] for c in mine), kernel


def test_the_lds_sizes_straddle_the_attribute():
    """64 (16 n + 4 depth + 64) bytes a block.  At stack depth 8: 39 936 bytes at n = 33, 66 560 at n = 59, 71 680 at n = 64.  The
    trees here are wide_comb(n, 7, ...), six nodes deep, which the library walks with a stack of 7: 39 680, 66 304 and 71 424 bytes,
    on the same sides of the 64 KiB beyond which the launch needs hipFuncAttributeMaxDynamicSharedMemorySize."""
    assert [hd.lds_bytes(n, 8) for n in (33, 59, 64)] == [39936, 66560, 71680]
    want = {11: 17152, 33: 39680, 59: 66304, 64: 71424}
    for case in CASES:
        s = ow.scene(case)
        assert s.stack_depth == ow.TREE and s.lds == hd.lds_bytes(case[0], ow.TREE), ow.case_id(case)
        if case[0] in want:
            assert s.lds == want[case[0]], (ow.case_id(case), s.lds)
    assert want[33] < hd.LDS_ATTRIBUTE < want[59] < want[64] < hd.LDS_LIMIT
