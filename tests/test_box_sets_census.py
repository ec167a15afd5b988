"""tools/box_sets_census.py -- box_stretch_code2 and the two classifiers of a ray-by-ray row restated in numpy -- on the bench's
160 cameras (CPU only): the shares of the four row classes DESIGN.md 4.1 works with, and the condition box_classify_sets rests
on: a "hit" or "miss" it gives from the stretch's T and C alone is the verdict box_classify gives from all N slabs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import box_sets_census as census  # noqa: E402


@pytest.fixture(scope="module")
def result():
    return census.bench_census(sample=3000, seed=7)


def test_row_class_shares_of_the_bench_call(result):
    share = result["share"]
    print({k: round(100 * v, 2) for k, v in share.items()})
    assert result["stretch_rows"] == 160 * 1080 * 30
    for name, pct in (("culled", 74.6), ("one_face", 14.7), ("near_tie", 3.9), ("ray_by_ray", 6.9)):
        assert abs(100 * share[name] - pct) <= 0.1, (name, 100 * share[name])


def test_sets_of_the_ray_by_ray_rows(result):
    """most ray-by-ray rows have valid sets, and small ones: that is what the restricted classifier saves on"""
    assert result["code15_sets_not_valid"] < 0.05
    assert result["mean_T"] < 2.0 and result["mean_C"] < 3.5
    assert abs(result["pairs"][(1, 2)] - 0.409) < 0.01 and abs(result["pairs"][(2, 2)] - 0.222) < 0.01


def test_restricted_verdicts_are_the_full_ones(result):
    s = result["sample"]
    print(s)
    assert s["rows"] == 3000
    assert s["rays_where_sets_verdict_is_not_the_full_one"] == 0
    # (its verdicts being a subset of the full one's, it leaves at least as many rows with an unclear lane)
    assert s["rows_unclear_sets"] >= s["rows_unclear_full"]
