"""The dispatch over the dimension (csrc/nt_dispatch.hpp), without a GPU: the helper itself through a stand-alone program
(tests/dispatch_probe.cpp, host compiler), the built library's per-dimension launchers -- none missing, none unexpected, the
sets build.units() compiles -- and the floors of tests/dimension_sweep_cases.py, by the oracle alone."""
import os
import re
import shutil
import subprocess

import pytest

import dimension_sweep_cases as dc
from ntracer_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntracer_amd", "csrc")


def _bound(name):
    src = open(os.path.join(CSRC, "nt_device.hpp")).read()
    return int(re.search(r"#define %s (\d+)\b" % name, src).group(1))


def test_the_helper_calls_the_callee_of_n_once_and_nothing_out_of_range(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dispatch_probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "dispatch_probe.cpp"), "-o", exe])
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe]).decode().splitlines() if line.strip()]
    his = (_bound("NT_DEV_MAX_FIXED"), _bound("NT_DEV_MAX_FIXED_BOX"))
    assert his == (10, 24)
    seen = {hi: set() for hi in his}
    for hi, n, in_range, r, total, of_n in rows:
        seen[hi].add(n)
        if 3 <= n <= hi:
            assert (in_range, r, total, of_n) == (1, 1000 + n, 1, 1), (hi, n, in_range, r, total, of_n)
        else:
            assert (in_range, r, total) == (0, -77, 0), (hi, n, in_range, r, total)       # nothing called, r as it was
    for hi in his:
        assert set(range(3, hi + 1)) | {0, 2, hi + 1, 64, -1} <= seen[hi]


def _symbols(*flags):
    """((launcher template, N) of every launcher of build.FAMILIES in the listing, the listing)"""
    out = subprocess.check_output(["nm", "-D", "-C"] + list(flags) + [_lib.LIB_PATH]).decode()
    names = "|".join(re.escape(name) for name in build.launcher_dims())
    return [(name, int(n)) for name, n in re.findall(r"\b(%s)<(\d+)>\(" % names, out)], out


def test_no_launcher_of_a_dimension_is_left_undefined():
    """a shared library links with an explicit specialisation missing and fails when that dimension is first called: this
    stands in for the link error"""
    bad, out = _symbols("--undefined-only")
    assert not bad, bad
    assert "hipLaunchKernel" in out                      # (the listing is the library's)


def test_every_family_exports_the_dimensions_the_build_compiles():
    sources = {src: box for src, _, box in build.FAMILIES}
    assert len(sources) == len(build.FAMILIES)
    his = {False: _bound("NT_DEV_MAX_FIXED"), True: _bound("NT_DEV_MAX_FIXED_BOX")}
    # what the build compiles is what the dispatch can call: a unit for 3 .. the bound of its family, each once, and no
    # unit of a dimension that the table does not explain
    compiled = {}
    for name, src, flags in build.units():
        ns = [int(f.split("=")[1]) for f in flags if f.startswith("-DNT_INST_N=")]
        if ns and ns[0] > 0:
            assert src in sources and len(ns) == 1, (name, src, flags)
            compiled.setdefault(src, []).append(ns[0])
    assert set(compiled) == set(sources)
    for src, dims in compiled.items():
        assert sorted(dims) == list(range(3, his[sources[src]] + 1)), (src, sorted(dims))
    # every launcher is defined for 3 .. one of the two bounds, and some launcher of a unit for every dimension the unit is compiled for
    # (CompositeScene's stop at NT_DEV_MAX_FIXED where they share a unit with BoxScene's)
    want = build.launcher_dims()
    assert sorted(want) == sorted(name for _, names, _ in build.FAMILIES for name in names)
    # (the table names every launcher template the dispatch header declares)
    declared = re.findall(r"^template <int N> int (nt_\w+)\(", open(os.path.join(CSRC, "nt_dispatch.hpp")).read(), re.M)
    assert sorted(declared) == sorted(want) and len(declared) == len(set(declared))
    for src, names, box in build.FAMILIES:
        for name in names:
            assert list(want[name]) == list(range(3, want[name][-1] + 1)) and want[name][-1] in his.values(), (name, want[name])
        assert max(want[name][-1] for name in names) == his[box], src
    got = {}
    for name, n in _symbols("--defined-only")[0]:
        got.setdefault(name, []).append(n)
    assert {f: sorted(d) for f, d in got.items()} == {f: sorted(d) for f, d in want.items()}
    # and every unit is a source that exists, with the one guard against a build without the dimension
    for src in sources:
        assert '#ifndef NT_INST_N\n#error' in open(os.path.join(CSRC, src)).read(), src


@pytest.mark.parametrize("n", range(3, 25))
def test_box_cases_of_the_sweep_are_not_vacuous(n):
    dc.check_box(n)


@pytest.mark.parametrize("n", range(3, 11))
def test_composite_cases_of_the_sweep_are_not_vacuous(n):
    dc.check_composite(n)
