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

# the families each instantiation unit defines; the CompositeScene ones stop at NT_DEV_MAX_FIXED where a unit is compiled beyond it
FAMILIES = {"nt_inst_box.hip": ("box",), "nt_inst_composite.hip": ("composite",), "nt_inst_query.hip": ("query",),
            "nt_inst_hits.hip": ("hits",), "nt_inst_rays.hip": ("rays_box", "rays"), "nt_inst_adaptive.hip": ("refine_box", "refine"),
            "nt_inst_lens.hip": ("lens",), "nt_inst_parallel.hip": ("parallel",), "nt_inst_ao.hip": ("ao",),
            "nt_inst_outline.hip": ("outline",)}
BOX_FAMILIES = ("box", "rays_box", "refine_box")


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
    out = subprocess.check_output(["nm", "-D", "-C"] + list(flags) + [_lib.LIB_PATH]).decode()
    return re.findall(r"\bnt_(\w+)_fixed<(\d+)>\(", out), out


def test_no_launcher_of_a_dimension_is_left_undefined():
    """a shared library links with an explicit specialisation missing and fails when that dimension is first called: this
    stands in for the link error"""
    _, out = _symbols("--undefined-only")
    bad = [line for line in out.splitlines() if "_fixed<" in line]
    assert not bad, bad
    assert "hipLaunchKernel" in out                      # (the listing is the library's)


def test_every_family_exports_the_dimensions_the_build_compiles():
    want = {}
    for _, src, flags in build.units():
        for fam in FAMILIES.get(src, ()):
            (n,) = [int(f.split("=")[1]) for f in flags if f.startswith("-DNT_INST_N=")]
            if fam in BOX_FAMILIES or n <= _bound("NT_DEV_MAX_FIXED"):
                want.setdefault(fam, []).append(n)
    assert set(want) == {f for fams in FAMILIES.values() for f in fams}
    # what the build compiles is what the dispatch can call: 3 .. the bound of the family, each once
    for fam, dims in want.items():
        hi = _bound("NT_DEV_MAX_FIXED_BOX" if fam in BOX_FAMILIES else "NT_DEV_MAX_FIXED")
        assert sorted(dims) == list(range(3, hi + 1)), (fam, sorted(dims))
    got = {}
    for fam, n in _symbols("--defined-only")[0]:
        got.setdefault(fam, []).append(int(n))
    assert {f: sorted(d) for f, d in got.items()} == {f: sorted(d) for f, d in want.items()}
    # and every unit is a source that exists, with the one guard against a build without the dimension
    for src in FAMILIES:
        assert '#ifndef NT_INST_N\n#error' in open(os.path.join(CSRC, src)).read(), src


@pytest.mark.parametrize("n", range(3, 25))
def test_box_cases_of_the_sweep_are_not_vacuous(n):
    dc.check_box(n)


@pytest.mark.parametrize("n", range(3, 11))
def test_composite_cases_of_the_sweep_are_not_vacuous(n):
    dc.check_composite(n)
