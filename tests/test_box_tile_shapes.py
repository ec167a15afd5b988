"""The launch shapes of tests/test_box_tile_matrix.py, pinned to the C++ that decides them: tests/box_tile_geom_probe.cpp
prints nt_box_tile_geom (nt_device.hpp) for every row of fixtures.BOX_TILE_SHAPES, so a change of the block-shape rule
that would move a row off the shape it is there to cover fails here, without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

import fixtures as fx
from ntracer_amd import distributed as ntd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    """(label, width, row_count, frames, expected (rows, waves), expected split)"""
    out = [("%dx%dx%d" % (w, h, f), w, h, f, geom, split) for w, h, f, geom, split, _ in fx.BOX_TILE_SHAPES]
    w, h, f, rank, world, band_rows, geom, split = fx.BOX_TILE_BAND
    out.append(("band %d/%d" % (rank, world), w, len(ntd.owned_rows(h, rank, world, band_rows)), f, geom, split))
    return out


def test_box_tile_shapes_land_on_the_intended_block_shapes_and_splits(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "box_tile_geom_probe")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "ntracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "box_tile_geom_probe.cpp"), "-o", exe])
    rows = _rows()
    args = [str(v) for _, w, r, f, _, _ in rows for v in (w, r, f)]
    out = subprocess.check_output([exe] + args).decode().split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line.strip()]
    assert got == [geom for _, _, _, _, geom, _ in rows], list(zip([r[0] for r in rows], got))
    for label, w, r, f, _, split in rows:
        assert fx.box_redo_split(w, r, f) == split, label
    # every block shape box_tile_kernel is instantiated with, and both redo splits, are covered
    assert {geom for *_, geom, _ in rows} == {(8, 4), (16, 4), (16, 3), (64, 1)}
    assert {split for *_, split in rows} == {1, 2}
    # fixtures.box_redo_split restates launch_box_fixed's rule: it must still read that way
    src = open(os.path.join(ROOT, "ntracer_amd", "csrc", "nt_box.hpp")).read()
    assert re.search(r"rwords\s*=\s*\(long long\)tg\.row_count \* li\.nframes \* tg\.redo_words;", src)
    assert re.search(r"tg\.redo_words\s*=\s*\(\(tg\.width \+ 63\) / 64 \+ 31\) / 32;", src)
    assert re.search(r"int split\s*=\s*rwords < 48 \* 1024 \? 2 : 1;", src)
