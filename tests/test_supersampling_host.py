"""The supersampling factor as a scene attribute (nt_scene_set_supersampling / scene.set_supersampling), without a GPU:
default, round trips through the ABI and through Python, refused values, the lock, pickling and with_rebuilt_tree()."""
import pickle

import numpy as np
import pytest

import fixtures as fx
from ntracer_amd import _lib, tracern


def box():
    return tracern.BoxScene(5)


def composite():
    return tracern.CompositeScene.from_flat(4, fx.flat_of(fx.load("cell600_n4")))


SCENES = [box, composite]


@pytest.mark.parametrize("make", SCENES)
def test_the_default_factor_is_one(make):
    sc = make()
    assert sc.supersampling == 1
    assert _lib.lib().nt_scene_get_supersampling(sc._handle) == 1


@pytest.mark.parametrize("make", SCENES)
def test_set_and_get_round_trip_through_the_abi_and_python(make):
    sc = make()
    L = _lib.lib()
    for s in (1, 2, 3, 4, 5, 6, 7, 8, 1):
        assert L.nt_scene_set_supersampling(sc._handle, s) == _lib.NT_OK
        assert L.nt_scene_get_supersampling(sc._handle) == s and sc.supersampling == s
    for s in (8, 2, np.int32(3), 1):
        sc.set_supersampling(s)
        assert sc.supersampling == int(s) and L.nt_scene_get_supersampling(sc._handle) == int(s)
    with pytest.raises(AttributeError):
        sc.supersampling = 2                                  # read-only, like fov


@pytest.mark.parametrize("make", SCENES)
def test_bad_factors_are_refused_and_leave_the_factor_unchanged(make):
    sc = make()
    sc.set_supersampling(3)
    L = _lib.lib()
    for bad in (0, -1, 9, 1 << 20):
        assert L.nt_scene_set_supersampling(sc._handle, bad) == _lib.NT_E_INVALID
        assert "between 1 and 8" in _lib.last_error()
        assert L.nt_scene_get_supersampling(sc._handle) == 3
        with pytest.raises(ValueError):
            sc.set_supersampling(bad)
        assert sc.supersampling == 3
    for bad in (2.0, 2.5, "2", None, True):
        with pytest.raises(ValueError):
            sc.set_supersampling(bad)
        assert sc.supersampling == 3
    assert L.nt_scene_set_supersampling(None, 2) == _lib.NT_E_INVALID
    assert L.nt_scene_get_supersampling(None) == _lib.NT_E_INVALID


@pytest.mark.parametrize("make", SCENES)
def test_a_locked_scene_refuses(make):
    sc = make()
    L = _lib.lib()
    sc.set_supersampling(2)
    assert L.nt_scene_lock(sc._handle) == _lib.NT_OK
    try:
        assert L.nt_scene_set_supersampling(sc._handle, 4) == _lib.NT_E_LOCKED
        with pytest.raises(_lib.LockedError):
            sc.set_supersampling(4)
        assert sc.supersampling == 2
    finally:
        assert L.nt_scene_unlock(sc._handle) == _lib.NT_OK
    sc.set_supersampling(4)
    assert sc.supersampling == 4


@pytest.mark.parametrize("make", SCENES)
def test_the_scratch_cap_round_trips_and_refuses_bad_values(make):
    sc = make()
    L = _lib.lib()
    assert sc.supersampling_scratch_mb == 1024 and L.nt_scene_get_supersampling_scratch_mb(sc._handle) == 1024
    for mib in (1, 4, 8192, 1 << 20):
        sc.set_supersampling_scratch_mb(mib)
        assert sc.supersampling_scratch_mb == mib and L.nt_scene_get_supersampling_scratch_mb(sc._handle) == mib
    sc.set_supersampling_scratch_mb(64)
    for bad in (0, -1, (1 << 20) + 1):
        assert L.nt_scene_set_supersampling_scratch_mb(sc._handle, bad) == _lib.NT_E_INVALID
        with pytest.raises(ValueError):
            sc.set_supersampling_scratch_mb(bad)
    for bad in (2.0, "2", None, True):
        with pytest.raises(ValueError):
            sc.set_supersampling_scratch_mb(bad)
    assert sc.supersampling_scratch_mb == 64 and sc.supersampling == 1
    assert L.nt_scene_lock(sc._handle) == _lib.NT_OK
    try:
        with pytest.raises(_lib.LockedError):
            sc.set_supersampling_scratch_mb(128)
    finally:
        assert L.nt_scene_unlock(sc._handle) == _lib.NT_OK
    assert sc.supersampling_scratch_mb == 64
    assert L.nt_scene_set_supersampling_scratch_mb(None, 2) == _lib.NT_E_INVALID
    assert L.nt_scene_get_supersampling_scratch_mb(None) == _lib.NT_E_INVALID


def test_the_factor_is_no_part_of_what_is_pickled():
    """The wire format is the reference's, which has no such setting, and scene objects have no reduce of their own (nor have
    the reference's): the factor lives in the native handle, like fov, so what pickle sees of a scene's Python state is the
    same bytes whatever the factor, and a scene made afresh -- which is what loading a scene's pickled contents comes to --
    starts at 1."""
    for make in SCENES:
        sc = make()
        state = {k: v for k, v in sc.__dict__.items() if k != "_handle"}
        before = pickle.dumps(state, 2)
        sc.set_supersampling(4)
        assert pickle.dumps({k: v for k, v in sc.__dict__.items() if k != "_handle"}, 2) == before
        assert not any("supersampling" in k for k in sc.__dict__)
        assert make().supersampling == 1


def test_with_rebuilt_tree_carries_the_factor_over():
    sc = composite()
    sc.set_fov(0.7)
    sc.set_supersampling(3)
    sc.set_supersampling_scratch_mb(96)
    other = sc.with_rebuilt_tree()
    assert other.supersampling == 3 and other.supersampling_scratch_mb == 96 and abs(other.fov - 0.7) < 1e-7
    assert sc.supersampling == 3
    assert composite().with_rebuilt_tree().supersampling == 1
