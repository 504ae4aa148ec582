"""Tracer particles without a device: the properties of the model (tracer_cases.advance), the records of the binding, the
argument errors every *_tracers_* symbol finds before any device call, and the wrapper's shape checks."""
import ctypes
import types

import numpy as np
import pytest

import tracer_cases as tc

INVALID = -1
NEW_SYMBOLS = ("nbody_tracers_set", "nbody_tracers_get", "nbody_batch_tracers_set", "nbody_batch_tracers_get")
FIELD = (100, 50)


def test_wall_flip_only_with_the_flag_and_only_by_the_acceleration_test():
    dt = 0.5
    # 0: x + ax dt crosses +W although v points inwards; 1: v would carry it across, ax dt does not; 2: already outside;
    # 3: y + ay dt crosses -H; 4: well inside
    pos = np.array([[99.0, 0.0], [99.0, 0.0], [101.0, 0.0], [0.0, -49.0], [10.0, 10.0]])
    vel = np.array([[-3.0, 1.0], [30.0, 1.0], [2.0, 1.0], [1.0, 4.0], [7.0, -7.0]])
    acc = np.array([[4.0, 0.0], [0.5, 0.0], [0.0, 0.0], [0.0, -4.0], [1.0, 1.0]])
    tr = {"pos": pos, "vel": vel}
    free = tc.advance(tr, acc, dt, False, FIELD)
    wall = tc.advance(tr, acc, dt, True, FIELD)
    assert tc.same_bits(free["vel"], vel + dt * acc) and tc.same_bits(free["pos"], pos + dt * (vel + dt * acc))
    flipped = vel.copy()
    flipped[0, 0], flipped[2, 0], flipped[3, 1] = 3.0, -2.0, -4.0
    assert tc.same_bits(wall["vel"], flipped + dt * acc)
    assert tc.same_bits(wall["pos"], pos + dt * (flipped + dt * acc))
    assert tc.same_bits(wall["vel"][[1, 4]], free["vel"][[1, 4]])   # v alone never flips: the test is on ax dt
    assert tr["pos"] is pos and tc.same_bits(pos[0], [99.0, 0.0])   # the input is left alone


def test_mirror_symmetry_about_a_source():
    P, M = np.array([[0.0, 0.0]]), np.array([3.0e9])
    a = np.array([[3.25, -1.5], [0.7, 11.0]])
    tr = {"pos": np.concatenate([a, -a]), "vel": np.concatenate([[[0.3, -0.2], [0.0, 1.0]], [[-0.3, 0.2], [-0.0, -1.0]]])}
    for _ in range(4):
        tr = tc.advance(tr, tc.point_field(P, M, tr["pos"]), 0.2, True, FIELD)
        assert tc.same_bits(tr["pos"][:2], -tr["pos"][2:]) and tc.same_bits(tr["vel"][:2], -tr["vel"][2:])
    assert not tc.same_bits(tr["vel"][:2], [[0.3, -0.2], [0.0, 1.0]])   # the source did pull


def test_empty_system_is_pure_drift():
    pos, vel = np.array([[1.5, -2.0], [1e200, 3.0]]), np.array([[0.25, 4.0], [-1.0, 0.0]])
    out = tc.advance({"pos": pos, "vel": vel}, tc.point_field(np.zeros((0, 2)), np.zeros(0), pos), 0.2, False, FIELD)
    assert tc.same_bits(out["vel"], vel) and tc.same_bits(out["pos"], pos + np.float64(0.2) * vel)


def test_nan_stays_in_its_tracer():
    P, M = np.array([[1.0, 2.0], [-4.0, 0.5]]), np.array([2.0e9, 5.0e8])
    pos = np.array([[0.0, 0.0], [np.nan, 1.0], [3.0, 3.0], [np.inf, -np.inf], [-2.0, 8.0]])
    vel = np.ones((5, 2))
    keep = [0, 2, 4]
    for walls in (False, True):
        full = tc.advance({"pos": pos, "vel": vel}, tc.point_field(P, M, pos), 0.2, walls, FIELD)
        part = tc.advance({"pos": pos[keep], "vel": vel[keep]}, tc.point_field(P, M, pos[keep]), 0.2, walls, FIELD)
        assert tc.same_bits(full["pos"][keep], part["pos"]) and tc.same_bits(full["vel"][keep], part["vel"])
        assert np.isfinite(part["pos"]).all() and np.isnan(full["pos"][1, 0])


def test_records_of_the_binding(nb):
    assert nb.TRACER_DTYPE.itemsize == 32
    assert [nb.TRACER_DTYPE.fields[k][1] for k in ("pos", "vel")] == [0, 16]
    assert nb.TRACER_INFO_DTYPE.itemsize == 24
    assert [nb.TRACER_INFO_DTYPE.fields[k][1] for k in ("steps", "coincident", "count", "flags")] == [0, 8, 16, 20]
    assert nb.TRACER_WALLS == 1
    for name in NEW_SYMBOLS:
        assert name in nb.SYMBOLS and getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
        assert getattr(nb.lib, name).restype is ctypes.c_int


def test_null_handles_are_invalid_and_say_so(nb):
    rec = np.zeros(4, dtype=nb.TRACER_DTYPE)
    last = np.zeros(4, dtype=nb.FIELD_DTYPE)
    info = np.zeros(4, dtype=nb.TRACER_INFO_DTYPE)
    calls = {"nbody_tracers_set": (None, rec.ctypes.data, 4, 0),
             "nbody_tracers_get": (None, rec.ctypes.data, last.ctypes.data, 4, info.ctypes.data),
             "nbody_batch_tracers_set": (None, rec.ctypes.data, 4, 0),
             "nbody_batch_tracers_get": (None, rec.ctypes.data, last.ctypes.data, info.ctypes.data)}
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(nb.lib, name)(*args) == INVALID, name
        msg = nb.lib.nbody_last_error_string().decode()
        assert name in msg and "NULL" in msg, (name, msg)
    assert not rec.view(np.uint8).any() and not info.view(np.uint8).any()


def test_wrapper_checks_shapes_before_the_library(nb):
    one = types.SimpleNamespace(_ctx=None)
    batch = types.SimpleNamespace(_b=None, systems=3)
    for bad in (np.zeros(4), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((0,))):
        with pytest.raises(ValueError):
            nb.Stepper.set_tracers(one, bad)
    with pytest.raises(ValueError):
        nb.Stepper.set_tracers(one, np.zeros((4, 2)), vel=np.zeros((5, 2)))
    for bad in (np.zeros(4), np.zeros((4, 3)), np.zeros((2, 4, 2)), np.zeros((3, 4, 2, 1))):
        with pytest.raises(ValueError):
            nb.StepperBatch.set_tracers(batch, bad)
    with pytest.raises(ValueError):
        nb.StepperBatch.set_tracers(batch, np.zeros((3, 4, 2)), vel=np.zeros((5, 2)))
    rec = nb._tracer_records(np.arange(8.0).reshape(4, 2), None, systems=3)          # (m, 2): given to every system
    assert rec.shape == (3, 4) and rec.dtype == nb.TRACER_DTYPE and rec.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(rec["pos"][s], np.arange(8.0).reshape(4, 2)) for s in range(3)) and not rec["vel"].any()
