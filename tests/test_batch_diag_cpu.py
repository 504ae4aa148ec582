"""Host side of the batch diagnostics (nbody_batch_diagnostics, nbody_batch_diag_*, StepperBatch.diagnostics and the
recorded series): everything that needs no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nbody_batch_diagnostics", "nbody_batch_diag_reserve", "nbody_batch_diag_record", "nbody_batch_diag_read")
INVALID = -1


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", nb.LIB_PATH], capture_output=True, check=True).stdout.decode()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in nb.SYMBOLS and getattr(nb.lib, name).restype is ctypes.c_int, name
    assert nb.lib.nbody_abi_version() == 2


def test_null_arguments_are_invalid_without_a_device(nb):
    L = nb.lib
    out = (nb.Diag * 4)()
    n = ctypes.c_int(-5)
    calls = {
        "diagnostics(NULL batch)": lambda: L.nbody_batch_diagnostics(None, out, None),
        "diagnostics(NULL batch, NULL out)": lambda: L.nbody_batch_diagnostics(None, None, None),
        "reserve(NULL batch)": lambda: L.nbody_batch_diag_reserve(None, 8),
        "record(NULL batch)": lambda: L.nbody_batch_diag_record(None),
        "read(NULL batch)": lambda: L.nbody_batch_diag_read(None, ctypes.addressof(out), 4, ctypes.byref(n)),
        "read(NULL batch, NULL out)": lambda: L.nbody_batch_diag_read(None, None, 4, ctypes.byref(n)),
        "read(NULL batch, NULL n_samples)": lambda: L.nbody_batch_diag_read(None, ctypes.addressof(out), 4, None),
    }
    for what, call in calls.items():
        L.nbody_batch_sync(None)                               # leaves another message behind
        before = L.nbody_last_error_string()
        assert call() == INVALID, what
        msg = L.nbody_last_error_string()
        assert msg and msg != before and b"nbody_batch_diag" in msg, (what, msg)
    assert n.value == -5                                       # nothing was stored


def test_stepper_batch_has_the_methods(nb):
    for name in ("diagnostics", "reserve_diagnostics", "record_diagnostics", "diagnostics_log"):
        assert callable(getattr(nb.StepperBatch, name)), name
    import inspect
    sig = inspect.signature(nb.StepperBatch.step)
    assert sig.parameters["record_every"].default == 0 and sig.parameters["nsteps"].default == 1
    assert inspect.signature(nb.StepperBatch.diagnostics).parameters["potential"].default is False


def test_log_dtype_mirrors_nbody_diag(nb):
    """The record of the series is struct nbody_diag itself: three int64 and eight doubles, 88 bytes, the size the C
    compiler gives the header's struct (tests/test_diagnostics_cpu.py) and the offsets of the ctypes mirror."""
    dt = nb.DIAG_DTYPE
    assert dt.itemsize == ctypes.sizeof(nb.Diag) == 88
    assert dt.names == tuple(name for name, _ in nb.Diag._fields_)
    for name, _ in nb.Diag._fields_:
        assert dt.fields[name][1] == getattr(nb.Diag, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(nb.Diag, name).size, name
    assert [dt.fields[k][0].base for k in dt.names[:3]] == [np.dtype(np.int64)] * 3
    assert all(dt.fields[k][0].base == np.dtype(np.float64) for k in dt.names[3:])
    assert dt.fields["momentum"][0].shape == (2,) and dt.fields["center_of_mass"][0].shape == (2,)
    # a ctypes record read through the dtype gives the same values
    d = nb.Diag()
    d.step, d.n_bodies, d.coincident_pairs, d.mass, d.potential = 7, 1000, 12, 3.5, -2.25
    d.momentum[1], d.center_of_mass[0] = 0.5, -8.0
    r = np.frombuffer(bytes(d), dtype=dt)[0]
    assert (r["step"], r["n_bodies"], r["coincident_pairs"], r["mass"], r["potential"]) == (7, 1000, 12, 3.5, -2.25)
    assert r["momentum"][1] == 0.5 and r["center_of_mass"][0] == -8.0


def test_record_every_must_not_be_negative(nb):
    import pytest
    b = nb.StepperBatch.__new__(nb.StepperBatch)               # no device: the argument is judged before any call
    b._b = None
    with pytest.raises(ValueError):
        b.step(3, record_every=-1)
