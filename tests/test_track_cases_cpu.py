"""The track log without a GPU: the model the GPU tests compare against (tests/track_cases.py) on the CPU oracle, and the
host side of nbody_track_* / nbody_batch_track_* - symbols, bindings and the NULL-handle rule."""
import ctypes
import os
import re

import numpy as np
import pytest

import lineage_cases as lc
import oracle_lib as ol
import track_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NEW_SYMBOLS = ("nbody_track_reserve", "nbody_track_record", "nbody_track_read", "nbody_batch_track_reserve",
               "nbody_batch_track_record", "nbody_batch_track_read")


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("semantics", [ol.LITERAL, ol.CLEAN], ids=["literal", "clean"])
@pytest.mark.parametrize("n0", lc.DENSE_N0)
def test_model_on_the_dense_runs(nb, n0, semantics, precision):
    cfg, bodies, tab = tc.dense_tables(nb, n0, precision, semantics)
    assert tab.index.shape == (lc.STEPS + 1, n0) and np.array_equal(tab.step, np.arange(lc.STEPS + 1))
    # row 0 is the upload: every identity at its own index, with the uploaded bits
    assert np.array_equal(tab.index[0], np.arange(n0))
    assert np.array_equal(tc.bits(tab.rec["m"][0]), tc.bits(bodies.Masses))
    assert np.array_equal(tc.bits(tab.rec["x"][0]), tc.bits(bodies.Positions[:, 0]))
    # the last row, read through `index`, is the oracle's final state
    blk = bodies.contiguousData[:6 * n0].copy()
    real = blk.dtype.type
    n = n0
    for _ in range(lc.STEPS):
        n, *_ = ol.port_step(blk, n, real(np.float32(cfg.timestep)), cfg.fieldWidth, cfg.fieldHeight,
                             real(np.float32(cfg.growthRate)), semantics=semantics, want_events=False)
    P, V, M, R = ol.carve(blk, n)
    last = tab.index[-1]
    here = np.nonzero(last >= 0)[0]
    assert len(here) == n == tab.n_bodies[-1] == lc.SURVIVORS[(n0, semantics)]
    assert np.array_equal(last[here], np.arange(n))             # survivors in identity order: the compaction is stable
    for f, src in (("x", P[:, 0]), ("y", P[:, 1]), ("vx", V[:, 0]), ("vy", V[:, 1]), ("m", M), ("r", R)):
        assert np.array_equal(tc.bits(tab.rec[f][-1][here]), tc.bits(src)), f
    # every row: the present columns count n_bodies, absent ones are all-zero bytes, an identity never comes back
    present = tab.index >= 0
    assert np.array_equal(present.sum(axis=1), tab.n_bodies)
    for f in tc.FIELDS:
        assert not tc.bits(tab.rec[f])[~present].any(), f
    assert not (present[1:] & ~present[:-1]).any()
    # non-vacuity, as conditions of the runs
    assert (~present[1:]).all(axis=0).any()                     # some identity is absent from row 1 on
    assert present.all(axis=0).any()                            # some identity is present in every row
    assert (~present[-1]).sum() >= n0 / 2                       # at least half are absent in the last row


@pytest.mark.parametrize("n0", lc.DENSE_N0)
def test_selection_and_stride_are_views_of_the_full_table(nb, n0):
    _, _, tab = tc.dense_tables(nb, n0)
    sel = tc.selection_of(tab, n0)
    assert np.all(np.diff(sel) > 0) and sel[0] == 0 and sel[-1] >= n0 and (n0 - 1) in sel
    sub = tab.columns(sel)
    assert sub.index.shape == (lc.STEPS + 1, len(sel))
    assert np.all(sub.index[:, -1] == -1) and not sub.rec["m"][:, -1].any()     # the identity that never existed
    for c, k in enumerate(sel[:-1]):
        assert np.array_equal(sub.index[:, c], tab.index[:, k])
    present = sub.index[:, :-1] >= 0
    assert present[0].all()
    assert (~present[1:]).all(axis=0).any() and present.all(axis=0).any()       # deleted in step 0; a survivor
    two = tab.every(2)
    assert np.array_equal(two.step, [0, 2, 4, 6, 8]) and np.array_equal(two.index, tab.index[::2])


def test_new_symbols_are_exported_declared_and_bound(nb):
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "%s is not declared in include/nbody.h" % name
        assert hasattr(raw, name), "library does not export %s" % name
        assert name in nb.SYMBOLS
    assert re.search(r"NBODY_TRACK_PHI\s*=\s*1u\s*<<\s*0", code)
    assert re.search(r"typedef\s+struct\s+nbody_track_f32\s*\{\s*float\s+x,\s*y,\s*vx,\s*vy,\s*m,\s*r;\s*\}", code)
    assert re.search(r"typedef\s+struct\s+nbody_track_f64\s*\{\s*double\s+x,\s*y,\s*vx,\s*vy,\s*m,\s*r;\s*\}", code)
    assert re.search(r"typedef\s+struct\s+nbody_track_row\s*\{\s*int64_t\s+step,\s*n_bodies;\s*\}", code)
    assert nb.TRACK_PHI == 1
    assert nb.TRACK_DTYPE[nb.F32].itemsize == 24 and nb.TRACK_DTYPE[nb.F64].itemsize == 48
    assert nb.TRACK_DTYPE[nb.F32].names == tc.FIELDS and nb.TRACK_ROW_DTYPE.itemsize == 16
    for cls in (nb.Stepper, nb.StepperBatch):
        for method in ("reserve_tracks", "record_tracks", "tracks"):
            assert callable(getattr(cls, method))
    assert nb.lib.nbody_abi_version() == 2
    assert re.search(r"#define\s+NBODY_ABI_VERSION\s+2\b", code)


def test_null_handle_is_invalid(nb):
    sel = (ctypes.c_int32 * 3)(0, 1, 2)
    n, cols = ctypes.c_int(0), ctypes.c_int(0)
    for reserve, record, read in ((nb.lib.nbody_track_reserve, nb.lib.nbody_track_record, nb.lib.nbody_track_read),
                                  (nb.lib.nbody_batch_track_reserve, nb.lib.nbody_batch_track_record,
                                   nb.lib.nbody_batch_track_read)):
        assert reserve(None, 4, None, 0, 0) == INVALID
        assert reserve(None, 4, sel, 3, nb.TRACK_PHI) == INVALID
        assert reserve(None, 0, None, 0, 0) == INVALID
        assert record(None) == INVALID
        assert read(None, None, None, None, None, 0, ctypes.byref(n), ctypes.byref(cols)) == INVALID
        assert read(None, None, None, None, None, 4, None, None) == INVALID
        assert nb.lib.nbody_last_error_string()
