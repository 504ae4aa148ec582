"""Body identities without a GPU: the model the GPU tests compare against (tests/lineage_cases.py) on the CPU oracle,
and the host side of NBODY_FLAG_TRACK_IDS - symbols, argument errors, and the flag rules, all of which must be decided
before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import lineage_cases as lc
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -5
NEW_SYMBOLS = ("nbody_get_ids", "nbody_get_lineage", "nbody_batch_get_ids", "nbody_batch_get_lineage")


# ---------------------------------------------------------------------------------------------------------
# the model on the oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("semantics", [ol.LITERAL, ol.CLEAN], ids=["literal", "clean"])
@pytest.mark.parametrize("n0", lc.DENSE_N0)
def test_model_on_the_dense_runs(nb, n0, semantics, precision):
    cfg, bodies = lc.dense_bodies(nb, n0, precision)
    model, final = lc.model_of_bodies(bodies, cfg, semantics)
    n = n0
    for t, m in enumerate(model):
        assert len(m.ids) == n and len(m.keep) == n
        assert m.n_after == int(m.keep.sum()), t                # survivor count = what the keep mask says
        assert np.all(np.diff(m.ids) > 0), t                    # stable compaction: identities strictly increasing
        assert not m.keep[m.D].any(), t                         # every deleted index is dropped
        assert len(set(int(d) for d in m.D)) == len(m.D), t
        assert int((~m.keep).sum()) == len(m.D), t              # and nothing else is (no zero masses in these runs)
        n = m.n_after
    assert len(final) == n and np.all(np.diff(final) > 0)
    # non-vacuity, as a condition: at least half of the bodies are deleted and no survivor keeps its index
    assert n == lc.SURVIVORS[(n0, semantics)]
    assert n0 - n >= n0 / 2
    assert np.all(final != np.arange(n))


def _with_special_masses(nb):
    cfg, bodies = lc.dense_bodies(nb, 300)
    for z in (5, 40, 299):                                      # uploaded with mass 0: gone at the first compaction;
        bodies.Masses[z] = 0.0                                  # far from everybody and without a radius, so that no
        bodies.Radii[z] = 0.0                                   # collision involves them: they leave with NO event
        bodies.Positions[z] = [1.0e6 + 10.0 * z, 1.0e6]
    bodies.Masses[17] = np.nan                                  # NaN != 0: stays
    return cfg, bodies


@pytest.mark.parametrize("semantics", [ol.LITERAL, ol.CLEAN], ids=["literal", "clean"])
def test_model_zero_mass_leaves_without_event_and_nan_stays(nb, semantics):
    cfg, bodies = _with_special_masses(nb)
    model, final = lc.model_of_bodies(bodies, cfg, semantics, steps=4)
    first = model[0]
    for z in (5, 40, 299):
        assert not first.keep[z]
        assert z not in set(int(d) for d in first.D)            # no D_t entry
        assert all(z != int(i) and z != int(j) for i, j in first.E)   # nor an absorb pair, on either side
        assert z not in model[1].ids
    dropped = set(np.nonzero(~first.keep)[0].tolist())
    assert dropped == set(int(d) for d in first.D) | {5, 40, 299}
    for m in model:
        assert 17 in m.ids                                      # the NaN mass is never compacted away
    assert 17 in final


# ---------------------------------------------------------------------------------------------------------
# host side
# ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared(nb):
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "%s is not declared in include/nbody.h" % name
        assert hasattr(raw, name), "library does not export %s" % name
        assert name in nb.SYMBOLS
    assert re.search(r"NBODY_FLAG_TRACK_IDS\s*=\s*1u\s*<<\s*3", code)
    assert re.search(r"typedef\s+struct\s+nbody_lineage\s*\{[^}]*step[^}]*id_i[^}]*id_j[^}]*kind[^}]*\}", code)
    assert nb.FLAG_TRACK_IDS == 8
    assert nb.LINEAGE_DTYPE.names == ("step", "id_i", "id_j", "kind") and nb.LINEAGE_DTYPE.itemsize == 16
    assert nb.lib.nbody_abi_version() == 2
    assert re.search(r"#define\s+NBODY_ABI_VERSION\s+2\b", code)


def test_null_and_negative_cap_are_invalid(nb):
    ids = (ctypes.c_int32 * 4)()
    rec = np.zeros(4, dtype=nb.LINEAGE_DTYPE)
    n, total = ctypes.c_int(0), ctypes.c_int64(0)
    assert nb.lib.nbody_get_ids(None, ids, 4, ctypes.byref(n)) == INVALID
    assert nb.lib.nbody_get_ids(None, ids, -1, ctypes.byref(n)) == INVALID
    assert nb.lib.nbody_get_ids(None, None, 4, None) == INVALID
    assert nb.lib.nbody_get_lineage(None, rec.ctypes.data, 4, ctypes.byref(total)) == INVALID
    assert nb.lib.nbody_get_lineage(None, rec.ctypes.data, -1, ctypes.byref(total)) == INVALID
    assert nb.lib.nbody_get_lineage(None, None, 4, None) == INVALID
    for system in (0, -1, 1 << 20):                             # no batch: every system number is out of range too
        assert nb.lib.nbody_batch_get_ids(None, system, ids, 4, ctypes.byref(n)) == INVALID
        assert nb.lib.nbody_batch_get_lineage(None, system, rec.ctypes.data, 4, ctypes.byref(total)) == INVALID
    assert nb.lib.nbody_last_error_string()


def _ctx_status(nb, **kw):
    d = nb._CtxDesc()
    cfg = nb.stock_config(particleCount=256)
    nb.lib.nbody_ctx_desc_from_config(ctypes.byref(d), ctypes.byref(cfg), nb.F32)
    d.device, d.rank, d.world, d.flags = 0, 0, 1, 0
    for k, v in kw.items():
        setattr(d, k, v)
    ctx = ctypes.c_void_p()
    rc = nb.lib.nbody_ctx_create(ctypes.byref(ctx), ctypes.byref(d))
    if rc == 0:
        nb.lib.nbody_ctx_destroy(ctx)
    return rc


@pytest.mark.parametrize("case", ["world-2", "world-2-rank-1", "group-exchange", "force-comm", "both-exchange-flags",
                                  "events-and-group"])
def test_track_ids_across_ranks_is_invalid_before_any_device_call(nb, case):
    """NBODY_ERR_INVALID, not NBODY_ERR_NO_DEVICE: found before the device is looked for."""
    T = nb.FLAG_TRACK_IDS
    kw = {"world-2": dict(world=2, flags=T), "world-2-rank-1": dict(world=2, rank=1, flags=T | nb.FLAG_GROUP_EXCHANGE),
          "group-exchange": dict(flags=T | nb.FLAG_GROUP_EXCHANGE), "force-comm": dict(flags=T | nb.FLAG_FORCE_COMM),
          "both-exchange-flags": dict(flags=T | nb.FLAG_GROUP_EXCHANGE | nb.FLAG_FORCE_COMM),
          "events-and-group": dict(world=2, flags=T | nb.FLAG_RECORD_EVENTS | nb.FLAG_GROUP_EXCHANGE)}[case]
    assert _ctx_status(nb, **kw) == INVALID
    assert b"NBODY_FLAG_TRACK_IDS" in nb.lib.nbody_last_error_string()


def test_stepper_group_with_track_ids_raises_invalid(nb):
    with pytest.raises(nb.NbodyError) as ei:
        nb.StepperGroup(2, cfg=nb.stock_config(particleCount=256), track_ids=True)
    assert ei.value.status == INVALID


@pytest.mark.parametrize("flags", [8, 9])
def test_track_ids_alone_is_a_valid_context_and_batch_descriptor(nb, flags):
    """The flag alone, and with NBODY_FLAG_RECORD_EVENTS, passes every argument check: what stops the call on a host
    without a GPU is the missing device."""
    d = nb._BatchDesc()
    d.precision, d.semantics, d.systems, d.capacity, d.device = nb.F32, nb.LITERAL, 4, 256, 0
    d.flags, d.event_capacity, d.kernel_variant = flags, 0, 0
    params = (nb._BatchParams * 4)()
    for p in params:
        p.timestep, p.growthRate, p.fieldWidth, p.fieldHeight = 0.2, 0.1, 100000, 100000
    b = ctypes.c_void_p()
    rc = nb.lib.nbody_batch_create(ctypes.byref(b), ctypes.byref(d), params)
    rc_ctx = _ctx_status(nb, flags=flags)
    if os.path.exists("/dev/kfd"):
        assert rc == 0 and rc_ctx == 0
        assert nb.lib.nbody_batch_destroy(b) == 0
    else:
        assert rc == NO_DEVICE and rc_ctx == NO_DEVICE
        assert not b.value


@pytest.mark.parametrize("flags", [8 | 2, 8 | 4, 8 | (1 << 9), 16])
def test_batch_still_refuses_other_flags(nb, flags):
    d = nb._BatchDesc()
    d.precision, d.semantics, d.systems, d.capacity, d.device, d.flags = nb.F32, nb.LITERAL, 4, 256, 0, flags
    params = (nb._BatchParams * 4)()
    b = ctypes.c_void_p()
    assert nb.lib.nbody_batch_create(ctypes.byref(b), ctypes.byref(d), params) == INVALID
