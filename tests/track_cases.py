"""The model of the track log (nbody_track_*, nbody_batch_track_*), in numpy on the CPU oracle.

Column c of a row stands for body IDENTITY sel[c] (its index in the upload).  The model steps the oracle as
lineage_cases.model_run does, keeps the block and the map after every step, and builds the tables a log must hold when a
row is recorded before the first step and after every `every`-th step: rows (step, n_bodies), index (where the identity is
now, -1: gone) and the six fields {x, y, vx, vy, m, r} (all-zero bytes where gone).  Nothing here touches the product's
device code.
"""
import functools

import numpy as np

import lineage_cases as lc
import oracle_lib as ol

FIELDS = ("x", "y", "vx", "vy", "m", "r")


class Tables:
    """step, n_bodies: int64[rows]; index: int32[rows, columns]; rec: {field: real[rows, columns]}; sel: the identities."""

    def __init__(self, sel, step, n_bodies, index, rec, states):
        self.sel, self.step, self.n_bodies, self.index, self.rec, self.states = sel, step, n_bodies, index, rec, states

    def columns(self, sel):
        """The table of a selection of identities (each either a column of this table, or one that never existed)."""
        sel = np.asarray(sel, dtype=np.int64)
        have = sel < len(self.sel)
        src = np.where(have, sel, 0)
        index = np.where(have[None, :], self.index[:, src], -1).astype(np.int32)
        rec = {f: np.where(have[None, :], self.rec[f][:, src], 0).astype(self.rec[f].dtype) for f in FIELDS}
        return Tables(sel, self.step, self.n_bodies, index, rec, self.states)

    def every(self, k):
        """Row 0 and the rows after every k-th step."""
        rows = [0] + [t for t in range(1, len(self.step)) if t % k == 0]
        return Tables(self.sel, self.step[rows], self.n_bodies[rows], self.index[rows],
                      {f: self.rec[f][rows] for f in FIELDS}, [self.states[t] for t in rows])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def row_of(block, n, ids, n0):
    """One row over all n0 identities from a block of n bodies whose identities are ids[0..n)."""
    P, V, M, R = ol.carve(block, n)
    index = np.full(n0, -1, dtype=np.int32)
    index[ids] = np.arange(n, dtype=np.int32)
    rec = {f: np.zeros(n0, dtype=block.dtype) for f in FIELDS}
    for f, src in (("x", P[:, 0]), ("y", P[:, 1]), ("vx", V[:, 0]), ("vy", V[:, 1]), ("m", M), ("r", R)):
        rec[f][ids] = src
    return index, rec


def model_tables(block, n0, cfg, semantics=ol.LITERAL, steps=lc.STEPS):
    """All-columns tables of `steps` oracle steps of a copy of block (row t = the state after t steps), with the state
    (block, n, ids) of every row kept in .states."""
    blk = np.array(block[:6 * n0], copy=True)
    real = blk.dtype.type
    ids = np.arange(n0, dtype=np.int32)
    n = n0
    rows, states = [], []
    for t in range(steps + 1):
        if t > 0:
            n2, _, _, _, pre = ol.port_step(blk, n, real(np.float32(cfg.timestep)), cfg.fieldWidth, cfg.fieldHeight,
                                            real(np.float32(cfg.growthRate)), semantics=semantics, pre=True)
            ids = ids[ol.carve(pre, n)[2] != 0]                 # the compaction's keep test, as lineage_cases.model_run
            n = n2
            assert len(ids) == n
        rows.append(row_of(blk, n, ids, n0))
        states.append((blk[:6 * n].copy(), n, ids.copy()))
    return Tables(np.arange(n0), np.arange(steps + 1, dtype=np.int64), np.array([s[1] for s in states], dtype=np.int64),
                  np.stack([r[0] for r in rows]), {f: np.stack([r[1][f] for r in rows]) for f in FIELDS}, states)


@functools.lru_cache(maxsize=None)
def dense_tables(nb, n0, precision=0, semantics=ol.LITERAL):
    """The dense runs of lineage_cases (seed 7003, 8 steps), computed once per session and never changed."""
    cfg, bodies = lc.dense_bodies(nb, n0, precision)
    return cfg, bodies, model_tables(bodies.contiguousData, n0, cfg, semantics)


def selection_of(tab, n0):
    """The selection of the issue, chosen from the model: identity 0, n0-1, one deleted in step 0, the last one absorbed,
    the first and the last survivor, one identity >= n0."""
    present = tab.index >= 0
    gone_at = np.where(present.all(axis=0), len(tab.step), np.argmin(present, axis=0))   # first row without it
    first_step = np.nonzero(gone_at == 1)[0]
    assert len(first_step) > 0
    last_gone = np.nonzero(gone_at == gone_at[gone_at < len(tab.step)].max())[0]
    survivors = np.nonzero(present[-1])[0]
    sel = {0, n0 - 1, int(first_step[len(first_step) // 2]), int(last_gone[-1]), int(survivors[0]), int(survivors[-1]),
           n0 + 5}
    return np.array(sorted(sel), dtype=np.int32)


def assert_tables_equal(got, want, what):
    """got: the dict of Stepper.tracks() (or one system of StepperBatch.tracks()); want: Tables.  Bitwise."""
    assert np.array_equal(got["step"], want.step), what
    assert np.array_equal(got["n_bodies"], want.n_bodies), what
    assert got["index"].dtype == np.int32 and got["index"].shape == want.index.shape, (what, got["index"].shape)
    assert np.array_equal(got["index"], want.index), what
    for f in FIELDS:
        assert got[f].dtype == want.rec[f].dtype, (what, f)
        assert np.array_equal(bits(got[f]), bits(want.rec[f])), (what, f)
