"""The model of body identities (NBODY_FLAG_TRACK_IDS), in numpy on the CPU oracle, and the runs the identity tests use.

The identity of a body is its index in the upload.  Every step ends with a stable compaction on `mass != 0`, so the model
is one line per step: keep = M_pre != 0 on the oracle's pre-compaction block, ids = ids[keep].  Next to the map of every
step it returns the oracle's E_t (absorb pairs) and D_t (deleted indices), both in the index space of step t - what the
library's lineage must say once it is read through the map of that step.  Nothing here touches the product's device code.
"""
import numpy as np

import oracle_lib as ol

SEED = 7003
STEPS = 8
FIELD_OF = {77: 1000, 130: 1500, 300: 2000, 1000: 5000, 1024: 5000, 1500: 6000}   # the table of test_gpu_batch.py
DENSE_N0 = (300, 1000, 1500)
# bodies after 8 steps of the dense runs (seed 7003), counted on the CPU oracle; fp64 gives the same counts
SURVIVORS = {(300, ol.LITERAL): 138, (1000, ol.LITERAL): 332, (1500, ol.LITERAL): 441,
             (300, ol.CLEAN): 29, (1000, ol.CLEAN): 267, (1500, ol.CLEAN): 361}


def dense_cfg(nb, n0, **kw):
    return nb.stock_config(particleCount=n0, fieldWidth=FIELD_OF[n0], fieldHeight=FIELD_OF[n0], **kw)


def dense_bodies(nb, n0, precision=0, seed=SEED):
    cfg = dense_cfg(nb, n0)
    return cfg, nb.init_bodies(cfg, precision, seed=seed)


class ModelStep:
    """One step of the model: `ids` is the map of step t (ids[i] = identity of the body at index i BEFORE the step),
    `keep` the survivors' mask over those indices, E / D the oracle's events in that index space."""

    def __init__(self, ids, keep, E, D, n_after):
        self.ids, self.keep, self.E, self.D, self.n_after = ids, keep, E, D, n_after

    def absorb_ids(self):
        return sorted((int(self.ids[i]), int(self.ids[j])) for i, j in self.E)

    def deleted_ids(self):
        return sorted(int(self.ids[d]) for d in self.D)


def model_run(block, n, cfg, semantics=ol.LITERAL, steps=STEPS):
    """Steps a copy of `block` (float32 or float64, reference layout, n bodies) with the oracle.
    Returns ([ModelStep per step], final ids)."""
    blk = np.array(block[:6 * n], copy=True)
    real = blk.dtype.type
    ids = np.arange(n, dtype=np.int32)
    out = []
    for _ in range(steps):
        n2, _, ab, de, pre = ol.port_step(blk, n, real(np.float32(cfg.timestep)), cfg.fieldWidth, cfg.fieldHeight,
                                          real(np.float32(cfg.growthRate)), semantics=semantics, pre=True)
        keep = ol.carve(pre, n)[2] != 0                        # a NaN mass stays, a mass of 0 goes, event or not
        out.append(ModelStep(ids.copy(), keep, np.array(ab, copy=True), np.array(de, copy=True), n2))
        ids = ids[keep]
        n = n2
    return out, ids


def model_of_bodies(bodies, cfg, semantics=ol.LITERAL, steps=STEPS):
    return model_run(bodies.contiguousData, bodies.numBodies, cfg, semantics, steps)


def lineage_sets(lin, step):
    """(kind-0 records as sorted (id_i, id_j) pairs, kind-1 records as sorted (id_i, id_j) pairs) of one step."""
    lin = lin[lin["step"] == step]
    return (sorted((int(e["id_i"]), int(e["id_j"])) for e in lin[lin["kind"] == 0]),
            sorted((int(e["id_i"]), int(e["id_j"])) for e in lin[lin["kind"] == 1]))


def absorb_lines(model):
    """The kind-0 lines `step kind id_i id_j` of the model, in the order nbody --lineage writes them."""
    rows = sorted((t, 0, a, b) for t, m in enumerate(model) for a, b in m.absorb_ids())
    return ["%d %d %d %d" % r for r in rows]
