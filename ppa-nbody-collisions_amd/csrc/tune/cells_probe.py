#!/usr/bin/env python3
"""Cost of the cell sums (nbody_get_cells, nbody_batch_get_cells): the five kernels of a call next to
render_discs - the O(n) kernel over the same records - and neighbors_at - the O(n^2) yardstick - timed in the same run on the
same state, and whole calls under the host clock.

    python3 csrc/tune/cells_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                        (a run of its own; nothing else is traced with it)
    python3 csrc/tune/cells_probe.py host [reps]        whole Stepper.cells() / StepperBatch.cells() calls under the host
                                                        clock, next to Stepper.neighbors() on the same state
    python3 csrc/tune/cells_probe.py report TRACE_DIR [HOST_LOG]
                                                        reads the kernel trace (csv) and prints the text of
                                                        profiles/cells_probe.txt

Shapes: N = 262144 fp32, the stock seeded state; grids of 256 x 256 and 1024 x 1024 over the field, moments and lists.  The
worst case: the same state shrunk (positions and radii) into one cell of the 8 x 8 grid over the field, so that every body is
a member of one segment - the counting sort walks n^2 index pairs and one wave adds all n terms.  A batch of 256 x 1024 on a
32 x 32 grid.  Before a time is taken every case is checked against the numpy model (tests/cell_cases.py)."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N = 262144, 256, 1024
ROUNDS = 3                                                   # what `report` expects of `kernels`
STAGES = ["cells_assign", "cells_scan", "cells_place", "cells_rank", "cells_sum"]
CASES = ["stock 256 x 256", "stock 1024 x 1024", "one cell of 8 x 8", "batch %d x %d, 32 x 32" % (BATCH_S, BATCH_N)]


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import cell_cases as cc

    def widen(b):
        return (np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Velocities, dtype=np.float64),
                np.asarray(b.Masses, dtype=np.float64))

    cfg = nb.stock_config(particleCount=N_ONE)
    bodies = nb.init_bodies(cfg)
    st = nb.Stepper(cfg)
    st.upload(bodies)
    P, V, M = widen(bodies)
    for nx in (256, 1024):
        got = st.cells(nx, lists=True)
        cc.assert_same(got, cc.model_cells(P, V, M, got["grid"]), "stock, %d x %d" % (nx, nx))
        count = got["cells"]["count"]
        print("# N=%d stock seeded state, %d x %d over the field: inside %d, occupied %d, largest %d, sum of s^2 %d (%.2f per "
              "body); equal to the model, lists included" % (N_ONE, nx, nx, got["info"]["inside"], got["info"]["occupied"],
                                                              got["info"]["largest"], int((count.astype(np.int64) ** 2).sum()),
                                                              float((count.astype(np.int64) ** 2).sum()) / N_ONE), flush=True)
    # the worst case: everything inside cell (4, 4) of 8 x 8 over [-W, W)^2, whose extent is W / 4, with a margin for fp32
    W = float(cfg.fieldWidth)
    shrunk = nb.BodiesData.from_arrays(P / 8.5 + W / 8.0, V, M, np.asarray(bodies.Radii, dtype=np.float64) / 8.5)
    worst = nb.Stepper(cfg)
    worst.upload(shrunk)
    Pw, Vw, Mw = widen(shrunk)
    got = worst.cells(8, lists=True)
    cc.assert_same(got, cc.model_cells(Pw, Vw, Mw, got["grid"]), "one cell")
    assert got["info"]["largest"] == N_ONE and got["info"]["occupied"] == 1
    print("# the same state shrunk by 8.5 into cell %d of 8 x 8: largest %d, occupied %d; equal to the model, lists included"
          % (got["info"]["largest_cell"], got["info"]["largest"], got["info"]["occupied"]), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    states = [nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)]
    batch.upload(states)
    got = batch.cells(32, lists=True)
    for s in (0, 1, 127, 255):
        n, inside = int(got["info"]["n"][s]), int(got["info"]["inside"][s])
        mine = {"cells": got["cells"][s], "info": got["info"][s], "cell_of": got["cell_of"][s, :n], "start": got["start"][s],
                "order": got["order"][s, :inside]}
        cc.assert_same(mine, cc.model_cells(*widen(states[s]), got["grid"]), "batch, system %d" % s)
    print("# %d x %d, 32 x 32 over the field: 4 whole systems equal to the model, lists included" % (BATCH_S, BATCH_N), flush=True)
    return np, cfg, st, worst, batch


def one_round(cfg, st, worst, batch):
    """neighbors_at opens a round; then the launches in the order of CASES."""
    st.neighbors()
    st.render_image(cfg.imgWidth, cfg.imgHeight)
    st.cells(256, lists=True)
    st.cells(1024, lists=True)
    worst.neighbors()
    worst.cells(8, lists=True)
    batch.cells(32, lists=True)


def run_kernels(rounds):
    np, cfg, st, worst, batch = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        one_round(cfg, st, worst, batch)
    print("PLAN " + json.dumps({"n": N_ONE, "rounds": rounds}), flush=True)
    st.close()
    worst.close()
    batch.close()


def timed(np, name, call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"call": name, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}), flush=True)
    return float(np.median(ms)), max(ms) - min(ms)


def run_host(reps):
    np, cfg, st, worst, batch = workloads()
    timed(np, "Stepper.neighbors N=%d, stock" % N_ONE, st.neighbors, reps)
    timed(np, "Stepper.render_image %d x %d, stock" % (cfg.imgWidth, cfg.imgHeight), lambda: st.render_image(cfg.imgWidth, cfg.imgHeight), reps)
    for nx in (256, 1024):
        timed(np, "Stepper.cells stock %d x %d, moments, lists" % (nx, nx), lambda: st.cells(nx, lists=True), reps)
        timed(np, "Stepper.cells stock %d x %d, moments, no lists" % (nx, nx), lambda: st.cells(nx), reps)
    near, near_spread = timed(np, "Stepper.neighbors N=%d, one cell of 8 x 8" % N_ONE, worst.neighbors, reps)
    cell, cell_spread = timed(np, "Stepper.cells one cell of 8 x 8, moments, lists", lambda: worst.cells(8, lists=True), reps)
    print("# the worst case, whole calls: cells %.3f ms (spread %.3f) against neighbors %.3f ms (spread %.3f) on the same state: "
          "%.3f; the condition cells <= neighbors %s" % (cell, cell_spread, near, near_spread, cell / near,
                                                         "HOLDS" if cell <= near else "FAILS"), flush=True)
    timed(np, "StepperBatch.cells %d x %d, 32 x 32, moments, lists" % (BATCH_S, BATCH_N), lambda: batch.cells(32, lists=True), reps)
    timed(np, "StepperBatch.cells %d x %d, 32 x 32, moments, no lists" % (BATCH_S, BATCH_N), lambda: batch.cells(32), reps)
    st.close()
    worst.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    rounds = []
    for _, name, ms in rows:
        if "neighbors_at" in name:
            if rounds and len(rounds[-1]["near"]) == 1 and rounds[-1]["cells"]:
                rounds[-1]["near"].append(ms)               # the worst case's, inside the round
            else:
                rounds.append({"near": [ms], "render": [], "cells": []})
        elif "render_discs" in name and rounds:
            rounds[-1]["render"].append(ms)
        elif rounds:
            for k, stage in enumerate(STAGES):
                if stage in name:
                    rounds[-1]["cells"].append((k, ms))
    want = [k for _ in CASES for k in range(len(STAGES))]
    rounds = [r for r in rounds if len(r["near"]) == 2 and len(r["render"]) >= 1 and [k for k, _ in r["cells"]] == want]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    stat = lambda v: "%9.3f ms (%.3f)" % (med(v), max(v) - min(v))
    print("# csrc/tune/cells_probe.py on one MI355X: the kernels of nbody_get_cells next to render_discs and neighbors_at, fp32, N = %d" % N_ONE)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python cells_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-44s %s" % ("neighbors_at own, stock", stat([r["near"][0] for r in rounds])))
    print("%-44s %s" % ("render_discs, stock", stat([r["render"][0] for r in rounds])))
    print("%-44s %s" % ("neighbors_at own, one cell of 8 x 8", stat([r["near"][1] for r in rounds])))
    for c, case in enumerate(CASES):
        total = []
        for k, stage in enumerate(STAGES):
            v = [r["cells"][c * len(STAGES) + k][1] for r in rounds]
            print("%-44s %s" % ("%s, %s" % (stage, case), stat(v)))
        total = [sum(ms for _, ms in r["cells"][c * len(STAGES):(c + 1) * len(STAGES)]) for r in rounds]
        print("%-44s %s" % ("the five kernels, %s" % case, stat(total)))
    if host_log:
        print("# whole calls under the host clock (cells_probe.py host 5; median of 5 after a warm-up), and what was checked:")
        for line in open(host_log):
            if line.startswith(("{", "#")):
                print(line.rstrip())


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    if mode == "kernels":
        run_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else ROUNDS)
    elif mode == "host":
        run_host(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(__doc__)
