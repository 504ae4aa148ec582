#!/usr/bin/env python3
"""Cost of the k nearest on the cell list (nbody_get_knn_grid, nbody_batch_get_knn_grid): the kernels of a
call - the four list stages of the cell sums, cells_gather and knn_grid_walk - next to knn_at, the O(n^2) yardstick, timed in
the same run on the same state, and whole Stepper.knn(k, grid=...) calls under the host clock next to Stepper.knn(k).

    python3 csrc/tune/knn_grid_probe.py kernels [rounds]  the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                          (a run of its own; nothing else is traced with it)
    python3 csrc/tune/knn_grid_probe.py host [reps]       whole calls under the host clock, the grid call next to the
                                                          brute-force call on the same state; states the speed condition
    python3 csrc/tune/knn_grid_probe.py report TRACE_DIR [HOST_LOG]
                                                          reads the kernel trace (csv) and prints the text of
                                                          profiles/knn_grid_probe.txt

Shapes: N = 262144 fp32, the stock seeded state, own rows, k = 8 and k = 32 on knn_grid(field, k, n), h0 = the cell side.
The worst case: the same state shrunk into one cell of the 8 x 8 grid over the field, k = 8 - every row walks all n records
from memory.  A batch of 256 x 1024 on 32 x 32, k = 8.  Before a time is taken every case is checked: SAMPLE rows (64 of
the worst case) against the numpy model (tests/knn_grid_cases.py; all rows of 4 systems for the batch) bit for bit, and,
where the grid holds every body, ALL rows against Stepper.knn(k) byte for byte."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N = 262144, 256, 1024
ROUNDS = 3                                                   # what `report` expects of `kernels`
SAMPLE = 1024
FIRST = "cells_assign"                                       # the kernel a grid call opens with
STAGES = ["cells_assign", "cells_scan", "cells_place", "cells_rank", "cells_gather", "knn_grid_walk"]
CASES = ["stock, k = 8 on knn_grid", "stock, k = 32 on knn_grid", "one cell of 8 x 8, k = 8", "batch %d x %d, 32 x 32, k = 8" % (BATCH_S, BATCH_N)]


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import knn_grid_cases as kg

    def widen(b):
        return np.asarray(b.Positions, dtype=np.float64)

    def check(st, P, grid, k, what, sample=SAMPLE, brute=True):
        got = st.knn(k, grid=grid)
        rows = np.random.default_rng(11).choice(len(P), size=sample, replace=False)
        want = kg.model_knn_grid_sample(P, got["grid"], k, np.inf, rows)
        kg.assert_same({"d2": got["d2"][rows], "index": got["index"][rows]}, want, what, info=False)
        assert got["info"]["outside"] == 0 and got["info"]["rows"] == len(P), (what, got["info"])
        if brute:
            plain = st.knn(k)
            assert plain["d2"].tobytes() == got["d2"].tobytes() and plain["index"].tobytes() == got["index"].tobytes(), what
        print("# %s: grid %d x %d, %d rows, widened %d (%.4f of the rows), rounds %d; %d sampled rows equal to the model bit for "
              "bit%s" % (what, got["grid"]["nx"], got["grid"]["ny"], got["info"]["rows"], got["info"]["widened"],
                         got["info"]["widened"] / max(got["info"]["rows"], 1), got["info"]["rounds"], sample,
                         ", all rows equal to Stepper.knn(k) byte for byte" if brute else ""), flush=True)

    cfg = nb.stock_config(particleCount=N_ONE)
    bodies = nb.init_bodies(cfg)
    st = nb.Stepper(cfg)
    st.upload(bodies)
    P = widen(bodies)
    W = float(cfg.fieldWidth)
    grids = {k: nb.knn_grid((W, W), k, N_ONE) for k in (8, 32)}
    for k in (8, 32):
        check(st, P, grids[k], k, "N=%d stock seeded state, k = %d" % (N_ONE, k))
    # the worst case: everything inside cell (4, 4) of 8 x 8 over [-W, W)^2, whose extent is W / 4, with a margin for fp32
    g8 = nb.make_grid(8, 8, (-W, W, -W, W))
    R = np.asarray(bodies.Radii, dtype=np.float64)
    shrunk = nb.BodiesData.from_arrays(P / 8.5 + W / 8.0, np.zeros_like(P), np.asarray(bodies.Masses, dtype=np.float64), R / 8.5)
    worst = nb.Stepper(cfg)
    worst.upload(shrunk)
    check(worst, widen(shrunk), g8, 8, "the same state shrunk by 8.5 into one cell of 8 x 8, k = 8", sample=64, brute=False)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    bW = float(bcfg.fieldWidth)
    bgrid = nb.make_grid(32, 32, (-bW, bW, -bW, bW))
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    states = [nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)]
    batch.upload(states)
    got = batch.knn(8, grid=bgrid)
    for s in (0, 1, 127, 255):
        kg.assert_same(got[s], kg.rule_model(widen(states[s]), bgrid[0], 8, kg.default_h0(bgrid[0])), "batch, system %d" % s)
    print("# %d x %d, 32 x 32 over the field, k = 8: 4 whole systems equal to the model, info included; widened %d rows in all" % (
        BATCH_S, BATCH_N, sum(g["info"]["widened"] for g in got)), flush=True)
    grid_calls = [lambda: st.knn(8, grid=grids[8]), lambda: st.knn(32, grid=grids[32]), lambda: worst.knn(8, grid=g8),
                  lambda: batch.knn(8, grid=bgrid)]
    brute_calls = [lambda: st.knn(8), lambda: st.knn(32), lambda: worst.knn(8), lambda: batch.knn(8)]
    return np, (st, worst, batch), grid_calls, brute_calls


def run_kernels(rounds):
    np, handles, grid_calls, brute_calls = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for brute, grid in zip(brute_calls, grid_calls):    # knn_at, then the grid call's kernels, case by case
            brute()
            grid()
    print("PLAN " + json.dumps({"n": N_ONE, "rounds": rounds}), flush=True)
    for h in handles:
        h.close()


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
    np, handles, grid_calls, brute_calls = workloads()
    for k, case in enumerate(CASES):
        who = "StepperBatch" if k == 3 else "Stepper"
        brute, bspread = timed(np, "%s.knn %s, no grid" % (who, case), brute_calls[k], reps)
        ms, spread = timed(np, "%s.knn %s" % (who, case), grid_calls[k], reps)
        if k < 2:
            print("# %s, whole call: %.3f ms (spread %.3f) against the brute-force call %.3f ms (spread %.3f) on the same state: "
                  "%.4f, %.1f times faster; the condition grid < brute force %s" % (case, ms, spread, brute, bspread, ms / brute, brute / ms,
                                                                                   "HOLDS" if ms < brute else "FAILS"), flush=True)
        else:
            print("# %s, whole call: %.3f ms (spread %.3f) against the brute-force call %.3f ms (spread %.3f): %.3f; no condition" % (
                case, ms, spread, brute, bspread, ms / brute), flush=True)
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    events = []                                             # ("brute", ms) or ("call", {stage: ms})
    for _, name, ms in rows:
        if "knn_at" in name:
            events.append(("brute", ms))
        elif FIRST in name:
            events.append(("call", {FIRST: ms}))
        elif events and events[-1][0] == "call":
            for stage in STAGES:
                if stage in name:
                    events[-1][1][stage] = events[-1][1].get(stage, 0.0) + ms
    per_round = 2 * len(CASES)
    events = events[-ROUNDS * per_round:]                   # without the checks and the warm-up round
    rounds = [events[k * per_round:(k + 1) * per_round] for k in range(ROUNDS)]
    assert all([kind for kind, _ in r] == ["brute", "call"] * len(CASES) for r in rounds), [[kind for kind, _ in r] for r in rounds]
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    stat = lambda v: "%9.3f ms (%.3f)" % (med(v), max(v) - min(v))   # noqa: E731
    print("# csrc/tune/knn_grid_probe.py on one MI355X: the kernels of nbody_get_knn_grid next to knn_at, fp32, N = %d" % N_ONE)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python knn_grid_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    for c, case in enumerate(CASES):
        print("%-60s %s" % ("knn_at own, %s" % case, stat([r[2 * c][1] for r in rounds])))
        calls = [r[2 * c + 1][1] for r in rounds]
        for stage in STAGES:
            assert all(stage in call for call in calls), (case, stage)
            print("%-60s %s" % ("%s, %s" % (stage, case), stat([call[stage] for call in calls])))
        print("%-60s %s" % ("all kernels, %s" % case, stat([sum(call.values()) for call in calls])))
    if host_log:
        print("# whole calls under the host clock (knn_grid_probe.py host 5; median of 5 after a warm-up), and what was checked:")
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
