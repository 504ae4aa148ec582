#!/usr/bin/env python3
"""Cost of the radius queries (nbody_get_within, nbody_batch_get_within): the kernels of a call - the four
list stages of the cell sums, then cells_gather, within_walk, the row scan and, with lists, the second walk and within_rank -
next to neighbors_at, the O(n^2) yardstick, timed in the same run on the same state, and whole calls under the host clock
next to Stepper.neighbors().

    python3 csrc/tune/within_probe.py kernels [rounds]  the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                        (a run of its own; nothing else is traced with it)
    python3 csrc/tune/within_probe.py host [reps]       whole Stepper.within() / StepperBatch.within() calls under the host
                                                        clock, next to Stepper.neighbors() on the same state
    python3 csrc/tune/within_probe.py report TRACE_DIR [HOST_LOG]
                                                        reads the kernel trace (csv) and prints the text of
                                                        profiles/within_probe.txt

Shapes: N = 262144 fp32, the stock seeded state; h = the cell side of a 256 x 256 and of a 1024 x 1024 grid over the field,
on that grid, without and with lists.  The worst case of the cell sums: the same state shrunk into one cell of the 8 x 8 grid
over the field, h = that cell's side - every row walks all n records from memory - without lists (n^2 entries have no
room).  A batch of 256 x 1024 on 32 x 32, h = the cell side, with lists.  Before a time is taken every case is checked:
SAMPLE rows (64 of the worst case) against the numpy model (tests/within_cases.py; all rows of 4 systems for the batch),
every row's list ascending and as long as its count, and the sum of the counts against Stepper.pair_counts()."""
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
FIRST = "cells_assign"                                       # the kernel a call opens with
STAGES = ["cells_assign", "cells_scan", "cells_place", "cells_rank", "cells_gather", "within_walk", "within_block_sums",
          "within_block_scan", "within_block_starts", "within_rank"]
LISTS_ONLY = ("within_block_starts", "within_rank")
CASES = [("stock 256 x 256, h = cell", False), ("stock 256 x 256, h = cell, lists", True), ("stock 1024 x 1024, h = cell", False),
         ("stock 1024 x 1024, h = cell, lists", True), ("one cell of 8 x 8, h = cell", False),
         ("batch %d x %d, 32 x 32, h = cell, lists" % (BATCH_S, BATCH_N), True)]


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import within_cases as wc

    def widen(b):
        return np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Radii, dtype=np.float64)

    def check(st, P, R, grid, h, what, lists=True, sample=SAMPLE):
        got = st.within(h, grid=grid, lists=lists)
        rows = np.random.default_rng(11).choice(len(P), size=sample, replace=False)
        want = wc.model_within(P, R, got["grid"], h * h, chunk=32, rows=rows)
        wc.assert_same({"rows": got["rows"][rows], "info": want["info"]}, want, what, lists=False)
        pairs = st.pair_counts(np.array([0.0, np.nextafter(h * h, np.inf)]), squared=True)
        assert got["info"]["outside"] == 0 and got["info"]["total"] == 2 * int(pairs["counts"][0]), (what, got["info"], pairs)
        if lists:
            assert wc.lists_consistent(got), what
            for k, i in enumerate(rows[:64]):
                assert np.array_equal(got["list"][got["start"][i]:got["start"][i + 1]], want["list"][want["start"][k]:want["start"][k + 1]]), what
        print("# %s: %d rows, total %d (%.2f per row), largest %d; %d sampled rows equal to the model, the total equal to 2 x "
              "pair_counts%s" % (what, got["info"]["rows"], got["info"]["total"], got["info"]["total"] / max(got["info"]["rows"], 1),
                                 got["info"]["largest"], sample, ", every list ascending" if lists else ""), flush=True)

    cfg = nb.stock_config(particleCount=N_ONE)
    bodies = nb.init_bodies(cfg)
    st = nb.Stepper(cfg)
    st.upload(bodies)
    P, R = widen(bodies)
    W = float(cfg.fieldWidth)
    grids = {nx: nb.make_grid(nx, nx, (-W, W, -W, W)) for nx in (8, 32, 256, 1024)}
    side = {nx: 2.0 * W / nx for nx in grids}
    for nx in (256, 1024):
        check(st, P, R, grids[nx], side[nx], "N=%d stock seeded state, %d x %d over the field, h = %g" % (N_ONE, nx, nx, side[nx]))
    # the worst case: everything inside cell (4, 4) of 8 x 8 over [-W, W)^2, whose extent is W / 4, with a margin for fp32
    shrunk = nb.BodiesData.from_arrays(P / 8.5 + W / 8.0, np.zeros_like(P), np.asarray(bodies.Masses, dtype=np.float64), R / 8.5)
    worst = nb.Stepper(cfg)
    worst.upload(shrunk)
    Pw, Rw = widen(shrunk)
    check(worst, Pw, Rw, grids[8], side[8], "the same state shrunk by 8.5 into one cell of 8 x 8, h = %g" % side[8], lists=False, sample=64)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    bW = float(bcfg.fieldWidth)
    bgrid, bh = nb.make_grid(32, 32, (-bW, bW, -bW, bW)), 2.0 * bW / 32
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    states = [nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)]
    batch.upload(states)
    got = batch.within(bh, grid=bgrid, lists=True)
    for s in (0, 1, 127, 255):
        wc.assert_same(got[s], wc.model_within(*widen(states[s]), bgrid[0], bh * bh), "batch, system %d" % s)
    print("# %d x %d, 32 x 32 over the field, h = %g: 4 whole systems equal to the model, lists included; total %d" % (
        BATCH_S, BATCH_N, bh, sum(g["info"]["total"] for g in got)), flush=True)
    calls = [lambda: st.within(side[256], grid=grids[256]), lambda: st.within(side[256], grid=grids[256], lists=True),
             lambda: st.within(side[1024], grid=grids[1024]), lambda: st.within(side[1024], grid=grids[1024], lists=True),
             lambda: worst.within(side[8], grid=grids[8]), lambda: batch.within(bh, grid=bgrid, lists=True)]
    return np, st, worst, batch, calls


def one_round(st, worst, calls):
    """neighbors_at opens a round and precedes the worst case; the calls in the order of CASES."""
    st.neighbors()
    for k, call in enumerate(calls):
        if k == 4:
            worst.neighbors()
        call()


def run_kernels(rounds):
    np, st, worst, batch, calls = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        one_round(st, worst, calls)
    print("PLAN " + json.dumps({"n": N_ONE, "rounds": rounds}), flush=True)
    for h in (st, worst, batch):
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
    np, st, worst, batch, calls = workloads()
    near, near_spread = timed(np, "Stepper.neighbors N=%d, stock" % N_ONE, st.neighbors, reps)
    for k, (case, _) in enumerate(CASES):
        if k == 4:
            wnear, wspread = timed(np, "Stepper.neighbors N=%d, one cell of 8 x 8" % N_ONE, worst.neighbors, reps)
        name = ("StepperBatch" if k == 5 else "Stepper") + ".within " + case
        ms, spread = timed(np, name, calls[k], reps)
        if k < 4:
            print("# %s, whole call: %.3f ms (spread %.3f) against neighbors %.3f ms (spread %.3f) on the same state: %.4f; the "
                  "condition within < neighbors %s" % (case, ms, spread, near, near_spread, ms / near,
                                                        "HOLDS" if ms < near else "FAILS"), flush=True)
        elif k == 4:
            print("# the worst case, whole call: %.3f ms (spread %.3f) against neighbors %.3f ms (spread %.3f): %.3f; no condition: "
                  "use a grid matched to h" % (ms, spread, wnear, wspread, ms / wnear), flush=True)
    for h in (st, worst, batch):
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    events = []                                             # ("near", ms) or ("call", {stage: [ms, ...]})
    for _, name, ms in rows:
        if "neighbors_at" in name:
            events.append(("near", ms))
        elif FIRST in name:
            events.append(("call", {FIRST: [ms]}))
        elif events and events[-1][0] == "call":
            for stage in STAGES:
                if stage in name:
                    events[-1][1].setdefault(stage, []).append(ms)
    per_round = len(CASES) + 2
    pattern = ["near"] + ["call"] * 4 + ["near"] + ["call"] * 2
    events = events[-ROUNDS * per_round:]                   # without the checks and the warm-up round
    rounds = [events[k * per_round:(k + 1) * per_round] for k in range(ROUNDS)]
    assert all([kind for kind, _ in r] == pattern for r in rounds), [[kind for kind, _ in r] for r in rounds]
    med = lambda v: sorted(v)[len(v) // 2]                  # noqa: E731
    stat = lambda v: "%9.3f ms (%.3f)" % (med(v), max(v) - min(v))   # noqa: E731
    print("# csrc/tune/within_probe.py on one MI355X: the kernels of nbody_get_within next to neighbors_at, fp32, N = %d" % N_ONE)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python within_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-60s %s" % ("neighbors_at own, stock", stat([r[0][1] for r in rounds])))
    print("%-60s %s" % ("neighbors_at own, one cell of 8 x 8", stat([r[5][1] for r in rounds])))
    slots = [1, 2, 3, 4, 6, 7]
    for c, (case, lists) in enumerate(CASES):
        calls = [r[slots[c]][1] for r in rounds]
        for stage in STAGES:
            launches = 2 if (lists and stage == "within_walk") else 1
            if stage in LISTS_ONLY and not lists:
                continue
            assert all(len(call.get(stage, [])) == launches for call in calls), (case, stage, [call.get(stage) for call in calls])
            for k in range(launches):
                label = stage + (", the counting pass" if launches == 2 and k == 0 else ", the filling pass" if launches == 2 else "")
                print("%-60s %s" % ("%s, %s" % (label, case), stat([call[stage][k] for call in calls])))
        print("%-60s %s" % ("all kernels, %s" % case, stat([sum(sum(v) for v in call.values()) for call in calls])))
    if host_log:
        print("# whole calls under the host clock (within_probe.py host 5; median of 5 after a warm-up), and what was checked:")
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
