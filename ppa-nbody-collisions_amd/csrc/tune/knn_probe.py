#!/usr/bin/env python3
"""Cost of the k-nearest-neighbour queries (nbody_get_knn, nbody_batch_get_knn): knn_at for k = 1, 4, 8, 16
and 32 next to neighbors_at - the kernel that walks the same pairs for the one nearest - timed in the same run on the same
state, and whole calls under the host clock.

    python3 csrc/tune/knn_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                      (a run of its own; nothing else is traced with it)
    python3 csrc/tune/knn_probe.py host [reps]        whole Stepper.knn() / StepperBatch.knn() calls under the host clock,
                                                      next to Stepper.neighbors()
    python3 csrc/tune/knn_probe.py report TRACE_DIR [HOST_LOG]
                                                      reads the kernel trace (csv) and prints the text of
                                                      profiles/knn_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps, points == NULL, k in KS; POINTS explicit points over the field
at k = K_SIDE; a batch of 256 x 1024 with points == NULL at k = K_SIDE.  Before a time is taken every k is checked against
the numpy model (tests/knn_cases.py) on CHECK_ROWS rows of the big state and on whole systems of the batch, and entry 0 of
every row against Stepper.neighbors().

The report sets the measured time next to what counting gives (nbody_knn.hpp): a wave of 64 rows whose lanes each keep the
K nearest takes the insertion branch on about 64 K (1 + ln(n / (64 K))) of its n sources, K the tier of k."""
import csv
import glob
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
POINTS, K_SIDE = 65536, 8
KS = (1, 4, 8, 16, 32)
CHECK_ROWS = 48
ROUNDS = 3                                                   # what `report` expects of `kernels`
NAMES = ["own k=%d" % k for k in KS] + ["%d points k=%d" % (POINTS, K_SIDE), "batch %d x %d k=%d" % (BATCH_S, BATCH_N, K_SIDE)]


def tier(k):
    return next(t for t in (4, 8, 16, 32) if t >= k)


def branch_share(n, k):
    """The share of a wave's pairs on which some lane inserts, by counting: all of the first 64 K, then 64 K / j."""
    full = 64 * tier(k)
    return 1.0 if n <= full else full * (1 + math.log(n / full)) / n


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import knn_cases as kc
    import neighbor_cases as nc
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    P, _ = nc.widen(st.download())
    n = len(P)
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0, 63, 64, 127, 128, n - 1], rng.choice(n, CHECK_ROWS - 6, replace=False)]))
    want = kc.model_knn(P, max(KS), rows=rows, chunk=8)     # the lists of k < 32 are its prefixes
    near = st.neighbors()
    for k in KS:
        got = st.knn(k)
        kc.assert_same(kc.sliced(got, rows), kc.sliced(want, (slice(None), slice(0, k))), "own, k %d" % k)
        assert np.array_equal(kc.bits(got["d2"][:, 0]), kc.bits(near["d2"])) and np.array_equal(got["index"][:, 0], near["index"])
    lo, hi = P.min(axis=0), P.max(axis=0)
    pts = lo + rng.uniform(0, 1, size=(POINTS, 2)) * (hi - lo)
    got = st.knn(K_SIDE, pts)
    kc.assert_same(kc.sliced(got, slice(0, CHECK_ROWS)), kc.model_knn(P, K_SIDE, points=pts[:CHECK_ROWS], chunk=8), "points")
    print("# N=%d after %d steps: n %d; k = %s on %d rows and %d of the %d points equal to the model, entry 0 of every row "
          "equal to neighbors()" % (N_ONE, STEPS, n, "/".join(map(str, KS)), len(rows), CHECK_ROWS, POINTS), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    got = batch.knn(K_SIDE)
    for s in (0, 1, 127, 255):
        kc.assert_same(got[s], kc.model_knn(nc.widen(batch.download(s))[0], K_SIDE), "batch, system %d" % s)
    print("# %d x %d after %d steps: %d bodies left; k = %d, 4 whole systems equal to the model"
          % (BATCH_S, BATCH_N, STEPS, int(batch.counts().sum()), K_SIDE), flush=True)
    return np, st, pts, batch, n


def run_kernels(rounds):
    np, st, pts, batch, n = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        st.neighbors()                                      # neighbors_at on the same state opens every round
        for k in KS:
            st.knn(k)
        st.knn(K_SIDE, pts)
        batch.knn(K_SIDE)
    print("PLAN " + json.dumps({"n": n, "rounds": rounds}), flush=True)
    st.close()
    batch.close()


def timed(np, name, call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"call": name, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}), flush=True)


def run_host(reps):
    np, st, pts, batch, n = workloads()
    timed(np, "Stepper.neighbors() N=%d (n %d)" % (N_ONE, n), lambda: st.neighbors(), reps)
    for k in KS:
        timed(np, "Stepper.knn(%d) N=%d (n %d)" % (k, N_ONE, n), lambda: st.knn(k), reps)
    timed(np, "Stepper.knn(%d, %d points)" % (K_SIDE, POINTS), lambda: st.knn(K_SIDE, pts), reps)
    timed(np, "StepperBatch.knn(%d) %d x %d" % (K_SIDE, BATCH_S, BATCH_N), lambda: batch.knn(K_SIDE), reps)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # a round: one neighbors_at launch, then the seven knn_at launches in the order of NAMES
    rounds = []
    for _, name, ms in rows:
        if "neighbors_at" in name:
            rounds.append({"near": ms, "knn": []})
        elif "knn_at" in name and rounds:
            rounds[-1]["knn"].append(ms)
    rounds = [r for r in rounds if len(r["knn"]) == len(NAMES)]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    n = None
    if host_log:
        for line in open(host_log):
            if line.startswith("# N=") and " n " in line:
                n = int(line.split(" n ")[1].split(";")[0])
    med = lambda v: sorted(v)[len(v) // 2]
    near = [r["near"] for r in rounds]
    print("# csrc/tune/knn_probe.py on one MI355X: knn_at next to neighbors_at, fp32, the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python knn_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("# branch: the share of a wave's pairs on which some lane inserts, by counting (64 K (1 + ln(n / (64 K))) / n, K the tier)")
    print("%-26s %8.3f ms (%.3f)" % ("neighbors_at own", med(near), max(near) - min(near)))
    for c, name in enumerate(NAMES):
        mine = [r["knn"][c] for r in rounds]
        line = "%-26s %8.3f ms (%.3f)" % (name, med(mine), max(mine) - min(mine))
        if c < len(KS):
            line += "  knn_at / neighbors_at %.3f  tier %2d" % (med(mine) / med(near), tier(KS[c]))
            if n:
                line += "  branch %.4f" % branch_share(n, KS[c])
        print(line)
    if host_log:
        print("# whole calls under the host clock (knn_probe.py host 5; median of 5 after a warm-up), and what was checked:")
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
