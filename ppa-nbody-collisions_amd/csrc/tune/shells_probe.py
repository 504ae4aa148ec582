#!/usr/bin/env python3
"""Cost of the shell sums (nbody_get_shells, nbody_batch_get_shells): shells_at next to pair_counts - whose
points kernel is the same full walk with the same hot loop - and neighbors_at, timed in the same run on the same state, and
whole calls under the host clock.

    python3 csrc/tune/shells_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                         (a run of its own; nothing else is traced with it)
    python3 csrc/tune/shells_probe.py host [reps]        whole Stepper.shells() / StepperBatch.shells() calls under the host
                                                         clock, next to Stepper.pair_counts()
    python3 csrc/tune/shells_probe.py report TRACE_DIR [HOST_LOG]
                                                         reads the kernel trace (csv) and prints the text of
                                                         profiles/shells_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps (the state of pairs_probe.py).  Edges: geometric over three decades
below the two tops of pairs_probe.py - (a) its sparse centre link, (b) its percolating one - with 8 and 32 bins, and one bin
[0, +inf), on which every pair takes the rare path.  Own rows; POINTS explicit points over the field, for shells_at and for
pair_counts (the yardstick, per pair); a batch of 256 x 1024 with points == NULL.  Before a time is taken every case is checked
against the numpy model (tests/shell_cases.py) on CHECK_ROWS rows of the big state and on whole systems of the batch, and the
row sums against pair_counts."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
POINTS = 65536
CHECK_ROWS = 48
ROUNDS = 3                                                   # what `report` expects of `kernels`
MEAN_SMALL, MEAN_PERCOLATING = 1.5, 7.0                     # pairs_probe.py's: others within reach of a body, on average
OWN = ["(a) 8 bins", "(a) 32 bins", "(b) 8 bins", "(b) 32 bins", "[0, inf) 1 bin"]
PTS = ["(a) 32 bins", "(b) 32 bins"]
PAIRS = ["pair_counts own (a) 32 bins", "pair_counts own (b) 32 bins", "pair_counts %d points (a) 32 bins" % POINTS,
         "pair_counts %d points (b) 32 bins" % POINTS]
SHELLS = (["shells_at own %s" % c for c in OWN] + ["shells_at %d points %s" % (POINTS, c) for c in PTS]
          + ["shells_at batch %d x %d (a) 8 bins" % (BATCH_S, BATCH_N)])


def centre_link(np, mean, P):
    """pairs_probe.py's: the length at which a body has `mean` others within reach on average."""
    area = float(np.prod(P.max(axis=0) - P.min(axis=0)))
    return float(np.sqrt(mean * area / (np.pi * len(P))))


def log_edges(np, top, bins):
    return np.geomspace(top / 1000.0, top, bins + 1) ** 2


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import shell_cases as shc
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    P, M = shc.widen_mass(st.download())
    n = len(P)
    small, perc = centre_link(np, MEAN_SMALL, P), centre_link(np, MEAN_PERCOLATING, P)
    own = list(zip(OWN, [log_edges(np, small, 8), log_edges(np, small, 32), log_edges(np, perc, 8), log_edges(np, perc, 32),
                         np.array([0.0, np.inf])]))
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0, 63, 64, 127, 128, n - 1], rng.choice(n, CHECK_ROWS - 6, replace=False)]))
    lo, hi = P.min(axis=0), P.max(axis=0)
    pts = lo + rng.uniform(0, 1, size=(POINTS, 2)) * (hi - lo)
    for name, e2 in own:                                    # equal to the model before any time is taken
        got = st.shells(e2, squared=True)
        shc.assert_same(shc.sliced(got, rows), shc.model_shells(P, M, e2, rows=rows), "own, " + name)
        inside = int(got["count"].sum(dtype=np.int64))
        if np.isfinite(e2[-1]):
            dd = st.pair_counts(e2, squared=True)
            assert got["count"].sum(axis=0, dtype=np.int64).tolist() == (2 * dd["counts"].astype(np.int64)).tolist(), name
        else:
            assert inside == n * (n - 1), name
        # a trip of four pairs takes the rare path where any of a wave's 256 pairs is in range: an upper bound from the share
        print("# N=%d after %d steps: n %d, own %s: edges %.6g .. %.6g (lengths) -> in range %d of %d ordered pairs (%.3e; at most "
              "%.4f of the wave-level trips); %d rows equal to the model, row sums equal to 2 x pair_counts"
              % (N_ONE, STEPS, n, name, np.sqrt(e2[0]), np.sqrt(e2[-1]), inside, n * (n - 1), inside / (n * (n - 1.0)),
                 min(1.0, 256.0 * inside / (n * (n - 1.0))), len(rows)), flush=True)
    pcases = [(PTS[0], own[1][1]), (PTS[1], own[3][1])]
    for name, e2 in pcases:
        got = st.shells(e2, pts, squared=True)
        shc.assert_same(shc.sliced(got, slice(0, CHECK_ROWS)), shc.model_shells(P, M, e2, pts[:CHECK_ROWS]), "points, " + name)
        dr = st.pair_counts(e2, points=pts, squared=True)
        assert got["count"].sum(axis=0, dtype=np.int64).tolist() == dr["counts"].astype(np.int64).tolist(), name
        print("# %d points %s: %d of the points equal to the model, sums equal to pair_counts' DR counts" % (POINTS, name, CHECK_ROWS),
              flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    be2 = log_edges(np, centre_link(np, MEAN_SMALL, shc.widen_mass(batch.download(0))[0]), 8)
    got = batch.shells(be2, squared=True)
    for s in (0, 1, 127, 255):
        Ps, Ms = shc.widen_mass(batch.download(s))
        shc.assert_same(got[s], shc.model_shells(Ps, Ms, be2), "batch, system %d" % s)
    print("# %d x %d after %d steps: %d bodies left; (a) 8 bins, edges %.6g .. %.6g (lengths), 4 whole systems equal to the model"
          % (BATCH_S, BATCH_N, STEPS, int(batch.counts().sum()), np.sqrt(be2[0]), np.sqrt(be2[-1])), flush=True)
    return np, st, own, pcases, pts, batch, be2, n


def one_round(st, own, pcases, pts, batch, be2):
    """neighbors_at opens a round; then the launches in the order of PAIRS and of SHELLS."""
    st.neighbors()
    for _, e2 in pcases:
        st.pair_counts(e2, squared=True)
    for _, e2 in pcases:
        st.pair_counts(e2, points=pts, squared=True)
    for _, e2 in own:
        st.shells(e2, squared=True)
    for _, e2 in pcases:
        st.shells(e2, pts, squared=True)
    batch.shells(be2, squared=True)


def run_kernels(rounds):
    np, st, own, pcases, pts, batch, be2, n = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        one_round(st, own, pcases, pts, batch, be2)
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
    np, st, own, pcases, pts, batch, be2, n = workloads()
    timed(np, "Stepper.pair_counts N=%d (n %d): (a) 32 bins" % (N_ONE, n), lambda: st.pair_counts(pcases[0][1], squared=True), reps)
    for name, e2 in own:
        timed(np, "Stepper.shells N=%d (n %d): %s" % (N_ONE, n, name), lambda: st.shells(e2, squared=True), reps)
    timed(np, "Stepper.shells(%d points): (a) 32 bins" % POINTS, lambda: st.shells(pcases[0][1], pts, squared=True), reps)
    timed(np, "StepperBatch.shells %d x %d: (a) 8 bins" % (BATCH_S, BATCH_N), lambda: batch.shells(be2, squared=True), reps)
    st.close()
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
            rounds.append({"near": ms, "pairs": [], "shells": []})
        elif "pair_counts" in name and rounds:
            rounds[-1]["pairs"].append(ms)
        elif "shells_at" in name and rounds:
            rounds[-1]["shells"].append(ms)
    rounds = [r for r in rounds if len(r["pairs"]) == len(PAIRS) and len(r["shells"]) == len(SHELLS)]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    n = None
    if host_log:
        for line in open(host_log):
            if line.startswith("# N=") and " n " in line:
                n = int(line.split(" n ")[1].split(",")[0])
    med = lambda v: sorted(v)[len(v) // 2]
    stat = lambda v: "%9.3f ms (%.3f)" % (med(v), max(v) - min(v))
    print("# csrc/tune/shells_probe.py on one MI355X: shells_at next to pair_counts and neighbors_at, fp32, the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python shells_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min); ps per pair where n is known")
    ordered = n * (n - 1.0) if n else None
    per = lambda ms, pairs: "  %7.3f ps/pair" % (ms * 1e9 / pairs) if pairs else ""
    near = [r["near"] for r in rounds]
    print("%-42s %s%s" % ("neighbors_at own", stat(near), per(med(near), ordered)))
    pm = []
    for c, name in enumerate(PAIRS):
        v = [r["pairs"][c] for r in rounds]
        pm.append(med(v))
        print("%-42s %s%s" % (name, stat(v), per(med(v), (ordered / 2 if c < 2 else POINTS * float(n)) if n else None)))
    for c, name in enumerate(SHELLS):
        v = [r["shells"][c] for r in rounds]
        line = "%-42s %s" % (name, stat(v))
        if c < len(OWN):
            line += per(med(v), ordered)
            if c < 4:
                line += "  shells_at / pair_counts own (the triangle) %.3f" % (med(v) / pm[c // 2])
        elif c < len(OWN) + len(PTS):
            line += per(med(v), POINTS * float(n) if n else None)
            line += "  shells_at / pair_counts, the same points and edges %.3f" % (med(v) / pm[2 + c - len(OWN)])
        print(line)
    if host_log:
        print("# whole calls under the host clock (shells_probe.py host 5; median of 5 after a warm-up), and what was checked:")
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
