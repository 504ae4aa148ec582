#!/usr/bin/env python3
"""Cost of the shell moments (nbody_get_shell_moments, nbody_batch_get_shell_moments): shell_moments_at next to
shells_at at its 8-bin tier - the same full walk with the same hot loop, the yardstick per pair - timed in the same run on the
same state and the same edges.

    python3 csrc/tune/shell_moments_probe.py kernels [rounds]    the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                                 (a run of its own; nothing else is traced with it)
    python3 csrc/tune/shell_moments_probe.py report TRACE_DIR [LOG]
                                                                 reads the kernel trace (csv) and the `kernels` run's output
                                                                 and prints the text of profiles/shell_moments_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps (the state of shells_probe.py).  Edges: shells_probe.py's (a) and
(b), geometric over three decades below its sparse and its percolating top, with 8 bins.  Own rows; POINTS explicit points
over the field moving with random velocities; a batch of 256 x 1024 with points == NULL.  Before a time is taken every case is
checked against the numpy model (tests/shell_moment_cases.py) on CHECK_ROWS rows of the big state and on whole systems of the
batch, and mass and count against shells()."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
POINTS = 65536
CHECK_ROWS = 48
ROUNDS = 3                                                   # what `report` expects of `kernels`
MEAN_SMALL, MEAN_PERCOLATING = 1.5, 7.0                     # shells_probe.py's
CASES = ["own (a) 8 bins", "own (b) 8 bins", "%d points (a) 8 bins" % POINTS, "%d points (b) 8 bins" % POINTS,
         "batch %d x %d (a) 8 bins" % (BATCH_S, BATCH_N)]


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import shell_moment_cases as smc
    from shells_probe import centre_link, log_edges
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    P, V, M = smc.widen_state(st.download())
    n = len(P)
    edges = [log_edges(np, centre_link(np, MEAN_SMALL, P), 8), log_edges(np, centre_link(np, MEAN_PERCOLATING, P), 8)]
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0, 63, 64, 127, 128, n - 1], rng.choice(n, CHECK_ROWS - 6, replace=False)]))
    lo, hi = P.min(axis=0), P.max(axis=0)
    pts = lo + rng.uniform(0, 1, size=(POINTS, 2)) * (hi - lo)
    vel = rng.uniform(-1, 1, size=(POINTS, 2)) * np.abs(V).max()
    for name, e2 in zip("ab", edges):                       # equal to the model before any time is taken
        got, sums = st.shell_moments(e2, squared=True)["moments"], st.shells(e2, squared=True)
        smc.assert_same(got[rows], smc.model_shell_moments(P, V, M, e2, rows=rows), "own, " + name)
        assert np.array_equal(smc.bits(got["mass"]), smc.bits(sums["mass"])) and np.array_equal(got["count"], sums["count"]), name
        inside = int(got["count"].sum(dtype=np.int64))
        hit_rows = int((got["count"].sum(axis=1) > 0).sum())
        print("# N=%d after %d steps: n %d, own (%s) 8 bins: edges %.6g .. %.6g (lengths) -> in range %d of %d ordered pairs (%.3e; at "
              "most %.4f of the wave-level trips), %d rows with a source in range; %d rows equal to the model, mass and count equal to "
              "shells()" % (N_ONE, STEPS, n, name, np.sqrt(e2[0]), np.sqrt(e2[-1]), inside, n * (n - 1), inside / (n * (n - 1.0)),
                            min(1.0, 256.0 * inside / (n * (n - 1.0))), hit_rows, len(rows)), flush=True)
        got, sums = st.shell_moments(e2, pts, vel, squared=True)["moments"], st.shells(e2, pts, squared=True)
        smc.assert_same(got[:CHECK_ROWS], smc.model_shell_moments(P, V, M, e2, pts[:CHECK_ROWS], vel[:CHECK_ROWS]), "points, " + name)
        assert np.array_equal(smc.bits(got["mass"]), smc.bits(sums["mass"])) and np.array_equal(got["count"], sums["count"]), name
        print("# %d moving points (%s) 8 bins: in range %d of %d pairs (%.3e); %d of the points equal to the model, mass and count "
              "equal to shells()" % (POINTS, name, int(got["count"].sum(dtype=np.int64)), POINTS * n,
                                     got["count"].sum(dtype=np.int64) / (POINTS * float(n)), CHECK_ROWS), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    be2 = log_edges(np, centre_link(np, MEAN_SMALL, smc.widen_state(batch.download(0))[0]), 8)
    got = batch.shell_moments(be2, squared=True)
    for s in (0, 1, 127, 255):
        smc.assert_same(got[s], smc.model_shell_moments(*smc.widen_state(batch.download(s)), be2), "batch, system %d" % s)
    print("# %d x %d after %d steps: %d bodies left; (a) 8 bins, edges %.6g .. %.6g (lengths), 4 whole systems equal to the model"
          % (BATCH_S, BATCH_N, STEPS, int(batch.counts().sum()), np.sqrt(be2[0]), np.sqrt(be2[-1])), flush=True)
    return st, edges, pts, vel, batch, be2, n


def one_round(st, edges, pts, vel, batch, be2):
    """neighbors_at opens a round; then, case by case in the order of CASES, shells_at and shell_moments_at."""
    st.neighbors()
    for e2 in edges:
        st.shells(e2, squared=True)
        st.shell_moments(e2, squared=True)
    for e2 in edges:
        st.shells(e2, pts, squared=True)
        st.shell_moments(e2, pts, vel, squared=True)
    batch.shells(be2, squared=True)
    batch.shell_moments(be2, squared=True)


def run_kernels(rounds):
    st, edges, pts, vel, batch, be2, n = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        one_round(st, edges, pts, vel, batch, be2)
    print("PLAN " + json.dumps({"n": n, "rounds": rounds}), flush=True)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    rounds = []
    for _, name, ms in rows:
        if "neighbors_at" in name:
            rounds.append({"shells": [], "moments": []})
        elif "shell_moments_at" in name and rounds:
            rounds[-1]["moments"].append(ms)
        elif "shells_at" in name and rounds:
            rounds[-1]["shells"].append(ms)
    rounds = [r for r in rounds if len(r["shells"]) == len(CASES) and len(r["moments"]) == len(CASES)]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    stat = lambda v: "%8.3f ms (%.3f)" % (med(v), max(v) - min(v))
    print("# csrc/tune/shell_moments_probe.py on one MI355X: shell_moments_at next to shells_at at its 8-bin tier, fp32, the stock state "
          "after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python shell_moments_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-32s %-22s %-22s %s" % ("case", "shells_at", "shell_moments_at", "moments / shells"))
    for c, name in enumerate(CASES):
        s, m = [r["shells"][c] for r in rounds], [r["moments"][c] for r in rounds]
        print("%-32s %-22s %-22s %.3f" % (name, stat(s), stat(m), med(m) / med(s)))
    if log:
        print("# what was checked before the times were taken:")
        for line in open(log):
            if line.startswith("#"):
                print(line.rstrip())


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        run_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else ROUNDS)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(__doc__)
