#!/usr/bin/env python3
"""Cost of the pair-separation counts (nbody_get_pair_counts, nbody_batch_get_pair_counts): the kernel for
three sets of edges next to groups_sweep at (link, radius_scale) = (0, 1) - the kernel that walks the same triangle - timed
in the same run on the same state, and whole calls under the host clock.

    python3 csrc/tune/pairs_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                        (a run of its own; nothing else is traced with it)
    python3 csrc/tune/pairs_probe.py host [reps]        whole Stepper.pair_counts() / StepperBatch.pair_counts() calls under
                                                        the host clock, next to Stepper.groups(0, 1)
    python3 csrc/tune/pairs_probe.py report TRACE_DIR [HOST_LOG]
                                                        reads the kernel trace (csv) and prints the text of
                                                        profiles/pairs_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps (the state of groups_probe.py), own form, 32 logarithmic bins:
  (a) sparse       top at the sparse centre link of groups_probe.py (1.5 others within reach of a body on average), three
                   decades of length below it;
  (b) percolating  top at its percolating link (7 others within reach), three decades below it;
  (c) everything   31 bins up to the percolating link and a last bin to +inf: every pair takes the search and an LDS atomic.
A batch of 256 x 1024 with (a)-like and (c)-like edges from the density of its first system.
Every histogram is checked equal to the host's (tests/pair_cases.py: window_pair_counts at N = 262144 - for (c) over the
finite edges, the last bin being what is left of the pairs, none of which is NaN or +inf in this state; model_pair_counts
for whole systems of the batch) before a time is taken."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
ROUNDS = 3                                                   # what `report` expects of `kernels`
BINS = 32
MEAN_SMALL, MEAN_PERCOLATING = 1.5, 7.0                     # others within reach of a body, on average (groups_probe.py)
NAMES = ["(a) sparse", "(b) percolating", "(c) everything", "batch (a) sparse", "batch (c) everything"]


def centre_link(np, mean, P):
    """groups_probe.py's: the length at which a body has `mean` others within reach on average."""
    area = float(np.prod(P.max(axis=0) - P.min(axis=0)))
    return float(np.sqrt(mean * area / (np.pi * len(P))))


def edge_sets(np, small, percolating):
    """-> (a), (b), (c) as squared edges, BINS bins each."""
    log = lambda top, k: np.geomspace(top / 1000.0, top, k) ** 2
    return log(small, BINS + 1), log(percolating, BINS + 1), np.concatenate([log(percolating, BINS), [np.inf]])


def in_range(res):
    return (res["below"] + int(res["counts"].sum())) / max(res["pairs"], 1)


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import pair_cases as pc
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    P, _ = pc.widen(st.download())
    n = len(P)
    small, percolating = centre_link(np, MEAN_SMALL, P), centre_link(np, MEAN_PERCOLATING, P)
    cases = list(zip(NAMES[:3], edge_sets(np, small, percolating)))
    for name, e2 in cases:                                  # equal to the host's counts before any time is taken
        got = st.pair_counts(e2, squared=True)
        if np.isfinite(e2[-1]):
            pc.assert_same(got, pc.window_pair_counts(P, e2), name)
        else:                                               # a finite state: what is not below the last finite edge is in the last bin
            want = pc.window_pair_counts(P, e2[:-1])
            assert got["counts"][:-1].tolist() == want["counts"].tolist() and got["below"] == want["below"], name
            assert got["rest"] == 0 and int(got["counts"][-1]) == want["rest"] and got["pairs"] == want["pairs"], name
        print("# N=%d after %d steps: n %d, %s: edges %.6g .. %.6g (lengths) -> below %d, in the bins %d, rest %d of %d pairs, in "
              "range %.3e; counts equal to the host's" % (N_ONE, STEPS, n, name, np.sqrt(e2[0]), np.sqrt(e2[-1]), got["below"],
                                                          int(got["counts"].sum()), got["rest"], got["pairs"], in_range(got)), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    P0, _ = pc.widen(batch.download(0))
    ba, _, bc = edge_sets(np, centre_link(np, MEAN_SMALL, P0), centre_link(np, MEAN_PERCOLATING, P0))
    bcases = [(NAMES[3], ba), (NAMES[4], bc)]
    for name, e2 in bcases:
        got = batch.pair_counts(e2, squared=True)
        for s in (0, 1, 127, 255):
            pc.assert_same(got[s], pc.model_pair_counts(pc.widen(batch.download(s))[0], e2), "%s, system %d" % (name, s))
        print("# %d x %d after %d steps, %s: edges %.6g .. %.6g (lengths) -> in range %.3e over the batch; 4 whole systems equal "
              "to the model" % (BATCH_S, BATCH_N, STEPS, name, np.sqrt(e2[0]), np.sqrt(e2[-1]),
                                sum(g["below"] + int(g["counts"].sum()) for g in got) / sum(g["pairs"] for g in got)), flush=True)
    return np, st, cases, batch, bcases


def run_kernels(rounds):
    np, st, cases, batch, bcases = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for name, e2 in cases:
            st.pair_counts(e2, squared=True)
        plan.append(st.groups(0.0, 1.0)["sweeps"])          # groups_sweep on the same state, in the same round
        for name, e2 in bcases:
            batch.pair_counts(e2, squared=True)
    print("PLAN " + json.dumps(plan), flush=True)
    st.close()
    batch.close()


def timed(np, name, call, reps, extra=None):
    out = call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    r = {"call": name, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}
    if extra:
        r.update(extra(out))
    print(json.dumps(r), flush=True)
    return r


def run_host(reps):
    np, st, cases, batch, bcases = workloads()
    timed(np, "Stepper.groups(0, 1) N=%d" % N_ONE, lambda: st.groups(0.0, 1.0), reps, lambda g: {"sweeps": g["sweeps"]})
    for name, e2 in cases:
        timed(np, "Stepper.pair_counts N=%d: %s" % (N_ONE, name), lambda: st.pair_counts(e2, squared=True), reps,
              lambda g: {"in_range": in_range(g)})
    for name, e2 in bcases:
        timed(np, "StepperBatch.pair_counts %d x %d: %s" % (BATCH_S, BATCH_N, name), lambda: batch.pair_counts(e2, squared=True), reps)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # rounds: five pair_counts launches in the order of NAMES, the sweeps of the one groups call between the third and the fourth
    rounds = [{"pairs": [], "sweep": []}]
    for _, name, ms in rows:
        if "pair_counts" in name:
            if len(rounds[-1]["pairs"]) == len(NAMES):
                rounds.append({"pairs": [], "sweep": []})
            rounds[-1]["pairs"].append(ms)
        elif "groups_sweep" in name:
            rounds[-1]["sweep"].append(ms)
    rounds = [r for r in rounds if len(r["pairs"]) == len(NAMES) and r["sweep"]]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    sweeps = [ms for r in rounds for ms in r["sweep"]]
    print("# csrc/tune/pairs_probe.py on one MI355X: pair_counts next to groups_sweep at (0, 1), fp32, the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python pairs_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-22s %8.3f ms (%.3f)  %s sweeps per call" % ("groups_sweep (0, 1)", med(sweeps), max(sweeps) - min(sweeps),
                                                        "/".join(str(len(r["sweep"])) for r in rounds)))
    for k, name in enumerate(NAMES):
        mine = [r["pairs"][k] for r in rounds]
        line = "%-22s %8.3f ms (%.3f)" % (name, med(mine), max(mine) - min(mine))
        if k < 3:
            line += "  pair_counts / groups_sweep %.3f" % (med(mine) / med(sweeps))
        print(line)
    if host_log:
        print("# whole calls under the host clock (pairs_probe.py host 5; median of 5 after a warm-up), and what was counted:")
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
