#!/usr/bin/env python3
"""Cost of the bound-pair query (nbody_get_binaries, nbody_batch_get_binaries): binaries_walk next to
pair_counts with the one bin [0, sep2) - the same hot loop by counting - and encounters_walk at h = the time step - the shape
that evaluates everything for every pair - timed in the same run on the same state, and whole calls under the host clock.

    python3 csrc/tune/binary_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                         (a run of its own; nothing else is traced with it)
    python3 csrc/tune/binary_probe.py host [reps]        whole Stepper.binaries() / StepperBatch.binaries() calls under the
                                                         host clock, next to Stepper.pair_counts and Stepper.encounters
    python3 csrc/tune/binary_probe.py report TRACE_DIR [HOST_LOG]
                                                         reads the kernel trace (csv) and prints the text of
                                                         profiles/binaries_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps (the state of encounter_probe.py), at the largest separation of the
ladder 1, 2, 4, ... at which at most 1e-4 of the pairs are near, and at sep2 = +inf; a batch of 256 x 1024 after STEPS steps
at the same small separation.  The small-separation list is checked equal to the host's (tests/binary_cases.py:
window_binaries at N = 262144, model_binaries for whole systems of the batch) and near + coincident against pair_counts
before a time is taken.  A call for the counts only (out = NULL, cap = 0) takes no slot in the log: the same separation with and
without the list shows what the appends cost, an eighth of it what the near pairs cost.  At +inf every pair is near and the
bound ones are too many to list: the counts only."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
ROUNDS = 3                                                   # what `report` expects of `kernels`
NEAR_FRACTION = 1e-4
NAMES = ["sep, the list", "sep, counts only", "sep / 8, counts only", "sep2 = +inf, counts only", "batch, sep, the list"]


def counts_only(nb, np, bc, st, sep2):
    info = np.zeros(1, dtype=bc.INFO_DTYPE)
    status = nb.lib.nbody_get_binaries(st._ctx, float(sep2), None, 0, info.ctypes.data)
    assert status == 0, status
    return {f: int(info[f][0]) for f in bc.COUNTS}


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import binary_cases as bc
    cfg = nb.stock_config(particleCount=N_ONE)
    dt = float(np.float32(cfg.timestep))
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    state = bc.widen(st.download())
    n = len(state[2])
    total = n * (n - 1) // 2
    ladder = [float(2 ** k) for k in range(0, 13)]
    pc = st.pair_counts([0.0] + ladder)
    inside = np.cumsum(pc["counts"].astype(np.int64)) + int(pc["below"])
    sep = max([s for s, c in zip(ladder, inside) if c <= NEAR_FRACTION * total] or [ladder[0]])
    sep2 = sep * sep
    got = st.binaries(sep)
    bc.assert_same(got, bc.window_binaries(*state, sep), "N = %d at sep %g" % (N_ONE, sep))
    info = got[1]
    one = st.pair_counts([0.0, np.nextafter(sep2, np.inf)], squared=True)
    assert info["near"] + info["coincident"] == int(one["counts"][0])
    print("# N=%d after %d steps: n %d, %d pairs; sep %g (sep2 %g): near %d (%.3g of the pairs), bound %d, coincident %d, "
          "overlapping %d, approaching %d; max |v| %.4g; the list equal to the host's"
          % (N_ONE, STEPS, n, total, sep, sep2, info["near"], info["near"] / total, info["pairs"], info["coincident"],
             info["overlapping"], info["approaching"], float(np.abs(state[1]).max())), flush=True)
    eighth = counts_only(nb, np, bc, st, sep2 / 64.0)
    assert {f: eighth[f] for f in bc.COUNTS} == {f: bc.window_binaries(*state, sep / 8.0)[1][f] for f in bc.COUNTS}
    print("# sep / 8 = %g: near %d, bound %d; the counts equal to the host's" % (sep / 8.0, eighth["near"], eighth["pairs"]), flush=True)
    far = counts_only(nb, np, bc, st, np.inf)
    assert far["near"] == total - far["coincident"]
    print("# sep2 = +inf: near %d (every pair at d2 > 0), bound %d, coincident %d; the counts only, no list"
          % (far["near"], far["pairs"], far["coincident"]), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    bgot = batch.binaries(sep)
    for s in (0, 1, 127, 255):
        bc.assert_same(bgot[s], bc.model_binaries(*bc.widen(batch.download(s)), sep2), "batch, system %d" % s)
    print("# %d x %d after %d steps, sep %g: near %d, bound %d over the batch, at most %d in a system; 4 whole systems equal to "
          "the model" % (BATCH_S, BATCH_N, STEPS, sep, sum(g[1]["near"] for g in bgot), sum(g[1]["pairs"] for g in bgot),
                         max(g[1]["pairs"] for g in bgot)), flush=True)
    bcap = max(max(g[1]["pairs"] for g in bgot), 1)
    return nb, np, bc, st, batch, dt, sep, max(info["pairs"], 1), bcap


def run_kernels(rounds):
    nb, np, bc, st, batch, dt, sep, cap, bcap = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        st.pair_counts([0.0, sep])                          # pair_counts, one bin [0, sep2): opens a round
        st.encounters(dt, cap=0)                            # encounters_walk at h = dt, one walk (the list is not fetched twice:
        #                                                     cap = 0 with pairs > 0 walks again, so the report takes the first)
        st.binaries(sep, cap=cap)                           # a slot atomic and a record per bound pair
        counts_only(nb, np, bc, st, sep * sep)              # the lanes count: what the appends cost is the difference
        counts_only(nb, np, bc, st, sep * sep / 64.0)       # a sixty-fourth of the area: what the near pairs cost
        counts_only(nb, np, bc, st, np.inf)
        batch.binaries(sep, cap=bcap)
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
    nb, np, bc, st, batch, dt, sep, cap, bcap = workloads()
    enc_cap = max(st.encounters(dt)[1]["pairs"], 1)
    timed(np, "Stepper.pair_counts N=%d: one bin [0, %g)" % (N_ONE, sep), lambda: st.pair_counts([0.0, sep]), reps)
    timed(np, "Stepper.encounters N=%d: h = dt" % N_ONE, lambda: st.encounters(dt, cap=enc_cap), reps, lambda g: {"pairs": g[1]["pairs"]})
    timed(np, "Stepper.binaries N=%d: sep %g" % (N_ONE, sep), lambda: st.binaries(sep, cap=cap), reps,
          lambda g: {"pairs": g[1]["pairs"], "near": g[1]["near"]})
    timed(np, "Stepper.binaries N=%d: sep %g, cap = 0 (the counts, then the list: two walks)" % (N_ONE, sep),
          lambda: st.binaries(sep, cap=0), reps)
    timed(np, "nbody_get_binaries N=%d: sep %g, the counts only" % (N_ONE, sep), lambda: counts_only(nb, np, bc, st, sep * sep), reps,
          lambda c: {"pairs": c["pairs"], "near": c["near"]})
    timed(np, "nbody_get_binaries N=%d: sep2 = +inf, the counts only" % N_ONE, lambda: counts_only(nb, np, bc, st, np.inf), reps,
          lambda c: {"pairs": c["pairs"], "near": c["near"]})
    timed(np, "StepperBatch.binaries %d x %d: sep %g" % (BATCH_S, BATCH_N, sep), lambda: batch.binaries(sep, cap=bcap), reps)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # a round: one pair_counts launch, encounters_walk (the first of the call's launches), then the three binaries_walk
    # launches in the order of NAMES
    rounds = []
    for _, name, ms in rows:
        if "pair_counts" in name:
            rounds.append({"pairs": ms, "enc": [], "bin": []})
        elif rounds and "encounters_walk" in name:
            rounds[-1]["enc"].append(ms)
        elif rounds and "binaries_walk" in name:
            rounds[-1]["bin"].append(ms)
    rounds = [r for r in rounds if len(r["bin"]) == len(NAMES) and r["enc"]]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    pairs = [r["pairs"] for r in rounds]
    enc = [r["enc"][0] for r in rounds]
    print("# csrc/tune/binary_probe.py on one MI355X: binaries_walk next to pair_counts (one bin [0, sep2)) and encounters_walk at "
          "h = dt, fp32, the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python binary_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-28s %8.3f ms (%.3f)" % ("pair_counts, one bin", med(pairs), max(pairs) - min(pairs)))
    print("%-28s %8.3f ms (%.3f)" % ("encounters_walk, h = dt", med(enc), max(enc) - min(enc)))
    for k, name in enumerate(NAMES):
        mine = [r["bin"][k] for r in rounds]
        line = "%-28s %8.3f ms (%.3f)" % (name, med(mine), max(mine) - min(mine))
        if k < 4:
            line += "  binaries_walk / pair_counts %.3f  / encounters_walk %.3f" % (med(mine) / med(pairs), med(mine) / med(enc))
        print(line)
    if host_log:
        print("# whole calls under the host clock (binary_probe.py host 5; median of 5 after a warm-up), and what was found:")
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
