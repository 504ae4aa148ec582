#!/usr/bin/env python3
"""Cost of the encounter query (nbody_get_encounters, nbody_batch_get_encounters): encounters_walk next to
neighbors_at's own-form kernel and groups_sweep at (link, radius_scale) = (0, 1) - the kernel that walks the same triangle -
timed in the same run on the same state, and whole calls under the host clock.

    python3 csrc/tune/encounter_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                            (a run of its own; nothing else is traced with it)
    python3 csrc/tune/encounter_probe.py host [reps]        whole Stepper.encounters() / StepperBatch.encounters() calls under
                                                            the host clock, next to Stepper.groups(0, 1) and Stepper.neighbors()
    python3 csrc/tune/encounter_probe.py report TRACE_DIR [HOST_LOG]
                                                            reads the kernel trace (csv) and prints the text of
                                                            profiles/encounter_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps (the state of groups_probe.py and pairs_probe.py), with the horizon
0, the time step and ten time steps; a batch of 256 x 1024 after STEPS steps with the time step.  Every list is checked equal to
the host's (tests/encounter_cases.py: window_encounters at N = 262144, model_encounters for whole systems of the batch), and
info.now at h = 0 against half the overlaps of neighbors(), before a time is taken.  Every call is given room for its list, so
a call is one walk."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
ROUNDS = 3                                                   # what `report` expects of `kernels`
MAX_CANDIDATES = 3e8                                         # pairs the host's check may evaluate per horizon (about a minute)
NAMES = ["h = 0", "h = dt", "h = 10 dt", "batch h = dt"]


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import encounter_cases as ec
    cfg = nb.stock_config(particleCount=N_ONE)
    dt = float(np.float32(cfg.timestep))
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    state = ec.widen(st.download())
    n = len(state[2])
    cases = []
    for name, h in zip(NAMES[:3], (0.0, dt, 10.0 * dt)):
        got = st.encounters(h)
        info = got[1]
        # equal to the host's list before any time is taken - where the host's window is affordable: a horizon over which the
        # fastest body crosses a good part of the field makes nearly every pair a candidate
        reach = 2.0 * float(state[2].max()) + 2.0 * float(np.abs(state[1][:, 0]).max()) * h
        candidates = 0.5 * n * n * min(1.0, 2.0 * reach / float(np.ptp(state[0][:, 0])))
        if candidates <= MAX_CANDIDATES:
            ec.assert_same(got, ec.window_encounters(*state, h), name)
            checked = "the list equal to the host's (about %.2g candidate pairs)" % candidates
        else:
            assert info["pairs"] == len(got[0]) and (np.diff(got[0]["t"]) >= 0).all()
            checked = "the list NOT compared with the host's (about %.2g candidate pairs)" % candidates
        if h == 0.0:
            assert 2 * info["now"] == int(st.neighbors()["overlaps"].sum())
        print("# N=%d after %d steps: n %d, %s (%.9g s): pairs %d, now %d, end %d, missed %d of %d pairs; max |v| %.4g; "
              "%s" % (N_ONE, STEPS, n, name, h, info["pairs"], info["now"], info["end"], info["missed"], n * (n - 1) // 2,
                      float(np.abs(state[1]).max()), checked), flush=True)
        cases.append((name, h, info["pairs"]))
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    got = batch.encounters(dt)
    for s in (0, 1, 127, 255):
        ec.assert_same(got[s], ec.model_encounters(*ec.widen(batch.download(s)), dt), "batch, system %d" % s)
    print("# %d x %d after %d steps, h = dt: pairs %d, now %d, end %d, missed %d over the batch, at most %d in a system; 4 whole "
          "systems equal to the model" % (BATCH_S, BATCH_N, STEPS, *[sum(g[1][f] for g in got) for f in ("pairs", "now", "end", "missed")],
                                          max(g[1]["pairs"] for g in got)), flush=True)
    bcap = max(max(g[1]["pairs"] for g in got), 1)
    return np, st, cases, batch, dt, bcap


def run_kernels(rounds):
    np, st, cases, batch, dt, bcap = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        st.neighbors()                                      # neighbors_at, own form, on the same state, in the same round
        plan.append(st.groups(0.0, 1.0)["sweeps"])          # groups_sweep
        for name, h, pairs in cases:
            st.encounters(h, cap=max(pairs, 1))
        batch.encounters(dt, cap=bcap)
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
    np, st, cases, batch, dt, bcap = workloads()
    timed(np, "Stepper.neighbors() N=%d" % N_ONE, lambda: st.neighbors(), reps)
    timed(np, "Stepper.groups(0, 1) N=%d" % N_ONE, lambda: st.groups(0.0, 1.0), reps, lambda g: {"sweeps": g["sweeps"]})
    for name, h, pairs in cases:
        timed(np, "Stepper.encounters N=%d: %s" % (N_ONE, name), lambda: st.encounters(h, cap=max(pairs, 1)), reps,
              lambda g: {"pairs": g[1]["pairs"]})
    timed(np, "Stepper.encounters N=%d: h = dt, cap = 0 (the counts, then the list: two walks)" % N_ONE,
          lambda: st.encounters(cases[1][1], cap=0), reps)
    timed(np, "StepperBatch.encounters %d x %d: h = dt" % (BATCH_S, BATCH_N), lambda: batch.encounters(dt, cap=bcap), reps)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # a round: one neighbors_at launch, the sweeps of the one groups call, then the four encounters_walk launches in the order of NAMES
    rounds = []
    for _, name, ms in rows:
        if "neighbors_at" in name:
            rounds.append({"near": ms, "sweep": [], "enc": []})
        elif rounds and "groups_sweep" in name:
            rounds[-1]["sweep"].append(ms)
        elif rounds and "encounters_walk" in name:
            rounds[-1]["enc"].append(ms)
    rounds = [r for r in rounds if len(r["enc"]) == len(NAMES) and r["sweep"]]
    assert len(rounds) >= ROUNDS + 1, len(rounds)
    rounds = rounds[-ROUNDS:]                               # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    sweeps = [ms for r in rounds for ms in r["sweep"]]
    near = [r["near"] for r in rounds]
    print("# csrc/tune/encounter_probe.py on one MI355X: encounters_walk next to neighbors_at (own form) and groups_sweep at (0, 1), fp32, "
          "the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python encounter_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread = max - min)")
    print("%-22s %8.3f ms (%.3f)" % ("neighbors_at, own form", med(near), max(near) - min(near)))
    print("%-22s %8.3f ms (%.3f)  %s sweeps per call" % ("groups_sweep (0, 1)", med(sweeps), max(sweeps) - min(sweeps),
                                                        "/".join(str(len(r["sweep"])) for r in rounds)))
    for k, name in enumerate(NAMES):
        mine = [r["enc"][k] for r in rounds]
        line = "%-22s %8.3f ms (%.3f)" % (name, med(mine), max(mine) - min(mine))
        if k < 3:
            line += "  encounters_walk / groups_sweep %.3f  / neighbors_at %.3f" % (med(mine) / med(sweeps), med(mine) / med(near))
        print(line)
    if host_log:
        print("# whole calls under the host clock (encounter_probe.py host 5; median of 5 after a warm-up), and what was found:")
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
