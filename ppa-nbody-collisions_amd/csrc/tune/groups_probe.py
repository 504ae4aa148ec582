#!/usr/bin/env python3
"""Cost of group finding (nbody_get_groups, nbody_batch_get_groups): whole calls, sweeps per call, and the
sweep kernel next to neighbors_at's own form, the kernel that walks the same j stream, timed in the same run.

    python3 csrc/tune/groups_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                         (a run of its own; nothing else is traced with it)
    python3 csrc/tune/groups_probe.py host [reps]        whole Stepper.groups() / StepperBatch.groups() calls under the host
                                                         clock, with the sweeps each took, next to Stepper.neighbors()
    python3 csrc/tune/groups_probe.py report TRACE_DIR [HOST_LOG]
                                                         reads the kernel trace (csv) and prints the text of
                                                         profiles/groups_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps, with (link, radius_scale) = (0, 1) - the overlap predicate - and
two centre-only links chosen from the density rho of the state (over the bodies' bounding box): a body has rho * pi * link^2
others within `link` on average, 1.5 for "many small groups" and 7 for "one percolating group" (continuum percolation in the
plane sets in near 4.5).  A batch of 256 x 1024 with (0, 1) and with the many-small-groups link of its own density.
Every label array is checked equal to the host's (tests/group_cases.py: window_groups at N = 262144, model_groups for whole
systems of the batch) before a time is taken."""
import collections
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, BATCH_S, BATCH_N, STEPS = 262144, 256, 1024, 3
ROUNDS = 3                                                   # what `report` expects of `kernels`
MEAN_SMALL, MEAN_PERCOLATING = 1.5, 7.0                     # others within `link` of a body, on average


def centre_link(np, mean, P):
    """The link at which a body has `mean` others within reach on average, from the density over the bodies' bounding box."""
    area = float(np.prod(P.max(axis=0) - P.min(axis=0)))
    return float(np.sqrt(mean * area / (np.pi * len(P))))


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import group_cases as gc
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    d = st.download()
    P, R = gc.widen(d)
    n = d.numBodies
    cases = [("overlap (0, 1)", 0.0, 1.0),
             ("many small groups", centre_link(np, MEAN_SMALL, P), 0.0),
             ("one percolating group", centre_link(np, MEAN_PERCOLATING, P), 0.0)]
    for name, link, scale in cases:                         # equal to the host's labels before any time is taken
        got, want = st.groups(link, scale), gc.window_groups(P, R, link, scale)
        gc.assert_same(got, want, name)
        print("# N=%d after %d steps: n %d, %s: link %.6g scale %g -> %d links, %d groups, largest %d, %d sweeps; labels equal "
              "to the host's" % (N_ONE, STEPS, n, name, link, scale, want["links"], got["n_groups"], got["largest"], got["sweeps"]),
              flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    bodies = [nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)]
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload(bodies)
    batch.step(STEPS)
    bcases = [("batch overlap (0, 1)", 0.0, 1.0),
              ("batch many small groups", centre_link(np, MEAN_SMALL, gc.widen(batch.download(0))[0]), 0.0)]
    for name, link, scale in bcases:
        got = batch.groups(link, scale)
        for s in (0, 1, 127, 255):
            gc.assert_same(got[s], gc.model_groups(*gc.widen(batch.download(s)), link, scale), "%s, system %d" % (name, s))
        print("# %d x %d after %d steps, %s: link %.6g scale %g -> %d sweeps, %.1f groups per system, largest %d; 4 whole "
              "systems equal to the model" % (BATCH_S, BATCH_N, STEPS, name, link, scale, got[0]["sweeps"],
                                              np.mean([g["n_groups"] for g in got]), max(g["largest"] for g in got)), flush=True)
    return np, st, cases, batch, bcases


def run_kernels(rounds):
    np, st, cases, batch, bcases = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for name, link, scale in cases:                     # a neighbors_at launch opens every segment of the trace
            st.neighbors()
            plan.append((name, st.groups(link, scale)["sweeps"]))
        for name, link, scale in bcases:
            batch.neighbors()
            plan.append((name, batch.groups(link, scale)[0]["sweeps"]))
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
    timed(np, "Stepper.neighbors() N=%d" % N_ONE, st.neighbors, reps)
    for name, link, scale in cases:
        timed(np, "Stepper.groups(%.6g, %g) N=%d: %s" % (link, scale, N_ONE, name), lambda: st.groups(link, scale), reps,
              lambda g: {"sweeps": g["sweeps"], "n_groups": g["n_groups"], "largest": g["largest"]})
    timed(np, "StepperBatch.neighbors() %d x %d" % (BATCH_S, BATCH_N), batch.neighbors, reps)
    for name, link, scale in bcases:
        timed(np, "StepperBatch.groups(%.6g, %g) %d x %d: %s" % (link, scale, BATCH_S, BATCH_N, name),
              lambda: batch.groups(link, scale), reps, lambda g: {"sweeps": g[0]["sweeps"]})
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # segments: a neighbors_at launch (own form), then the launches of one groups call
    segs = []
    for _, name, ms in rows:
        if "neighbors_at" in name:
            segs.append({"neighbors": ms, "sweep": [], "other": collections.defaultdict(float)})
        elif segs and "groups_sweep" in name:
            segs[-1]["sweep"].append(ms)
        elif segs and ("groups_init" in name or "groups_flatten" in name):
            segs[-1]["other"]["init" if "groups_init" in name else "flatten"] += ms
    segs = [s for s in segs if s["sweep"]]
    names = ["overlap (0, 1)", "many small groups", "one percolating group", "batch overlap (0, 1)", "batch many small groups"]
    per_round = len(names)
    assert len(segs) >= per_round * (ROUNDS + 1), (len(segs), per_round)
    segs = segs[-per_round * ROUNDS:]                         # without the checks and the warm-up round
    print("# csrc/tune/groups_probe.py on one MI355X: groups_sweep next to neighbors_at's own form, fp32, the stock state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python groups_probe.py kernels 3 (a run of its own); ms, median over "
          "the sweeps of the rounds (spread); neighbors_at: the launch before each call")
    med = lambda v: sorted(v)[len(v) // 2]
    for k, name in enumerate(names):
        mine = segs[k::per_round]
        sweeps = [ms for s in mine for ms in s["sweep"]]
        first = [s["sweep"][0] for s in mine]
        last = [s["sweep"][-1] for s in mine]
        nb_ms = [s["neighbors"] for s in mine]
        print("%-26s sweeps per call %s  sweep %8.3f ms (%.3f; first %.3f, last %.3f)  neighbors_at %8.3f ms  sweep / neighbors_at %.3f  "
              "init + flatten %.3f ms" % (name, "/".join(str(len(s["sweep"])) for s in mine), med(sweeps), max(sweeps) - min(sweeps),
                                          med(first), med(last), med(nb_ms), med(sweeps) / med(nb_ms),
                                          med([sum(s["other"].values()) for s in mine])))
    if host_log:
        print("# whole calls under the host clock (groups_probe.py host 5; median of 5 after a warm-up):")
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
