#!/usr/bin/env python3
"""Cost of the group energies (nbody_get_group_potential, nbody_batch_get_group_potential): the
group_potential kernel next to field_at's own form (the potential walk without labels) and groups_sweep (the triangular
pair walk of the same call), all launched in the same run, and whole calls under the host clock.

    python3 csrc/tune/group_energy_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                               (a run of its own; nothing else is traced with it)
    python3 csrc/tune/group_energy_probe.py host [reps]        whole group_potential() / group_energies() calls under the host
                                                               clock, next to groups() and field()
    python3 csrc/tune/group_energy_probe.py report TRACE_DIR [HOST_LOG]
                                                               reads the kernel trace (csv) and prints the text of
                                                               profiles/group_energy_probe.txt

Shapes: those of groups_probe.py - N = 262144 fp32, the stock state after 3 steps, with (link, radius_scale) = (0, 1) and
the two centre-only links of 1.5 and 7 others within reach on average (many small groups; one percolating group) - and the
batch of 256 x 1024 with (0, 1) and its own many-small-groups link.
Checked before any time is taken: the labels equal to groups()' for the same arguments; every row of every group of fewer
than BIG_GROUP members against the long-double oracle and its bound (tests/group_energy_cases.py, the group's members
alone: the pairs of other groups are not part of the sum); of a larger group, whose oracle is n_g^2 long-double terms,
SAMPLE rows spread over its members against all of them."""
import collections
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from groups_probe import BATCH_N, BATCH_S, MEAN_PERCOLATING, MEAN_SMALL, N_ONE, STEPS, centre_link  # noqa: E402

ROUNDS = 3                                                   # what `report` expects of `kernels`
BIG_GROUP, SAMPLE = 4096, 512


def check(np, ge, got, want_label, P, M, what):
    """Labels, then every row (or SAMPLE rows of a group of BIG_GROUP members or more) against the oracle's bound."""
    assert np.array_equal(got["label"], want_label), what
    label, phi = got["label"], got["phi"]
    n = len(label)
    size = np.bincount(label, minlength=n)
    alone = size[label] == 1
    assert (ge.bits(phi[alone]) == ge.bits(np.float64(-0.0))).all(), what
    order = np.argsort(label, kind="stable")                 # members of a group next to each other, ascending
    order = order[~alone[order]]
    starts = np.flatnonzero(np.r_[True, np.diff(label[order]) != 0]) if len(order) else order   # nothing but singletons: no group
    worst, rows, coincident = 0.0, int(alone.sum()), 0
    for a, b in zip(starts, np.r_[starts[1:], len(order)]):
        members = order[a:b]
        pick = None if len(members) < BIG_GROUP else np.linspace(0, len(members) - 1, SAMPLE).astype(np.int64)
        exact, coin, sz = ge.exact_group_phi(P[members], M[members], np.zeros(len(members), dtype=np.int64), pick)
        r = ge.phi_errors(phi[members] if pick is None else phi[members][pick], exact, sz)
        worst = max(worst, float(r.max()))
        rows += len(r)
        coincident += coin if pick is None else 0
    assert worst <= 1.0 and np.isfinite(phi).all(), (what, worst)
    if size.max() < BIG_GROUP:
        assert coincident == got["coincident"], (what, coincident, got["coincident"])
    return "%d of %d rows within the bound (worst error / bound %.3f), coincident %d" % (rows, n, worst, got["coincident"])


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import group_cases as gc
    import group_energy_cases as ge
    ge.require_long_double()
    cfg = nb.stock_config(particleCount=N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(STEPS)
    d = st.download()
    P, R = gc.widen(d)
    M = np.asarray(d.Masses, dtype=np.float64)
    n = d.numBodies
    cases = [("overlap (0, 1)", 0.0, 1.0),
             ("many small groups", centre_link(np, MEAN_SMALL, P), 0.0),
             ("one percolating group", centre_link(np, MEAN_PERCOLATING, P), 0.0)]
    for name, link, scale in cases:
        got = st.group_potential(link, scale)
        said = check(np, ge, got, st.groups(link, scale)["label"], P, M, name)
        print("# N=%d after %d steps: n %d, %s: link %.6g scale %g -> %d groups, largest %d, %d sweeps; labels equal to groups(), %s"
              % (N_ONE, STEPS, n, name, link, scale, got["n_groups"], got["largest"], got["sweeps"], said), flush=True)
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    batch.step(STEPS)
    bcases = [("batch overlap (0, 1)", 0.0, 1.0),
              ("batch many small groups", centre_link(np, MEAN_SMALL, gc.widen(batch.download(0))[0]), 0.0)]
    for name, link, scale in bcases:
        got, grp = batch.group_potential(link, scale), batch.groups(link, scale)
        for s in range(BATCH_S):
            assert np.array_equal(got[s]["label"], grp[s]["label"]), (name, s)
        said = []
        for s in (0, 1, 127, 255):
            b = batch.download(s)
            said.append(check(np, ge, got[s], grp[s]["label"], gc.widen(b)[0], np.asarray(b.Masses, dtype=np.float64), "%s, system %d" % (name, s)))
        print("# %d x %d after %d steps, %s: link %.6g scale %g -> %d sweeps, %.1f groups per system, largest %d; every system's labels "
              "equal to groups(); system 0: %s" % (BATCH_S, BATCH_N, STEPS, name, link, scale, got[0]["sweeps"],
                                                   np.mean([g["n_groups"] for g in got]), max(g["largest"] for g in got), said[0]), flush=True)
    return np, st, cases, batch, bcases


def run_kernels(rounds):
    np, st, cases, batch, bcases = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for name, link, scale in cases:                     # a field_at launch (own form) opens every segment of the trace
            st.field()
            plan.append((name, st.group_potential(link, scale)["sweeps"]))
        for name, link, scale in bcases:
            batch.field()
            plan.append((name, batch.group_potential(link, scale)[0]["sweeps"]))
    print("PLAN " + json.dumps(plan), flush=True)
    st.close()
    batch.close()


def timed(np, name, call, reps):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"call": name, "reps": reps, "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3),
                      "ms_max": round(max(ms), 3)}), flush=True)


def run_host(reps):
    np, st, cases, batch, bcases = workloads()
    timed(np, "Stepper.field() N=%d" % N_ONE, st.field, reps)
    for name, link, scale in cases:
        what = "(%.6g, %g) N=%d: %s" % (link, scale, N_ONE, name)
        timed(np, "Stepper.groups" + what, lambda: st.groups(link, scale), reps)
        timed(np, "Stepper.group_potential" + what, lambda: st.group_potential(link, scale), reps)
        timed(np, "Stepper.group_energies" + what, lambda: st.group_energies(link, scale), reps)
    timed(np, "StepperBatch.field() %d x %d" % (BATCH_S, BATCH_N), batch.field, reps)
    for name, link, scale in bcases:
        what = "(%.6g, %g) %d x %d: %s" % (link, scale, BATCH_S, BATCH_N, name)
        timed(np, "StepperBatch.groups" + what, lambda: batch.groups(link, scale), reps)
        timed(np, "StepperBatch.group_potential" + what, lambda: batch.group_potential(link, scale), reps)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # segments: a field_at launch (own form), then the launches of one group_potential call
    segs = []
    for _, name, ms in rows:
        if "field_at" in name:
            segs.append({"field": ms, "sweep": [], "potential": []})
        elif segs and "groups_sweep" in name:
            segs[-1]["sweep"].append(ms)
        elif segs and "group_potential" in name:
            segs[-1]["potential"].append(ms)
    segs = [s for s in segs if s["potential"]]
    names = ["overlap (0, 1)", "many small groups", "one percolating group", "batch overlap (0, 1)", "batch many small groups"]
    per_round = len(names)
    assert len(segs) >= per_round * (ROUNDS + 1), (len(segs), per_round)
    segs = segs[-per_round * ROUNDS:]                         # without the checks and the warm-up round
    assert all(len(s["potential"]) == 1 for s in segs)
    print("# csrc/tune/group_energy_probe.py on one MI355X: group_potential next to field_at's own form and groups_sweep, fp32, the stock "
          "state after %d steps" % STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python group_energy_probe.py kernels 3 (a run of its own); ms, median over "
          "the rounds (spread); field_at: the launch before each call; groups_sweep: the sweeps of the same call")
    med = lambda v: sorted(v)[len(v) // 2]
    for k, name in enumerate(names):
        mine = segs[k::per_round]
        pot = [s["potential"][0] for s in mine]
        sweeps = [ms for s in mine for ms in s["sweep"]]
        fld = [s["field"] for s in mine]
        print("%-26s group_potential %8.3f ms (%.3f)  field_at %8.3f ms (%.3f)  groups_sweep %8.3f ms (%.3f; %s per call)  "
              "/ field_at %.3f  / groups_sweep %.3f" % (name, med(pot), max(pot) - min(pot), med(fld), max(fld) - min(fld), med(sweeps),
                                                       max(sweeps) - min(sweeps), "/".join(str(len(s["sweep"])) for s in mine),
                                                       med(pot) / med(fld), med(pot) / med(sweeps)))
    if host_log:
        print("# whole calls under the host clock (group_energy_probe.py host 5; median of 5 after a warm-up):")
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
