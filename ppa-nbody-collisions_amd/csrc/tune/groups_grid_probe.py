#!/usr/bin/env python3
"""Cost of the groups on the cell list (nbody_get_groups_grid, nbody_batch_get_groups_grid) next to the
triangular walk of nbody_get_groups, both timed in the same run on the state and the links of
groups_probe.py.

    python3 csrc/tune/groups_grid_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                              (a run of its own; nothing else is traced with it)
    python3 csrc/tune/groups_grid_probe.py host [reps]        whole Stepper.groups() / StepperBatch.groups() calls, with and
                                                              without a grid, under the host clock: a warm-up, then the
                                                              median of `reps`
    python3 csrc/tune/groups_grid_probe.py report TRACE_DIR HOST_LOG
                                                              reads the kernel trace (csv) and the output of `host`, which
                                                              names the calls, and prints the text of
                                                              profiles/groups_grid_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps, the three (link, radius_scale) of groups_probe.py, and its batch
of 256 x 1024.  Grids: `matched` = groups_grid(field, link, radius_scale, the state's MEDIAN radius); and the known bad
cases, `largest` = groups_grid with the LARGEST radius instead, and `1 x 1`.  The field is the configuration's, widened to the
bodies' bounding box where a body has left it, so that nothing is outside: every label array is checked equal to
Stepper.groups() without a grid in the same run before any time is taken."""
import collections
import csv
import glob
import json
import os
import sys

import groups_probe as gp

ROOT = gp.ROOT
ROUNDS = 3                                                   # what `report` expects of `kernels`
GRIDS = ("matched", "largest", "1 x 1")


def window_cells(np, P, R, grid, link, scale):
    """The cells of every row's window (tests/groups_grid_cases.py restates the rule) -> (the widest, the mean)."""
    import within_cases as wc
    g = grid[0]
    a = np.abs(R)
    S = (scale * (a + a)) + link
    c0, c1 = wc._span((P[:, 0] - g["x0"]) * g["sx"], S * g["sx"], int(g["nx"]))
    r0, r1 = wc._span((P[:, 1] - g["y0"]) * g["sy"], S * g["sy"], int(g["ny"]))
    cells = np.maximum(c1 - c0 + 1, 0) * np.maximum(r1 - r0 + 1, 0)
    return int(cells.max()), float(cells.mean())


def workloads():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import group_cases as gc
    cfg = nb.stock_config(particleCount=gp.N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(gp.STEPS)
    d = st.download()
    P, R = gc.widen(d)
    n = d.numBodies
    field = (max(float(cfg.fieldWidth), float(np.abs(P[:, 0]).max()) * 1.001), max(float(cfg.fieldHeight), float(np.abs(P[:, 1]).max()) * 1.001))
    median, largest = float(np.median(R)), float(np.abs(R).max())
    print("# N=%d after %d steps: n %d, radii median %.6g, largest %.6g, field %r" % (gp.N_ONE, gp.STEPS, n, median, largest, field), flush=True)
    cases = []
    for name, link, scale in [("overlap (0, 1)", 0.0, 1.0), ("many small groups", gp.centre_link(np, gp.MEAN_SMALL, P), 0.0),
                              ("one percolating group", gp.centre_link(np, gp.MEAN_PERCOLATING, P), 0.0)]:
        grids = {"matched": nb.groups_grid(field, link, scale, median), "largest": nb.groups_grid(field, link, scale, largest),
                 "1 x 1": nb.make_grid(1, 1, (-field[0], field[0], -field[1], field[1]))}
        want = st.groups(link, scale)
        for kind in GRIDS:                                  # equal to the triangular walk's labels before any time is taken
            got = st.groups(link, scale, grid=grids[kind])
            assert got["outside"] == 0 and got["label"].tobytes() == want["label"].tobytes(), (name, kind)
            assert (got["n_groups"], got["largest"]) == (want["n_groups"], want["largest"]), (name, kind)
            widest, mean = window_cells(np, P, R, grids[kind], link, scale)
            print("# %s, link %.6g scale %g, grid %s %d x %d: %d groups, largest %d, %d sweeps (triangular %d); window in cells: "
                  "widest %d, mean %.2f; labels equal to Stepper.groups()" % (name, link, scale, kind, grids[kind]["nx"][0], grids[kind]["ny"][0],
                                                                              got["n_groups"], got["largest"], got["sweeps"], want["sweeps"],
                                                                              widest, mean), flush=True)
        cases.append((name, link, scale, grids))
    bcfg = nb.stock_config(particleCount=gp.BATCH_N)
    bodies = [nb.init_bodies(bcfg, seed=100 + s) for s in range(gp.BATCH_S)]
    batch = nb.StepperBatch(gp.BATCH_S, gp.BATCH_N, cfg=bcfg)
    batch.upload(bodies)
    batch.step(gp.STEPS)
    P0, R0 = gc.widen(batch.download(0))
    reach = max(float(np.abs(gc.widen(batch.download(s))[0]).max()) for s in range(gp.BATCH_S)) * 1.001
    bfield = (max(float(bcfg.fieldWidth), reach), max(float(bcfg.fieldHeight), reach))
    bcases = []
    for name, link, scale in [("batch overlap (0, 1)", 0.0, 1.0), ("batch many small groups", gp.centre_link(np, gp.MEAN_SMALL, P0), 0.0)]:
        grid = nb.groups_grid(bfield, link, scale, float(np.median(R0)), most=int(np.sqrt((1 << 22) // gp.BATCH_S)))
        want, got = batch.groups(link, scale), batch.groups(link, scale, grid=grid)
        for s in range(gp.BATCH_S):
            assert got[s]["outside"] == 0 and got[s]["label"].tobytes() == want[s]["label"].tobytes(), (name, s)
        print("# %d x %d after %d steps, %s: link %.6g scale %g, grid %d x %d -> %d sweeps (triangular %d); every system's labels "
              "equal to StepperBatch.groups()" % (gp.BATCH_S, gp.BATCH_N, gp.STEPS, name, link, scale, grid["nx"][0], grid["ny"][0],
                                                  got[0]["sweeps"], want[0]["sweeps"]), flush=True)
        bcases.append((name, link, scale, {"matched": grid}))
    return np, st, cases, batch, bcases


def calls_of(st, cases, batch, bcases):
    """(label, callable) of every timed call, the triangular walk before the grids of each link."""
    out = []
    for handle, group, sweeps in ((st, cases, lambda g: g["sweeps"]), (batch, bcases, lambda g: g[0]["sweeps"])):
        for name, link, scale, grids in group:
            out.append((name + " | triangular", lambda h=handle, l=link, s=scale: h.groups(l, s), sweeps))
            for kind, grid in grids.items():
                out.append(("%s | %s" % (name, kind), lambda h=handle, l=link, s=scale, g=grid: h.groups(l, s, grid=g), sweeps))
    return out


def run_kernels(rounds):
    np, st, cases, batch, bcases = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for label, call, sweeps in calls_of(st, cases, batch, bcases):
            plan.append((label, sweeps(call())))
    print("PLAN " + json.dumps(plan), flush=True)
    st.close()
    batch.close()


def run_host(reps):
    np, st, cases, batch, bcases = workloads()
    for label, call, sweeps in calls_of(st, cases, batch, bcases):
        gp.timed(np, label, call, reps, lambda g: {"sweeps": sweeps(g)})
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # a call ends with its groups_flatten; what came before belongs to it
    calls, cur = [], {"sweep": [], "grid": False, "other": collections.defaultdict(float)}
    for _, name, ms in rows:
        if "groups_grid_sweep" in name:
            cur["sweep"].append(ms)
            cur["grid"] = True
        elif "groups_sweep" in name:
            cur["sweep"].append(ms)
        elif "groups_flatten" in name:
            cur["other"]["init + flatten"] += ms
            calls.append(cur)
            cur = {"sweep": [], "grid": False, "other": collections.defaultdict(float)}
        elif "groups_init" in name:
            cur["other"]["init + flatten"] += ms
        elif "cells_" in name:                               # the list's stages and cells_gather
            cur["other"]["list + gather"] += ms
    host = [line for line in open(host_log)]
    labels = [json.loads(line)["call"] for line in host if line.startswith("{")]
    assert labels, "the host log names the calls of one round"
    per_round = len(labels)
    assert len(calls) >= per_round * (ROUNDS + 1), (len(calls), per_round)
    calls = calls[-per_round * ROUNDS:]                      # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]
    print("# csrc/tune/groups_grid_probe.py on one MI355X: groups_grid_sweep next to groups_sweep, fp32, the stock state after %d steps" % gp.STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python groups_grid_probe.py kernels 3 (a run of its own); ms, median over "
          "the sweeps of the rounds (spread); list + gather: the cell list's stages and cells_gather of one call")
    for k, label in enumerate(labels):
        mine = calls[k::per_round]
        assert all(c["grid"] == ("triangular" not in label) for c in mine), label
        sweeps = [ms for c in mine for ms in c["sweep"]]
        print("%-44s sweeps per call %-8s sweep %8.3f ms (%.3f; first %.3f, last %.3f)  all sweeps of a call %8.3f ms  list + gather %.3f ms  "
              "init + flatten %.3f ms" % (label, "/".join(str(len(c["sweep"])) for c in mine), med(sweeps), max(sweeps) - min(sweeps),
                                          med([c["sweep"][0] for c in mine]), med([c["sweep"][-1] for c in mine]),
                                          med([sum(c["sweep"]) for c in mine]), med([c["other"]["list + gather"] for c in mine]),
                                          med([c["other"]["init + flatten"] for c in mine])))
    print("# the share of a sweep spent by its slowest workgroup: not shown by a kernel trace, not measured")
    print("# whole calls under the host clock (groups_grid_probe.py host 5; a warm-up, then the median of 5):")
    for line in host:
        if line.startswith(("{", "#")):
            print(line.rstrip())


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    if mode == "kernels":
        run_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else ROUNDS)
    elif mode == "host":
        run_host(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
