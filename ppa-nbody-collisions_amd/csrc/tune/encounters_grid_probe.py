#!/usr/bin/env python3
"""Cost of the encounters on the cell list (nbody_get_encounters_grid, nbody_batch_get_encounters_grid) next to
the triangular tile walk of nbody_get_encounters, timed in the same run on the state of encounter_probe.py.

    python3 csrc/tune/encounters_grid_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                                  (a run of its own; nothing else is traced with it)
    python3 csrc/tune/encounters_grid_probe.py host [rounds]      whole calls under the host clock around the synchronising
                                                                  call: a warm-up, then `rounds` rounds, the grid form
                                                                  alternating with the plain call in one process
    python3 csrc/tune/encounters_grid_probe.py report TRACE_DIR HOST_LOG
                                                                  reads the kernel trace (csv) and the output of `host`, which
                                                                  names the calls, and prints the text of
                                                                  profiles/encounters_grid_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps, the horizons 0, 0.2 (the time step) and 2.0, the counts only and
with the list.  Grids: `matched` = encounters_grid(field, h, median radius, median |vx| + |vy|), and once the known bad case
`1 x 1`.  A batch of 256 x 1024 at the time step.  The field is the configuration's, widened to the bodies' bounding box where
a body has left it, so that nothing is outside: every result is checked equal to the plain call's in the same run before any
time is taken.  Per workload the host also counts, on the downloaded state, the cells of every row's window (median and
widest), the candidates the walk reads and those that pass the hot compare d2 <= H2 (a k-d tree with the row's own H)."""
import csv
import glob
import json
import os
import sys
import time

import pairs_probe as pp

ROOT = pp.ROOT
ROUNDS = 3                                                   # what `report` expects of `kernels`
HORIZONS = (0.0, 0.2, 2.0)
MAIN = ("encounters_grid_walk", "encounters_walk")           # a call ends with one of these


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(a[1][f] == b[1][f] for f in ("n_bodies", "pairs", "now", "end", "missed", "horizon"))


def window_stats(np, eg, state, grid, h):
    """-> (median cells, widest window in cells, candidates per row, the share of them that pass d2 <= H2)."""
    from scipy.spatial import cKDTree
    P, V, R = state
    rho, H, H2 = eg.reach(P, V, R, h, np.float32)
    c0, c1, r0, r1, ix, iy, cell = eg._windows(P, grid, H)
    nx, ny = int(grid["nx"]), int(grid["ny"])
    cells = np.maximum(c1 - c0 + 1, 0) * np.maximum(r1 - r0 + 1, 0)
    count = np.bincount(cell[cell >= 0], minlength=nx * ny).reshape(ny, nx)
    S = np.zeros((ny + 1, nx + 1), dtype=np.int64)           # members of the cells below and left of a corner
    S[1:, 1:] = count.cumsum(axis=0).cumsum(axis=1)
    some = cells > 0
    cand = np.where(some, S[r1 + 1, c1 + 1] - S[r0, c1 + 1] - S[r1 + 1, c0] + S[r0, c0], 0)
    finite = np.isfinite(H)
    passing = int((~finite).sum()) * (len(R) - 1)
    if finite.any():
        tree = cKDTree(P)
        passing += int(tree.query_ball_point(P[finite], H[finite], return_length=True).sum()) - int(finite.sum())
    return float(np.median(cells)), int(cells.max()), float(cand.mean()), passing / max(float(cand.sum()), 1.0)


def workloads():
    """-> (np, [(label, plain call, grid call)], the handles to close)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import encounter_cases as ec
    import encounters_grid_cases as eg
    cfg = nb.stock_config(particleCount=pp.N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(pp.STEPS)
    state = ec.widen(st.download())
    P, V, R = state
    n = len(R)
    field = (max(float(cfg.fieldWidth), float(np.abs(P[:, 0]).max()) * 1.001), max(float(cfg.fieldHeight), float(np.abs(P[:, 1]).max()) * 1.001))
    one_cell = nb.make_grid(1, 1, (-field[0], field[0], -field[1], field[1]))
    r_typ, v_typ = float(np.median(np.abs(R))), float(np.median(np.abs(V[:, 0]) + np.abs(V[:, 1])))
    print("# N=%d after %d steps: n %d, field %r, median radius %.4g, median |vx| + |vy| %.4g, max %.4g"
          % (pp.N_ONE, pp.STEPS, n, field, r_typ, v_typ, float((np.abs(V[:, 0]) + np.abs(V[:, 1])).max())), flush=True)
    calls = []

    def counts_only(handle, fn, systems, dtype, h, grid=None):
        info = np.zeros(systems, dtype=dtype)
        args = (handle,) + (() if grid is None else (grid.ctypes.data,)) + (float(h), None, 0, info.ctypes.data)
        assert fn(*args) == 0
        return info

    def add(handle, name, h, grid, kind, many, listed, stats_of=None):
        plain_fn = nb.lib.nbody_batch_get_encounters if many else nb.lib.nbody_get_encounters
        grid_fn = nb.lib.nbody_batch_get_encounters_grid if many else nb.lib.nbody_get_encounters_grid
        hd = handle._b if many else handle._ctx
        S = handle.systems if many else 1
        want, got = handle.encounters(h), handle.encounters(h, grid=grid)
        for w, g in zip(want, got) if many else ((want, got),):
            assert g[1]["outside"] == 0 and same(g, w), name
        every = got if many else (got,)
        cap = max(max(g[1]["pairs"] for g in every), 1)
        tot = {f: sum(g[1][f] for g in every) for f in ("pairs", "now", "end", "missed")}
        text = ""
        if stats_of is not None:
            med, widest, cand, share = window_stats(np, eg, stats_of, grid[0], h)
            text = "; windows: median %g cells, widest %d; %.1f candidates per row, %.4f of them pass d2 <= H2" % (med, widest, cand, share)
        print("# %s, h %g, grid %s %d x %d: pairs %d, now %d, end %d, missed %d (cap %d); the list and the counts equal to the plain "
              "call's%s" % (name, h, kind, grid["nx"][0], grid["ny"][0], tot["pairs"], tot["now"], tot["end"], tot["missed"], cap, text),
              flush=True)
        if listed:
            calls.append(("%s, the list | %s" % (name, kind), lambda: handle.encounters(h, cap=cap), lambda: handle.encounters(h, cap=cap, grid=grid)))
        calls.append(("%s, counts only | %s" % (name, kind), lambda: counts_only(hd, plain_fn, S, nb.ENCOUNTER_INFO_DTYPE, h),
                      lambda: counts_only(hd, grid_fn, S, nb.ENCOUNTER_GRID_INFO_DTYPE, h, grid)))

    for h in HORIZONS:
        add(st, "encounters h %g" % h, h, nb.encounters_grid(field, h, r_typ, v_typ), "matched", False, True, state)
    add(st, "encounters h %g" % HORIZONS[1], HORIZONS[1], one_cell, "1 x 1", False, False, state)

    bcfg = nb.stock_config(particleCount=pp.BATCH_N)
    batch = nb.StepperBatch(pp.BATCH_S, pp.BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(pp.BATCH_S)])
    batch.step(pp.STEPS)
    states = [ec.widen(batch.download(s)) for s in range(pp.BATCH_S)]
    reach = max(float(np.abs(s[0]).max()) for s in states) * 1.001
    bfield = (max(float(bcfg.fieldWidth), reach), max(float(bcfg.fieldHeight), reach))
    br = float(np.median(np.abs(np.concatenate([s[2] for s in states]))))
    bv = float(np.median(np.concatenate([np.abs(s[1][:, 0]) + np.abs(s[1][:, 1]) for s in states])))
    bgrid = nb.encounters_grid(bfield, HORIZONS[1], br, bv, most=int(np.sqrt((1 << 22) // pp.BATCH_S)))
    add(batch, "batch %d x %d encounters h %g" % (pp.BATCH_S, pp.BATCH_N, HORIZONS[1]), HORIZONS[1], bgrid, "matched", True, True, states[0])
    return np, calls, (st, batch)


def run_kernels(rounds):
    np, calls, handles = workloads()
    plan = []
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        for label, plain, onlist in calls:
            plain()
            onlist()
            plan += [label + " | plain", label + " | grid"]
    print("PLAN " + json.dumps(plan[:2 * len(calls)]), flush=True)
    for h in handles:
        h.close()


def run_host(rounds):
    np, calls, handles = workloads()
    for label, plain, onlist in calls:
        plain()
        onlist()                                            # the warm-up
        ms = {"plain": [], "grid": []}
        for _ in range(rounds):                             # alternating, in one process
            for kind, call in (("plain", plain), ("grid", onlist)):
                t0 = time.perf_counter()
                call()
                ms[kind].append((time.perf_counter() - t0) * 1e3)
        for kind in ("plain", "grid"):
            v = ms[kind]
            print(json.dumps({"call": "%s | %s" % (label, kind), "rounds": rounds, "ms": [round(x, 3) for x in v],
                              "ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)}), flush=True)
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
def report(trace_dir, host_log):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    rows = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
                  for r in csv.DictReader(open(files[0])))
    # a call ends with its walk; the cell list's stages and cells_gather before it belong to it
    done, list_ms = [], 0.0
    for _, name, ms in rows:
        main = next((k for k in MAIN if k in name), None)
        if main:
            done.append({"kernel": main, "walk": ms, "list": list_ms})
            list_ms = 0.0
        elif "cells_" in name:
            list_ms += ms
    host = [line for line in open(host_log)]
    labels = [json.loads(line)["call"] for line in host if line.startswith("{")]
    assert labels, "the host log names the calls of one round"
    per_round = len(labels)
    assert len(done) >= per_round * (ROUNDS + 1), (len(done), per_round)
    done = done[-per_round * ROUNDS:]                        # without the checks and the warm-up round
    med = lambda v: sorted(v)[len(v) // 2]                   # noqa: E731
    print("# csrc/tune/encounters_grid_probe.py on one MI355X: encounters_grid_walk next to encounters_walk, fp32, the stock state "
          "after %d steps" % pp.STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python encounters_grid_probe.py kernels 3 (a run of its own); ms, median of "
          "the rounds (spread); list + gather: the cell list's stages and cells_gather of the call; kernels = walk + list + gather")
    kernels = {}
    for k, label in enumerate(labels):
        mine = done[k::per_round]
        assert all(("grid" in c["kernel"]) == label.endswith("| grid") for c in mine), (label, [c["kernel"] for c in mine])
        walk, lst = [c["walk"] for c in mine], [c["list"] for c in mine]
        kernels[label] = med([w + l for w, l in zip(walk, lst)])
        print("%-62s %-20s walk %8.3f ms (%.3f)  list + gather %6.3f ms  kernels %8.3f ms"
              % (label, mine[0]["kernel"], med(walk), max(walk) - min(walk), med(lst), kernels[label]))
    print("# whole calls under the host clock (encounters_grid_probe.py host 3: a warm-up, then 3 rounds, plain and grid alternating):")
    whole = {}
    for line in host:
        if line.startswith("#"):
            print(line.rstrip())
        elif line.startswith("{"):
            r = json.loads(line)
            whole[r["call"]] = r
            print("%-62s rounds %s ms  median %8.3f  spread %.3f" % (r["call"], r["ms"], r["ms_median"], r["ms_max"] - r["ms_min"]))
    print("# the grid form against the plain call: kernels (plain / grid), whole calls (plain / grid), and whether the whole call wins "
          "by more than the spread of the rounds (no overlap between the two sets of rounds)")
    for label in labels:
        if not label.endswith("| grid"):
            continue
        plain = label[:-len("grid")] + "plain"
        g, p = whole[label], whole[plain]
        print("%-62s kernels %8.3f / %8.3f ms = %7.1f x   whole %8.3f / %8.3f ms = %6.2f x   %s"
              % (label[:-len(" | grid")], kernels[plain], kernels[label], kernels[plain] / kernels[label], p["ms_median"], g["ms_median"],
                 p["ms_median"] / g["ms_median"], "wins" if g["ms_max"] < p["ms_min"] else "loses" if g["ms_min"] > p["ms_max"] else "within the spread"))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    if mode == "kernels":
        run_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else ROUNDS)
    elif mode == "host":
        run_host(int(sys.argv[2]) if len(sys.argv) > 2 else ROUNDS)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
