#!/usr/bin/env python3
"""Cost of the pair counts and the bound pairs on the cell list (nbody_get_pair_counts_grid, nbody_get_binaries_grid and their
batch forms) next to the tile walks of nbody_get_pair_counts and nbody_get_binaries
(DESIGN.md 4.15), both timed in the same run on the state and the values of pairs_probe.py and binary_probe.py.

    python3 csrc/tune/pairs_grid_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                             (a run of its own; nothing else is traced with it)
    python3 csrc/tune/pairs_grid_probe.py host [rounds]      whole calls under the host clock around the synchronising call:
                                                             a warm-up, then `rounds` rounds, the grid form alternating
                                                             with the plain call in one process
    python3 csrc/tune/pairs_grid_probe.py report TRACE_DIR HOST_LOG
                                                             reads the kernel trace (csv) and the output of `host`, which
                                                             names the calls, and prints the text of
                                                             profiles/pairs_grid_probe.txt

Shapes: N = 262144 fp32, the stock state after STEPS steps.  Pair counts with 32 logarithmic bins up to the two lengths of
pairs_probe.py (a body has 1.5 and 7 others within reach on average); binaries at sep = 128 and sep = 1024 (binary_probe.py's
sep / 8 and sep), the counts only and with the list.  Grids: `matched` = within_grid(field, top edge or sep), and once each
the known bad case `1 x 1`.  A batch of 256 x 1024 with the sparse edges and that top as the separation.  The field is the
configuration's, widened to the bodies' bounding box where a body has left it, so that nothing is outside: every result is
checked equal to the plain call's in the same run before any time is taken."""
import collections
import csv
import glob
import json
import os
import sys
import time

import pairs_probe as pp

ROOT = pp.ROOT
ROUNDS = 3                                                   # what `report` expects of `kernels`
SEPS = (128.0, 1024.0)
MAIN = ("pair_counts_grid", "binaries_grid_walk", "pair_counts", "binaries_walk")      # a call ends with one of these


def same_pairs(a, b):
    return a["counts"].tobytes() == b["counts"].tobytes() and (a["below"], a["rest"], a["pairs"]) == (b["below"], b["rest"], b["pairs"])


def same_binaries(a, b, counts):
    return a[0].tobytes() == b[0].tobytes() and all(a[1][f] == b[1][f] for f in counts)


def workloads():
    """-> (np, [(label, plain call, grid call, summary of a result)], the handles to close)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import binary_cases as bc
    cfg = nb.stock_config(particleCount=pp.N_ONE)
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    st.step(pp.STEPS)
    P = bc.widen(st.download())[0]
    n = len(P)
    field = (max(float(cfg.fieldWidth), float(np.abs(P[:, 0]).max()) * 1.001), max(float(cfg.fieldHeight), float(np.abs(P[:, 1]).max()) * 1.001))
    one_cell = nb.make_grid(1, 1, (-field[0], field[0], -field[1], field[1]))
    print("# N=%d after %d steps: n %d, field %r" % (pp.N_ONE, pp.STEPS, n, field), flush=True)
    calls = []

    def counts_only(handle, fn, systems, dtype, sep2, grid=None):
        info = np.zeros(systems, dtype=dtype)
        args = (handle,) + (() if grid is None else (grid.ctypes.data,)) + (float(sep2), None, 0, info.ctypes.data)
        assert fn(*args) == 0
        return info

    def add_pairs(handle, name, e2, grid, kind, many):
        plain = lambda: handle.pair_counts(e2, squared=True)                      # noqa: E731
        onlist = lambda: handle.pair_counts(e2, squared=True, grid=grid)          # noqa: E731
        want, got = plain(), onlist()
        for w, g in zip(want, got) if many else ((want, got),):
            assert g["outside"] == 0 and same_pairs(g, w), name
        g0 = got[0] if many else got
        print("# %s, top edge %.6g, grid %s %d x %d: in range %.3e of %d pairs; counts equal to the plain call's"
              % (name, np.sqrt(e2[-1]), kind, grid["nx"][0], grid["ny"][0], pp.in_range(g0), g0["pairs"]), flush=True)
        calls.append(("%s | %s" % (name, kind), plain, onlist))

    def add_binaries(handle, name, sep, grid, kind, many, listed):
        plain_fn = nb.lib.nbody_batch_get_binaries if many else nb.lib.nbody_get_binaries
        grid_fn = nb.lib.nbody_batch_get_binaries_grid if many else nb.lib.nbody_get_binaries_grid
        h = handle._b if many else handle._ctx
        S = handle.systems if many else 1
        want, got = handle.binaries(sep), handle.binaries(sep, grid=grid)
        for w, g in zip(want, got) if many else ((want, got),):
            assert g[1]["outside"] == 0 and same_binaries(g, w, bc.COUNTS), name
        cap = max(max(g[1]["pairs"] for g in (got if many else (got,))), 1)
        g0 = got[0] if many else got
        print("# %s, sep %g, grid %s %d x %d: near %d, bound %d (cap %d); the list and the counts equal to the plain call's"
              % (name, sep, kind, grid["nx"][0], grid["ny"][0], g0[1]["near"], g0[1]["pairs"], cap), flush=True)
        if listed:
            calls.append(("%s, the list | %s" % (name, kind), lambda: handle.binaries(sep, cap=cap), lambda: handle.binaries(sep, cap=cap, grid=grid)))
        calls.append(("%s, counts only | %s" % (name, kind), lambda: counts_only(h, plain_fn, S, nb.BINARY_INFO_DTYPE, sep * sep),
                      lambda: counts_only(h, grid_fn, S, nb.BINARY_GRID_INFO_DTYPE, sep * sep, grid)))

    small, percolating = pp.centre_link(np, pp.MEAN_SMALL, P), pp.centre_link(np, pp.MEAN_PERCOLATING, P)
    ea, eb, _ = pp.edge_sets(np, small, percolating)
    add_pairs(st, "pair counts (a) sparse", ea, nb.within_grid(field, small), "matched", False)
    add_pairs(st, "pair counts (b) percolating", eb, nb.within_grid(field, percolating), "matched", False)
    for sep in SEPS:
        add_binaries(st, "binaries sep %g" % sep, sep, nb.within_grid(field, sep), "matched", False, True)
    add_pairs(st, "pair counts (a) sparse", ea, one_cell, "1 x 1", False)
    add_binaries(st, "binaries sep %g" % SEPS[0], SEPS[0], one_cell, "1 x 1", False, False)

    bcfg = nb.stock_config(particleCount=pp.BATCH_N)
    batch = nb.StepperBatch(pp.BATCH_S, pp.BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(pp.BATCH_S)])
    batch.step(pp.STEPS)
    reach = max(float(np.abs(bc.widen(batch.download(s))[0]).max()) for s in range(pp.BATCH_S)) * 1.001
    bfield = (max(float(bcfg.fieldWidth), reach), max(float(bcfg.fieldHeight), reach))
    P0 = bc.widen(batch.download(0))[0]
    bsmall = pp.centre_link(np, pp.MEAN_SMALL, P0)
    ba, _, _ = pp.edge_sets(np, bsmall, pp.centre_link(np, pp.MEAN_PERCOLATING, P0))
    bgrid = nb.within_grid(bfield, bsmall, most=int(np.sqrt((1 << 22) // pp.BATCH_S)))
    add_pairs(batch, "batch %d x %d pair counts (a) sparse" % (pp.BATCH_S, pp.BATCH_N), ba, bgrid, "matched", True)
    add_binaries(batch, "batch %d x %d binaries" % (pp.BATCH_S, pp.BATCH_N), bsmall, bgrid, "matched", True, True)
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
    med = lambda v: sorted(v)[len(v) // 2]
    print("# csrc/tune/pairs_grid_probe.py on one MI355X: pair_counts_grid and binaries_grid_walk next to pair_counts and binaries_walk, "
          "fp32, the stock state after %d steps" % pp.STEPS)
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python pairs_grid_probe.py kernels 3 (a run of its own); ms, median of the "
          "rounds (spread); list + gather: the cell list's stages and cells_gather of the call; kernels = walk + list + gather")
    kernels = {}
    for k, label in enumerate(labels):
        mine = done[k::per_round]
        assert all(("grid" in c["kernel"]) == label.endswith("| grid") for c in mine), (label, [c["kernel"] for c in mine])
        walk, lst = [c["walk"] for c in mine], [c["list"] for c in mine]
        kernels[label] = med([w + l for w, l in zip(walk, lst)])
        print("%-62s %-18s walk %8.3f ms (%.3f)  list + gather %6.3f ms  kernels %8.3f ms"
              % (label, mine[0]["kernel"], med(walk), max(walk) - min(walk), med(lst), kernels[label]))
    print("# whole calls under the host clock (pairs_grid_probe.py host 3: a warm-up, then 3 rounds, plain and grid alternating):")
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
