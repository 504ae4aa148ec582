#!/usr/bin/env python3
"""Cost of the field evaluation (nbody_get_field, nbody_batch_get_field) against its yardstick,
diag_potential<T> at the same N in the same run: the same walk over j with fewer instructions per pair.

    python3 csrc/tune/field_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                        (a run of its own; nothing else is traced with it)
    python3 csrc/tune/field_probe.py host [reps]        whole Stepper.field() / StepperBatch.field() calls, host clock
    python3 csrc/tune/field_probe.py report TRACE_DIR [HOST_LOG] [BENCH_JSON]
                                                        reads the kernel trace (csv), counts the fp64 VALU instructions per
                                                        pair of both inner loops in build/csrc/nbody_ctx.s (make asm), weights
                                                        them with profiles/r03_issue_probe_f64.txt, and prints the text of
                                                        profiles/field_probe.txt

Shapes: N = 262144 fp32 with points=None; the same state with 65536 explicit points; a batch of 256 x 1024."""
import collections
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
N_ONE, M_POINTS, BATCH_S, BATCH_N = 262144, 65536, 256, 1024


def workloads():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    cfg = nb.stock_config(particleCount=N_ONE)
    b = nb.init_bodies(cfg)
    b.Velocities[:] = np.random.default_rng(1).uniform(-3, 3, size=(N_ONE, 2)).astype(np.float32)
    st = nb.Stepper(cfg)
    st.upload(b)
    pts = np.random.default_rng(2).uniform(0, 1, size=(M_POINTS, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
    bcfg = nb.stock_config(particleCount=BATCH_N)
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    batch.upload([nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)])
    return np, st, pts, batch


def run_kernels(rounds):
    np, st, pts, batch = workloads()
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        st.diagnostics(potential=True)
        st.field()
        st.field(pts)
        batch.diagnostics(potential=True)
        batch.field()
    st.close()
    batch.close()


def run_host(reps):
    np, st, pts, batch = workloads()
    calls = (("Stepper.field() N=%d" % N_ONE, st.field), ("Stepper.field(%d points) N=%d" % (M_POINTS, N_ONE), lambda: st.field(pts)),
             ("Stepper.diagnostics(potential=True) N=%d" % N_ONE, lambda: st.diagnostics(potential=True)),
             ("StepperBatch.field() %d x %d" % (BATCH_S, BATCH_N), batch.field),
             ("StepperBatch.diagnostics(potential=True) %d x %d" % (BATCH_S, BATCH_N), lambda: batch.diagnostics(potential=True)))
    for name, call in calls:
        call()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"call": name, "reps": reps, "ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}),
              flush=True)
    st.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
def hot_loop(asm, sub):
    """Opcode histogram per pair of the kernel's hottest block (most v_rsq_f64: the unchecked 4-pair loop)."""
    lines = asm.split("\n")
    k0 = next(k for k, l in enumerate(lines) if re.match(r"_ZN\w*" + sub + r"\w*:", l))
    k1 = next(k for k in range(k0, len(lines)) if lines[k].startswith(".Lfunc_end"))
    blocks = re.split(r"\n(?=\.LBB)", "\n".join(lines[k0:k1]))
    best = max(blocks, key=lambda b: b.count("v_rsq_f64"))
    pairs = best.count("v_rsq_f64")
    ops = collections.Counter(l.split()[0] for l in best.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";")))
    cls = collections.Counter()
    for op, k in ops.items():
        if op.startswith("v_rsq_f64"):
            cls["v_rsq_f64"] += k
        elif op.startswith(("v_fma_f64", "v_fmac_f64")):
            cls["v_fma_f64"] += k
        elif op.startswith("v_mul_f64"):
            cls["v_mul_f64"] += k
        elif op.startswith("v_add_f64"):
            cls["v_add_f64"] += k
        elif op.startswith("v_"):
            cls["other VALU"] += k
        elif op.startswith("ds_"):
            cls["ds_read"] += k
    return {k: v / pairs for k, v in cls.items()}, pairs


def issue_costs():
    cost = {}
    for line in open(os.path.join(ROOT, "profiles", "r03_issue_probe_f64.txt")):
        m = re.match(r"(v_\w+)\s+([0-9.]+) ns per wave-instruction", line)
        if m:
            cost[m.group(1)] = float(m.group(2))
    return cost


def report(trace_dir, host_log, bench_json):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no *kernel_trace.csv under %s" % trace_dir
    dur = collections.defaultdict(list)
    for row in csv.DictReader(open(files[0])):
        dur[row["Kernel_Name"]].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))

    def ms_of(*alternatives):                                # the name as the trace has it: demangled, or mangled
        names = [k for k in dur if any(all(s in k for s in subs) for subs in alternatives)]
        assert len(names) == 1, (alternatives, names)
        d = [t for _, t in sorted(dur[names[0]])][1:]        # without the warm-up round
        d.sort()
        return d[len(d) // 2], d[-1] - d[0], len(d)

    asm = open(os.path.join(ROOT, "build", "csrc", "nbody_ctx.s")).read()
    cost = issue_costs()
    loops = {"diag_potential<float>": hot_loop(asm, "diag_potentialIfEE"), "field_at<float, own>": hot_loop(asm, "field_atIfLb1E"),
             "field_at<float, points>": hot_loop(asm, "field_atIfLb0E")}
    ns = {}
    print("# csrc/tune/field_probe.py on one MI355X: field_at against diag_potential, the same walk with fewer instructions per pair")
    print("# inner loops (build/csrc/nbody_ctx.s, the unchecked 4-pair block), instructions per pair, and their saturated issue cost")
    print("# by profiles/r03_issue_probe_f64.txt (ns per wave-instruction per SIMD):")
    for name, (per, pairs) in loops.items():
        ns[name] = sum(per.get(k, 0) * cost[k] for k in ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_rsq_f64"))
        print("#   %-24s %s  -> %.2f ns per wave-pair" % (name, "  ".join("%s %.2f" % (k, per[k]) for k in sorted(per)), ns[name]))
    print("# expected ratio of time per pair: own %.3f, points %.3f"
          % (ns["field_at<float, own>"] / ns["diag_potential<float>"], ns["field_at<float, points>"] / ns["diag_potential<float>"]))
    pairs_one, pairs_pts, pairs_batch = float(N_ONE) * N_ONE, float(M_POINTS) * N_ONE, float(BATCH_S) * BATCH_N * BATCH_N
    one_own = (("field_at<float, true", "RowsOneCount"), ("field_atIfLb1E", "RowsOneCount"))
    one_pts = (("field_at<float, false", "RowsOneCount"), ("field_atIfLb0E", "RowsOneCount"))
    batch_own = (("field_at<float, true", "RowsBatchCount"), ("field_atIfLb1E", "RowsBatchCount"))
    diag_one = (("nbk::diag_potential<float>",), ("3nbk14diag_potentialIfEE",))
    diag_batch = (("batch_diag_potential<true>",), ("batch_diag_potentialILb1E",))
    shapes = (("N=%d points=None" % N_ONE, one_own, diag_one, pairs_one, pairs_one, "own"),
              ("N=%d, %d points" % (N_ONE, M_POINTS), one_pts, diag_one, pairs_pts, pairs_one, "points"),
              ("batch %d x %d points=None" % (BATCH_S, BATCH_N), batch_own, diag_batch, pairs_batch, pairs_batch, "own"))
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python field_probe.py kernels 3 (a run of its own); ms, median of the rounds (spread)")
    for what, fsub, dsub, fpairs, dpairs, kind in shapes:
        f, fs, k = ms_of(*fsub)
        d, ds, _ = ms_of(*dsub)
        ratio = (f / fpairs) / (d / dpairs)
        spread = ratio * (fs / f + ds / d)
        want = ns["field_at<float, %s>" % kind] / ns["diag_potential<float>"]
        print("%-34s field_at %8.3f (%.3f)  potential %8.3f (%.3f)  %d rounds  ps per pair %.3f against %.3f  ratio %.3f "
              "(spread %.3f), expected %.3f: %s"
              % (what, f, fs, d, ds, k, f / fpairs * 1e9, d / dpairs * 1e9, ratio, spread, want,
                 "within" if ratio <= want + spread else "ABOVE the expected ratio"))
    if host_log:
        print("# whole calls under the host clock (field_probe.py host 5; median of 5 after a warm-up):")
        for line in open(host_log):
            if line.startswith("{"):
                print(line.rstrip())
    if bench_json:
        for line in open(bench_json):
            if line.startswith("{"):
                r = json.loads(line)
                print("# same visit, bench.py --gpus 1 --steps 20 --warmup 3: %s" % json.dumps(
                    {k: r[k] for k in r if k in ("ms_per_step", "pairs_per_s", "n", "N", "kernel")}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    if mode == "kernels":
        run_kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    elif mode == "host":
        run_host(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None, sys.argv[4] if len(sys.argv) > 4 else None)
    else:
        sys.exit(__doc__)
