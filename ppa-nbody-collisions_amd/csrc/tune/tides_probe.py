#!/usr/bin/env python3
"""Cost of the tidal tensor and the jerk (nbody_get_tides, nbody_batch_get_tides) against its yardsticks,
diag_potential<float> and field_at<float> at the same N in the same run: the same ascending walk over j with more
instructions per pair.

    python3 csrc/tune/tides_probe.py kernels [rounds]   the launches alone: target of `rocprofv3 --kernel-trace --stats`
                                                        (a run of its own; nothing else is traced with it)
    python3 csrc/tune/tides_probe.py host [reps]        whole Stepper.tides() / StepperBatch.tides() calls, host clock
    python3 csrc/tune/tides_probe.py report TRACE_DIR [HOST_LOG] [BENCH_JSON]
                                                        reads the kernel trace (csv), counts the fp64 VALU instructions per
                                                        pair of the inner loops in build/csrc/nbody_ctx.s (make asm), weights
                                                        them with profiles/r03_issue_probe_f64.txt, and prints the text of
                                                        profiles/tides_probe.txt

Shapes: N = 262144 fp32 own rows with and without the jerk; the same state with 65536 explicit points (the tensor alone,
and moving points with the jerk); a batch of 256 x 1024 with and without the jerk."""
import collections
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from field_probe import BATCH_N, BATCH_S, M_POINTS, N_ONE, hot_loop, issue_costs, workloads  # noqa: E402


def point_velocities(np):
    return np.random.default_rng(3).uniform(-4, 4, size=(M_POINTS, 2))


def run_kernels(rounds):
    np, st, pts, batch = workloads()
    pv = point_velocities(np)
    for _ in range(rounds + 1):                             # the first round warms up (code objects, lazy buffers)
        st.diagnostics(potential=True)
        st.field()
        st.field(pts)
        st.tides()
        st.tides(jerk=True)
        st.tides(pts)
        st.tides(pts, pv, jerk=True)
        batch.diagnostics(potential=True)
        batch.field()
        batch.tides()
        batch.tides(jerk=True)
    st.close()
    batch.close()


def run_host(reps):
    np, st, pts, batch = workloads()
    pv = point_velocities(np)
    calls = (("Stepper.tides() N=%d" % N_ONE, st.tides),
             ("Stepper.tides(jerk=True) N=%d" % N_ONE, lambda: st.tides(jerk=True)),
             ("Stepper.tides(%d points) N=%d" % (M_POINTS, N_ONE), lambda: st.tides(pts)),
             ("Stepper.tides(%d points, point_vel, jerk=True) N=%d" % (M_POINTS, N_ONE), lambda: st.tides(pts, pv, jerk=True)),
             ("Stepper.field() N=%d" % N_ONE, st.field),
             ("Stepper.diagnostics(potential=True) N=%d" % N_ONE, lambda: st.diagnostics(potential=True)),
             ("StepperBatch.tides() %d x %d" % (BATCH_S, BATCH_N), batch.tides),
             ("StepperBatch.tides(jerk=True) %d x %d" % (BATCH_S, BATCH_N), lambda: batch.tides(jerk=True)),
             ("StepperBatch.field() %d x %d" % (BATCH_S, BATCH_N), batch.field))
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
FP64 = ("v_fma_f64", "v_mul_f64", "v_add_f64", "v_rsq_f64")


def report(trace_dir, host_log, bench_json):
    import csv
    import glob
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
    loops = collections.OrderedDict((
        ("diag_potential<float>", hot_loop(asm, "diag_potentialIfEE")),
        ("field_at<float, own>", hot_loop(asm, "field_atIfLb1E")),
        ("tides_at<float, own>", hot_loop(asm, "tides_atIfLb1ELb0E")),
        ("tides_at<float, own, jerk>", hot_loop(asm, "tides_atIfLb1ELb1E")),
        ("tides_at<float, points>", hot_loop(asm, "tides_atIfLb0ELb0E")),
        ("tides_at<float, points, jerk>", hot_loop(asm, "tides_atIfLb0ELb1E"))))
    ns = {}
    print("# csrc/tune/tides_probe.py on one MI355X: tides_at against diag_potential and field_at, the same ascending walk with")
    print("# more instructions per pair.  Inner loops (build/csrc/nbody_ctx.s, the unchecked 4-pair block), instructions per pair,")
    print("# and their saturated issue cost by profiles/r03_issue_probe_f64.txt (ns per wave-instruction per SIMD):")
    for name, (per, pairs) in loops.items():
        ns[name] = sum(per.get(k, 0) * cost[k] for k in FP64)
        print("#   %-30s %s  -> %.2f ns per wave-pair" % (name, "  ".join("%s %.2f" % (k, per[k]) for k in sorted(per)), ns[name]))
    pot, fld = ns["diag_potential<float>"], ns["field_at<float, own>"]
    for name in list(loops)[2:]:
        print("# expected ratio of time per pair, %-30s %.3f of the potential, %.3f of the field" % (name + ":", ns[name] / pot, ns[name] / fld))
    p_one, p_pts, p_batch = float(N_ONE) * N_ONE, float(M_POINTS) * N_ONE, float(BATCH_S) * BATCH_N * BATCH_N

    def k_tides(own, jerk, count):
        b = lambda v: "true" if v else "false"               # noqa: E731
        return (("tides_at<float, %s, %s" % (b(own), b(jerk)), count), ("tides_atIfLb%dELb%dE" % (own, jerk), count))

    def k_field(own, count):
        return (("field_at<float, %s" % ("true" if own else "false"), count), ("field_atIfLb%dE" % own, count))

    diag_one = (("nbk::diag_potential<float>",), ("3nbk14diag_potentialIfEE",))
    diag_batch = (("batch_diag_potential<true>",), ("batch_diag_potentialILb1E",))
    one, bat = "RowsOneCount", "RowsBatchCount"
    shapes = (("N=%d own rows" % N_ONE, k_tides(1, 0, one), k_field(1, one), diag_one, p_one, p_one, p_one, "tides_at<float, own>"),
              ("N=%d own rows, jerk" % N_ONE, k_tides(1, 1, one), k_field(1, one), diag_one, p_one, p_one, p_one, "tides_at<float, own, jerk>"),
              ("N=%d, %d points" % (N_ONE, M_POINTS), k_tides(0, 0, one), k_field(0, one), diag_one, p_pts, p_pts, p_one, "tides_at<float, points>"),
              ("N=%d, %d points, jerk" % (N_ONE, M_POINTS), k_tides(0, 1, one), k_field(0, one), diag_one, p_pts, p_pts, p_one,
               "tides_at<float, points, jerk>"),
              ("batch %d x %d own rows" % (BATCH_S, BATCH_N), k_tides(1, 0, bat), k_field(1, bat), diag_batch, p_batch, p_batch, p_batch,
               "tides_at<float, own>"),
              ("batch %d x %d own rows, jerk" % (BATCH_S, BATCH_N), k_tides(1, 1, bat), k_field(1, bat), diag_batch, p_batch, p_batch, p_batch,
               "tides_at<float, own, jerk>"))
    print("# kernel trace: rocprofv3 --kernel-trace --stats -- python tides_probe.py kernels 3 (a run of its own); ms, median of the rounds (spread)")
    for what, tsub, fsub, dsub, tp, fp, dp, loop in shapes:
        t, ts, k = ms_of(*tsub)
        f, fs, _ = ms_of(*fsub)
        d, ds, _ = ms_of(*dsub)
        rd, rf = (t / tp) / (d / dp), (t / tp) / (f / fp)
        sd, sf = rd * (ts / t + ds / d), rf * (ts / t + fs / f)
        wd, wf = ns[loop] / pot, ns[loop] / fld
        print("%-36s tides_at %8.3f (%.3f)  field_at %8.3f (%.3f)  potential %8.3f (%.3f)  %d rounds  ps per pair %.3f | %.3f | %.3f"
              % (what, t, ts, f, fs, d, ds, k, t / tp * 1e9, f / fp * 1e9, d / dp * 1e9))
        print("%-36s   against the potential: ratio %.3f (spread %.3f), expected %.3f: %s;  against the field: ratio %.3f (spread %.3f), "
              "expected %.3f: %s" % ("", rd, sd, wd, "within" if rd <= wd + sd else "ABOVE the expected ratio", rf, sf, wf,
                                     "within" if rf <= wf + sf else "ABOVE the expected ratio"))
    if host_log:
        print("# whole calls under the host clock (tides_probe.py host 5; median of 5 after a warm-up):")
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
