#!/usr/bin/env python3
"""Diagnostics of every system of a batch: one StepperBatch.diagnostics() against the route there was before it.

    python3 csrc/tune/batch_diag_probe.py --baseline-root DIR [--shapes 1024x256,256x1024,64x4096,16x16384] [--rounds 3]
    python3 csrc/tune/batch_diag_probe.py --trace 256x1024     (a short candidate run with a recorded series, target of
                                                                 rocprofv3 --kernel-trace --stats)

DIR is a checkout of the commit BEFORE the batch diagnostics, built (make -C ppa-nbody-collisions_amd/csrc): the baseline
runs that library, in a child process of its own that loads it by path - two builds of one library do not share a
process.  The child stays alive and the two sides take turns, round by round, in the same GPU call.

Shapes are S x N: S systems of N bodies, the stock configuration (stock radii), fp32, literal semantics, seeds 1..S,
random velocities, three ensemble steps after the upload.  Both sides hold the same batch state.
    baseline   what DESIGN.md 9 recommended: for every system download(s), upload into ONE reused Stepper, diagnostics()
    candidate  one StepperBatch.diagnostics()
One call per round, host clock around work that ends in a synchronise.  Before any time is reported the results must be
bit-equal (sha256 over every field of every system but `step`: a freshly uploaded Stepper counts its steps from 0).
Medians over the rounds, the spread (max - min) of the baseline's own rounds, and the ratio.
"""
import argparse
import hashlib
import json
import os
import select
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
REPLY_TIMEOUT_S = 240           # a side that does not answer within this is killed and the probe fails
STEPS_BEFORE = 3


def load_package(root):
    sys.path.insert(0, root)
    try:
        import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    except ImportError:
        pass
    import ppa_nbody_collisions_amd as nb
    return nb


def make_batch(nb, S, N):
    import numpy as np
    cfg = nb.stock_config(particleCount=N)
    bodies = []
    for s in range(S):
        b = nb.init_bodies(cfg, seed=1 + s)
        b.Velocities[:] = np.random.default_rng(1 + s).uniform(-3, 3, size=(N, 2)).astype(np.float32)
        bodies.append(b)
    batch = nb.StepperBatch(S, N, cfg=cfg)
    batch.upload(bodies)
    batch.step(STEPS_BEFORE)
    batch.sync()
    return cfg, bodies, batch


def digest(diags):
    import numpy as np
    h = hashlib.sha256()
    for d in diags:
        h.update(b"%d:%d:" % (d["n_bodies"], d["coincident_pairs"]))
        vals = [d["mass"], *d["momentum"], *d["center_of_mass"], d["angular_momentum"], d["kinetic"], d["potential"]]
        h.update(np.array(vals, dtype=np.float64).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------
# baseline side: a child process on the older library
# ---------------------------------------------------------------------------------------------------------
def baseline_call(batch, st):
    t0 = time.perf_counter()
    out = []
    for s in range(batch.systems):
        st.upload(batch.download(s))
        out.append(st.diagnostics())
    return time.perf_counter() - t0, out


def baseline_child(root):
    nb = load_package(root)
    assert not hasattr(nb.StepperBatch, "diagnostics"), "the baseline root already has the batch diagnostics"
    batch = st = None
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "setup":
            if batch is not None:
                batch.close()
                st.close()
            cfg, _, batch = make_batch(nb, cmd["S"], cmd["N"])
            st = nb.Stepper(cfg)
            baseline_call(batch, st)                                       # warm: code objects, lazy buffers
            reply = {"kernel": batch.kernel_name()}
        elif cmd["op"] == "call":
            seconds, out = baseline_call(batch, st)
            reply = {"seconds": seconds, "digest": digest(out)}
        else:
            break
        sys.stdout.write(json.dumps(reply) + "\n")
        sys.stdout.flush()
    if batch is not None:
        batch.close()
        st.close()


class Baseline:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        ready, _, _ = select.select([self.p.stdout], [], [], REPLY_TIMEOUT_S)
        line = self.p.stdout.readline() if ready else ""
        if not line:
            self.p.kill()
            raise SystemExit("baseline child did not answer %r (exit status %r): nothing more is started" % (cmd, self.p.poll()))
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


# ---------------------------------------------------------------------------------------------------------
# candidate side
# ---------------------------------------------------------------------------------------------------------
def candidate_call(batch, potential=False):
    t0 = time.perf_counter()
    out = batch.diagnostics(potential=potential)
    return time.perf_counter() - t0, out


def probe_shape(nb, base, S, N, rounds):
    _, _, batch = make_batch(nb, S, N)
    out = {"S": S, "N": N, "radii": "stock", "steps_before": STEPS_BEFORE, "kernel": batch.kernel_name()}
    base.ask(op="setup", S=S, N=N)
    candidate_call(batch)                                                  # warm
    t_base, t_cand, t_phi = [], [], []
    for r in range(rounds):                                                # the two sides take turns
        rb = base.ask(op="call")
        tc, got = candidate_call(batch)
        if digest(got) != rb["digest"]:
            raise SystemExit("%dx%d round %d: the diagnostics differ - no time is reported" % (S, N, r))
        t_base.append(rb["seconds"])
        t_cand.append(tc)
        t_phi.append(candidate_call(batch, potential=True)[0])
    batch.close()
    ms = lambda xs: [round(x * 1e3, 4) for x in xs]                                # noqa: E731
    pairs = sum(d["n_bodies"] * (d["n_bodies"] - 1) for d in got)
    out["results_bit_equal"] = True
    out["baseline_ms_per_call"] = ms(t_base)
    out["candidate_ms_per_call"] = ms(t_cand)
    out["candidate_with_phi_ms_per_call"] = ms(t_phi)
    out["baseline_median_ms"] = round(statistics.median(t_base) * 1e3, 4)
    out["baseline_fastest_ms"] = round(min(t_base) * 1e3, 4)
    out["baseline_spread_ms"] = round((max(t_base) - min(t_base)) * 1e3, 4)
    out["candidate_median_ms"] = round(statistics.median(t_cand) * 1e3, 4)
    out["candidate_with_phi_median_ms"] = round(statistics.median(t_phi) * 1e3, 4)
    out["ratio_baseline_over_candidate"] = round(out["baseline_median_ms"] / out["candidate_median_ms"], 2)
    out["candidate_median_below_baseline_fastest"] = out["candidate_median_ms"] < out["baseline_fastest_ms"]
    out["ordered_pairs_per_call"] = pairs
    out["pairs_per_s_end_to_end"] = float("%.4g" % (pairs / statistics.median(t_cand)))
    return out


def trace_run(nb, S, N, records=20):
    """What the profiler looks at: `records` ensemble steps with a record after each, enqueued in one go, then a few
    synchronising calls.  The ordered pairs of every record come from the series itself (n_bodies per system)."""
    _, _, batch = make_batch(nb, S, N)
    batch.reserve_diagnostics(records)
    batch.sync()
    t0 = time.perf_counter()
    batch.step(records, record_every=1)
    t_enqueue = time.perf_counter() - t0
    batch.sync()
    t_all = time.perf_counter() - t0
    log = batch.diagnostics_log()
    n = log["n_bodies"].astype("int64")
    for _ in range(3):
        batch.diagnostics()
    got = batch.diagnostics(potential=True)
    rec = {"trace": "%dx%d" % (S, N), "kernel": batch.kernel_name(), "steps": records, "records": int(log.shape[0]),
           "enqueue_ms": round(t_enqueue * 1e3, 3), "enqueue_and_run_ms": round(t_all * 1e3, 3),
           "ordered_pairs_all_records": int((n * (n - 1)).sum()),
           "ordered_pairs_per_record_first_last": [int((n[0] * (n[0] - 1)).sum()), int((n[-1] * (n[-1] - 1)).sum())],
           "synchronising_calls_after": {"without_phi": 3, "with_phi": 1,
                                         "ordered_pairs_each": sum(d["n_bodies"] * (d["n_bodies"] - 1) for d in got)}}
    batch.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--baseline-root")
    ap.add_argument("--shapes", default="1024x256,256x1024,64x4096,16x16384")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace")
    ap.add_argument("--out", help="append the result lines to this file as well")
    a = ap.parse_args()
    if a.child:
        return baseline_child(a.child)
    nb = load_package(ROOT)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    if a.trace:
        S, N = (int(x) for x in a.trace.split("x"))
        emit(trace_run(nb, S, N))
    else:
        if not a.baseline_root:
            ap.error("--baseline-root DIR (a built checkout of the commit before the batch diagnostics)")
        if a.rounds < 3:
            ap.error("at least 3 rounds")
        base = Baseline(os.path.abspath(a.baseline_root))
        try:
            for shape in a.shapes.split(","):
                S, N = (int(x) for x in shape.split("x"))
                emit(probe_shape(nb, base, S, N, a.rounds))
        finally:
            base.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
