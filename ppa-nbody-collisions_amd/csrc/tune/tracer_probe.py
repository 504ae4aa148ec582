#!/usr/bin/env python3
"""Cost of the tracer particles (nbody_tracers_*, nbody_batch_tracers_*): ms per step over plain stepping,
against the route they replace - a host loop per step of field(points), a numpy update and step(1).

    python3 csrc/tune/tracer_probe.py [OUT]        writes OUT (default profiles/tracer_probe.txt)

Shapes: N = 262144 fp32 with M = 65536 and M = 1048576 tracers; a batch of 256 x 1024 with M = 1024 per system.  The stock
state merges bodies in every step (262144 -> about 131000 in three), so every round starts from a fresh upload and runs the
same K steps; a figure is the median of 3 rounds after a warm-up round, with the spread (max - min).  K = 1 is the step the
one expectation is about: profiles/field_probe.txt has 65536 explicit points on the N = 262144 state at 13.9 ms of field_at
against 28.7 ms for a step, and the advance is that walk plus an epilogue, so the first step's overhead should be that of
one field(points) kernel on the same state - measured here in the same run as a whole field(points) call.
The host loop waits for the device in every step, which also tells the host the exact body count for the next step's grids;
K steps enqueued at once run under the upload's count as the bound.  On the stock state that favours the host loop from the
second step on; the K = 1 lines are free of it."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 3
N_ONE, BATCH_S, BATCH_N = 262144, 256, 1024


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[-1] - xs[0]


def rounds(prepare, run, sync):
    """ms of run() between two syncs, per round: a warm-up round, then ROUNDS measured ones, each after prepare()."""
    ms = []
    for r in range(ROUNDS + 1):
        prepare()
        sync()
        t0 = time.perf_counter()
        run()
        sync()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main(out_path):
    import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    import numpy as np
    import ppa_nbody_collisions_amd as nb
    import tracer_cases as tc

    lines = ["# csrc/tune/tracer_probe.py on one MI355X, fp32, host clock between two syncs; ms per step, median of %d rounds "
             "(spread), every round from a fresh upload" % ROUNDS]
    lines.append("# the host loop waits for the device in every step, so its steps are enqueued with the exact body count; plain stepping and the tracers' enqueue K steps at once with the count of the upload as the grids' bound - on this state, which halves in three steps, that is in the host loop's favour from the second step on (K = 4)")

    def shape(what, st, upload, cfg, pos, K, acc_of):
        """acc_of(field result) -> the (m, 2) accelerations the host loop's numpy update uses."""
        dt, wh = tc.dt_of(nb, cfg, nb.F32), (cfg.fieldWidth, cfg.fieldHeight)

        def host_loop():
            tr = {"pos": pos, "vel": np.zeros_like(pos)}
            for _ in range(K):
                tr = tc.advance(tr, acc_of(st.field(tr["pos"])), dt, False, wh)
                st.step(1)

        st.clear_tracers()
        plain = [x / K for x in rounds(upload, lambda: st.step(K), st.sync)]
        st.set_tracers(pos)
        with_t = [x / K for x in rounds(upload, lambda: st.step(K), st.sync)]
        st.clear_tracers()
        loop = [x / K for x in rounds(upload, host_loop, st.sync)]
        (p, ps), (w, ws), (l, ls) = med(plain), med(with_t), med(loop)
        line = ("%-40s K %2d  plain %8.3f (%.3f)  with tracers %8.3f (%.3f)  overhead %8.3f  host loop %8.3f (%.3f)  overhead "
                "%8.3f = %.2f x the tracers'" % (what, K, p, ps, w, ws, w - p, l, ls, l - p, (l - p) / (w - p)))
        lines.append(line)
        print(line, flush=True)
        return p, ps, w, ws

    cfg = nb.stock_config(particleCount=N_ONE)
    b = nb.init_bodies(cfg)
    st = nb.Stepper(cfg)
    for m in (65536, 1048576):
        pos = np.random.default_rng(m).uniform(0, 1, size=(m, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
        for K in (1, 4):
            p, ps, w, ws = shape("N=%d, M=%d" % (N_ONE, m), st, lambda: st.upload(b), cfg, pos, K, lambda f: f["acc"])
            if K == 1:
                call = rounds(lambda: st.upload(b), lambda: st.field(pos), st.sync)
                c, cs = med(call)
                ok = w - p <= c + ws + ps + cs
                line = ("#   expectation, first step: overhead %.3f against one field(%d points) call %.3f (%.3f) on the same "
                        "state: %s; %.3f of the plain step (field_probe.txt: 13.9 / 28.7 = 0.484 at M = 65536)"
                        % (w - p, m, c, cs, "within" if ok else "ABOVE the expectation", (w - p) / p))
                lines.append(line)
                print(line, flush=True)
    st.close()

    bcfg = nb.stock_config(particleCount=BATCH_N)
    bodies = [nb.init_bodies(bcfg, seed=100 + s) for s in range(BATCH_S)]
    batch = nb.StepperBatch(BATCH_S, BATCH_N, cfg=bcfg)
    pos = np.random.default_rng(7).uniform(0, 1, size=(BATCH_N, 2)) * [bcfg.fieldWidth, bcfg.fieldHeight]
    # the host loop of a batch: one field() call serves every system only while all have the same points, so the loop gives
    # every system the one (m, 2) set and follows system 0's update - a lower bound of what S different sets would cost
    shape("batch %d x %d, M=%d per system" % (BATCH_S, BATCH_N, BATCH_N), batch, lambda: batch.upload(bodies), bcfg, pos, 20,
          lambda f: f["acc"][0])
    batch.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tracer_probe.txt"))
