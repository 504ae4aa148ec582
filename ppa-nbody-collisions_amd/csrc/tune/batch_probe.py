#!/usr/bin/env python3
"""Ensembles of small systems: one StepperBatch against the best that could be done before it, S Stepper contexts.

    python3 csrc/tune/batch_probe.py --baseline-root DIR [--shapes 1024x256,256x1024,64x4096,16x16384] [--rounds 3]
    python3 csrc/tune/batch_probe.py --variants            (the batch kernel's K = 1, 2, 4, 8 side by side, no baseline)
    python3 csrc/tune/batch_probe.py --trace 256x1024      (a short candidate run, target of rocprofv3 --kernel-trace --stats)

DIR is a checkout of the commit BEFORE the batched stepper, built (make -C ppa-nbody-collisions_amd/csrc): the baseline
runs that library, in a child process of its own that loads it by path - two builds of one library do not share a
process.  The child stays alive and the two sides take turns, round by round, in the same GPU call.

Shapes are S x N: S systems of N bodies, the stock configuration (collisions on) and the same with radii 0, fp32,
literal semantics, seeds 1..S.
    baseline   S contexts, a stream each; every ensemble step enqueues step(1) on all of them; ONE synchronisation of
               all of them at the end of the window
    candidate  one StepperBatch: step(W), sync
Both start every window from a fresh upload.  The baseline is host-bound and slow, so its window is the first Wb steps;
the candidate is timed twice: over the same Wb steps ("same window") and over the first Wc >= Wb steps, Wc chosen so
that the window is more than 0.5 s of work ("long window").  Before any time is reported the states after Wb steps
must be bit-equal (sha256 over every system's downloaded block and count).  Host clock around work that ends in a
synchronise; medians over the rounds, and the spread (max - min) of the baseline's own rounds.
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


def load_package(root):
    sys.path.insert(0, root)
    import ppa_nbody_collisions_amd as nb
    return nb


def make_systems(nb, S, N, radii0):
    over = dict(minRadius=0.0, maxRadius=0.0) if radii0 else {}
    cfg = nb.stock_config(particleCount=N, **over)
    if hasattr(nb.lib, "nbody_init_bodies_seeded"):
        bodies = [nb.init_bodies(cfg, seed=1 + s) for s in range(S)]
    else:
        bodies = [seeded_init(nb, cfg, 1 + s) for s in range(S)]
    return cfg, bodies


def seeded_init(nb, cfg, seed):
    """init_bodies(seed=...) for a library that does not have it yet: the same draws, x, y, m, r per body (fp32)."""
    import ctypes
    import numpy as np
    g = nb.Rng()
    nb.lib.nbody_rng_seed(ctypes.byref(g), seed)
    n = cfg.particleCount
    b = nb.BodiesData(n)
    draw = lambda lo, hi: nb.lib.nbody_rng_fval_range(ctypes.byref(g), float(lo), float(hi))   # noqa: E731
    P, M, R = b.Positions, b.Masses, b.Radii
    for i in range(n):
        P[i, 0] = np.float32(draw(0, cfg.fieldWidth << 1) - cfg.fieldWidth)
        P[i, 1] = np.float32(draw(0, cfg.fieldHeight << 1) - cfg.fieldHeight)
        M[i] = np.float32(draw(cfg.minRandBodyMass, cfg.maxRandBodyMass))
        R[i] = np.float32(draw(cfg.minRadius, cfg.maxRadius))
    return b


def digest(blocks):
    h = hashlib.sha256()
    for b in blocks:
        h.update(b"%d:" % b.numBodies)
        h.update(b.block.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------
# baseline side: a child process on the older library
# ---------------------------------------------------------------------------------------------------------
def baseline_child(root):
    nb = load_package(root)
    assert not hasattr(nb, "StepperBatch"), "the baseline root already has the batched stepper"
    ctxs, bodies = [], []
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "setup":
            for st in ctxs:
                st.close()
            cfg, bodies = make_systems(nb, cmd["S"], cmd["N"], cmd["radii0"])
            ctxs = [nb.Stepper(cfg, event_capacity=1024) for _ in range(cmd["S"])]
            reply = {"kernel": ctxs[0].force_kernel_name()}
        elif cmd["op"] == "window":
            for st, bd in zip(ctxs, bodies):
                st.upload(bd)
            for st in ctxs:
                st.sync()
            step, handles = nb.lib.nbody_step, [st._ctx for st in ctxs]
            t0 = time.perf_counter()
            for _ in range(cmd["steps"]):
                for h in handles:
                    step(h, 1)
            for st in ctxs:
                st.sync()
            t1 = time.perf_counter()
            reply = {"seconds": t1 - t0, "digest": digest([st.download() for st in ctxs])}
        else:
            break
        sys.stdout.write(json.dumps(reply) + "\n")
        sys.stdout.flush()
    for st in ctxs:
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
def candidate_window(b, bodies, steps, want_digest=False):
    b.upload(bodies)
    b.sync()
    t0 = time.perf_counter()
    b.step(steps)
    b.sync()
    t1 = time.perf_counter()
    return t1 - t0, (digest(b.download_all()) if want_digest else None)


def pairs_per_step(nb, N):
    """Ordered pairs one literal step evaluates (src/nbody.cu:473 and quirk Q1: the last tile is N % 129 long)."""
    nblk = 1 if N < 128 else N // 128
    active = N if N < 128 else nblk * 128
    per_body = 0
    for k in range(nblk):
        L = N % 129 if k == nblk - 1 else 128
        per_body += max(L - 1, 0) if k == 0 else L         # the first walk position of tile 0 is the body itself
    return active * per_body


def probe_shape(nb, base, S, N, radii0, rounds, wb_budget_s, lanes=0):
    cfg, bodies = make_systems(nb, S, N, radii0)
    out = {"S": S, "N": N, "radii": "0" if radii0 else "stock"}
    with nb.StepperBatch(S, N, cfg=cfg, kernel_variant=lanes) as b:
        out["candidate_kernel"] = b.kernel_name()
        candidate_window(b, bodies, 20)                                    # warm
        t20, _ = candidate_window(b, bodies, 20)
        wc = max(20, int(0.6 / (t20 / 20)) + 1)                            # > 0.5 s of candidate work
        wb = wc
        if base is not None:
            out["baseline_kernel"] = base.ask(op="setup", S=S, N=N, radii0=radii0)["kernel"]
            warm = base.ask(op="window", steps=5)                          # warm, and the baseline's rate
            wb = max(5, min(wc, int(wb_budget_s / (warm["seconds"] / 5))))
        out["steps_baseline_window"], out["steps_long_window"] = wb, wc
        t_base, t_same, t_long = [], [], []
        for r in range(rounds):                                            # the two sides take turns
            if base is not None:
                rb = base.ask(op="window", steps=wb)
                ts, dg = candidate_window(b, bodies, wb, want_digest=True)
                if dg != rb["digest"]:
                    raise SystemExit("%dx%d radii %s round %d: states after %d steps differ - no time is reported"
                                     % (S, N, out["radii"], r, wb))
                t_base.append(rb["seconds"] / wb)
                t_same.append(ts / wb)
            tl, _ = candidate_window(b, bodies, wc)
            t_long.append(tl / wc)
    us = lambda xs: [round(x * 1e6, 2) for x in xs]                                # noqa: E731
    out["candidate_us_per_step_long_window"] = us(t_long)
    out["candidate_median_us"] = round(statistics.median(t_long) * 1e6, 2)
    if base is not None:
        out["states_bit_equal_after_baseline_window"] = True
        out["baseline_us_per_step"] = us(t_base)
        out["candidate_us_per_step_same_window"] = us(t_same)
        out["baseline_median_us"] = round(statistics.median(t_base) * 1e6, 2)
        out["baseline_spread_us"] = round((max(t_base) - min(t_base)) * 1e6, 2)
        out["candidate_same_window_median_us"] = round(statistics.median(t_same) * 1e6, 2)
        # like for like: both sides over the SAME steps (with stock radii bodies merge, later steps are cheaper)
        out["gain_same_window_us"] = round(out["baseline_median_us"] - out["candidate_same_window_median_us"], 2)
        out["ratio_baseline_over_candidate_same_window"] = round(out["baseline_median_us"] / out["candidate_same_window_median_us"], 2)
        out["faster_by_more_than_baseline_spread"] = out["gain_same_window_us"] > out["baseline_spread_us"]
    # whole ensemble step (force + commit launches), not the force kernel alone: that split is rocprofv3's
    out["pairs_per_ensemble_step_at_upload"] = S * pairs_per_step(nb, N)
    out["ensemble_step_pair_rate_per_s"] = float("%.4g" % (out["pairs_per_ensemble_step_at_upload"] / statistics.median(t_long)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--baseline-root")
    ap.add_argument("--shapes", default="1024x256,256x1024,64x4096,16x16384")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--baseline-window-seconds", type=float, default=2.0)
    ap.add_argument("--variants", action="store_true")
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
        cfg, bodies = make_systems(nb, S, N, False)
        with nb.StepperBatch(S, N, cfg=cfg) as b:
            t, _ = candidate_window(b, bodies, 200)
            emit({"trace": a.trace, "steps": 200, "kernel": b.kernel_name(), "us_per_step_under_the_profiler": round(t / 200 * 1e6, 2),
                  "pairs_per_ensemble_step_at_upload": S * pairs_per_step(nb, N)})
    elif a.variants:
        for shape in a.shapes.split(","):
            S, N = (int(x) for x in shape.split("x"))
            for lanes in (1, 2, 4, 8):
                r = probe_shape(nb, None, S, N, False, a.rounds, 0.0, lanes)
                emit({k: r[k] for k in ("S", "N", "candidate_kernel", "steps_long_window", "candidate_us_per_step_long_window",
                                        "candidate_median_us")})
    else:
        if not a.baseline_root:
            ap.error("--baseline-root DIR (a built checkout of the commit before the batched stepper)")
        base = Baseline(os.path.abspath(a.baseline_root))
        try:
            for shape in a.shapes.split(","):
                S, N = (int(x) for x in shape.split("x"))
                for radii0 in (False, True):
                    emit(probe_shape(nb, base, S, N, radii0, a.rounds, a.baseline_window_seconds))
        finally:
            base.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
