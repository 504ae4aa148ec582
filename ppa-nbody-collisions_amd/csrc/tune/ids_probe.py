#!/usr/bin/env python3
"""What body identities (NBODY_FLAG_TRACK_IDS) cost per step, and that they cost nothing when they are off.

    python3 csrc/tune/ids_probe.py --baseline-root DIR [--shapes ctx262144,ctx1024,256x1024,64x4096] [--rounds 3]
    python3 csrc/tune/ids_probe.py --trace 256x1024      (a short tracked run, target of rocprofv3 --kernel-trace --stats)

DIR is a checkout of the commit BEFORE the identities, built (make -C ppa-nbody-collisions_amd/csrc): the baseline runs
that library, in a child process of its own that loads it by path - two builds of one library do not share a process.
The `off` side runs in a child process of the same kind on this library, so that the two sides of the "no cost when unused"
comparison differ in the library alone.  The children stay alive and the sides take turns, round by round, in the same GPU
call.

Shapes: ctxN is one Stepper of N bodies, SxN one StepperBatch of S systems of N bodies; the stock configuration (stock
radii), fp32, literal semantics, the event log on (so that a tracked step carries both of its launches), seeds 1..S.
Three sides run the same window - upload, synchronise, clock, step(W), synchronise, clock:
    parent   the baseline library (it has no flag), child process
    control  the baseline library once more, in a second child process: parent against itself, i.e. what two processes
             on one library differ by (buffers land elsewhere) - the yardstick next to the parent's round-to-round spread
    off      this library, track_ids=False, child process  -> against `parent`: inside the parent's own round-to-round spread?
    on       this library, track_ids=True, this process    -> against `off`: the cost of the feature, us per step
Before any time is reported the final states of the three sides must be bit-equal (sha256 of every system's download).
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
WINDOW = {"ctx262144": 20, "ctx1024": 2000, "256x1024": 1000, "64x4096": 500}     # steps per timed window: ~0.1 to 0.7 s


def load_package(root):
    sys.path.insert(0, root)
    try:
        import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    except ImportError:
        pass
    import ppa_nbody_collisions_amd as nb
    return nb


def parse_shape(shape):
    if shape.startswith("ctx"):
        return 0, int(shape[3:])
    S, N = (int(x) for x in shape.split("x"))
    return S, N


class Side:
    """One stepper (Stepper or StepperBatch) and the bodies it is re-uploaded with for every window."""

    def __init__(self, nb, shape, track):
        self.S, self.N = parse_shape(shape)
        cfg = nb.stock_config(particleCount=self.N)
        kw = dict(track_ids=True) if track else {}
        if self.S == 0:
            self.bodies = nb.init_bodies(cfg, seed=1)
            self.st = nb.Stepper(cfg, record_events=True, **kw)
            self.name = self.st.force_kernel_name()
        else:
            self.bodies = [nb.init_bodies(cfg, seed=1 + s) for s in range(self.S)]
            self.st = nb.StepperBatch(self.S, self.N, cfg=cfg, record_events=True, **kw)
            self.name = self.st.kernel_name()

    def window(self, steps):
        self.st.upload(self.bodies)
        self.st.sync()
        t0 = time.perf_counter()
        self.st.step(steps)
        self.st.sync()
        seconds = time.perf_counter() - t0
        h = hashlib.sha256()
        outs = [self.st.download()] if self.S == 0 else self.st.download_all()
        for o in outs:
            h.update(b"%d:" % o.numBodies)
            h.update(o.block.tobytes())
        return seconds, h.hexdigest(), sum(o.numBodies for o in outs)

    def close(self):
        self.st.close()


def child(root):
    nb = load_package(root)
    if os.path.abspath(root) != ROOT:
        assert not hasattr(nb, "FLAG_TRACK_IDS"), "the baseline root already has the identities"
    side = None
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "setup":
            if side is not None:
                side.close()
            side = Side(nb, cmd["shape"], False)
            side.window(cmd["steps"])                                      # warm: code objects, lazy buffers
            reply = {"kernel": side.name}
        elif cmd["op"] == "window":
            seconds, digest, _ = side.window(cmd["steps"])
            reply = {"seconds": seconds, "digest": digest}
        else:
            break
        sys.stdout.write(json.dumps(reply) + "\n")
        sys.stdout.flush()
    if side is not None:
        side.close()


class Child:
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
            raise SystemExit("child process did not answer %r (exit status %r): nothing more is started" % (cmd, self.p.poll()))
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def probe_shape(nb, base, control, off, shape, rounds):
    steps = WINDOW.get(shape, 200)
    on = Side(nb, shape, True)
    base.ask(op="setup", shape=shape, steps=steps)
    control.ask(op="setup", shape=shape, steps=steps)
    off.ask(op="setup", shape=shape, steps=steps)
    on.window(steps)                                                       # warm
    t = {"parent": [], "control": [], "off": [], "on": []}
    left = None
    for r in range(rounds):                                                # the sides take turns
        rb = base.ask(op="window", steps=steps)
        rc = control.ask(op="window", steps=steps)
        ro = off.ask(op="window", steps=steps)
        s_off, d_off = ro["seconds"], ro["digest"]
        s_on, d_on, left = on.window(steps)
        if not (rb["digest"] == rc["digest"] == d_off == d_on):
            raise SystemExit("%s round %d: the final states differ - no time is reported" % (shape, r))
        t["parent"].append(rb["seconds"])
        t["control"].append(rc["seconds"])
        t["off"].append(s_off)
        t["on"].append(s_on)
    ids_moved = None
    if on.S == 0:
        import numpy as np
        ids = on.st.ids()
        ids_moved = int((ids != np.arange(len(ids))).sum())
    on.close()
    us = lambda xs: [round(x / steps * 1e6, 2) for x in xs]                        # noqa: E731
    med = {k: statistics.median(us(v)) for k, v in t.items()}
    out = {"shape": shape, "steps_per_window": steps, "kernel": on.name, "states_bit_equal": True,
           "bodies_left": left, "ids_not_at_their_index": ids_moved,
           "parent_us_per_step": us(t["parent"]), "control_us_per_step": us(t["control"]), "off_us_per_step": us(t["off"]), "on_us_per_step": us(t["on"]),
           "parent_median": med["parent"], "control_median": med["control"], "off_median": med["off"], "on_median": med["on"],
           "parent_spread": round(max(us(t["parent"])) - min(us(t["parent"])), 2),
           "control_minus_parent": round(med["control"] - med["parent"], 2),
           "off_minus_parent": round(med["off"] - med["parent"], 2),
           "on_minus_off_us_per_step": round(med["on"] - med["off"], 2)}
    out["off_inside_parent_spread"] = abs(out["off_minus_parent"]) <= out["parent_spread"]
    out["off_no_further_from_parent_than_control"] = abs(out["off_minus_parent"]) <= max(abs(out["control_minus_parent"]),
                                                                                         out["parent_spread"])
    return out


def trace_run(nb, shape, steps=200):
    """What the profiler looks at: `steps` tracked steps from the upload, enqueued in one go."""
    side = Side(nb, shape, True)
    seconds, _, left = side.window(steps)
    rec = {"trace": shape, "kernel": side.name, "steps": steps, "us_per_step": round(seconds / steps * 1e6, 2),
           "bodies_left": left}
    side.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--baseline-root")
    ap.add_argument("--shapes", default="ctx262144,ctx1024,256x1024,64x4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace")
    ap.add_argument("--out", help="append the result lines to this file as well")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    nb = load_package(ROOT)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    if a.trace:
        emit(trace_run(nb, a.trace))
    else:
        if not a.baseline_root:
            ap.error("--baseline-root DIR (a built checkout of the commit before the identities)")
        if a.rounds < 3:
            ap.error("at least 3 rounds")
        base, control, off = Child(os.path.abspath(a.baseline_root)), Child(os.path.abspath(a.baseline_root)), Child(ROOT)
        try:
            for shape in a.shapes.split(","):
                emit(probe_shape(nb, base, control, off, shape, a.rounds))
        finally:
            for side in (base, control, off):
                side.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
