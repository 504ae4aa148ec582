#!/usr/bin/env python3
"""This library against the parent commit's, on the work of the kernels that share a rule with another kernel: the
compaction's offsets (compact_count / compact_scatter, batch_count / batch_commit, ids_scatter), the potential's walk
(diag_potential, batch_diag_potential, track_potential, and with it field_at, tides_at and tracers_advance: the ordered
walk and the exact walk of nbody_diag.hpp), the finish of the diagnostics (batch_diag_reduce) and the row queries'
prologue, tile walk and host drivers (field_at, neighbors_at, groups_sweep, pair_counts, encounters_walk, binaries_walk,
group_potential, shells_at, shell_moments_at; nbody_rows.hpp), and the cell list with the three queries on it - the cell sums,
the radius queries and the groups on the grid (nbody_cells.hpp, nbody_within.hpp, nbody_groups_grid.hpp), which share the
list's view, its window walk and its sorted records, and whose buffers are the handles' to keep and free.

    python3 csrc/tune/ab_parent.py --baseline-root DIR [--lines a,b256,...] [--rounds 3] [--out FILE]
    python3 csrc/tune/ab_parent.py --trace [--root DIR]     (every line once, target of rocprofv3 --kernel-trace --stats)

DIR is a built checkout of the parent commit (make -C ppa-nbody-collisions_amd/csrc).  Three child processes, each loading
one library by path (two builds of one library do not share a process), stay alive and take turns round by round in the same
GPU call:
    parent     the baseline library
    control    the baseline library once more: what two processes on ONE library differ by (buffers land elsewhere)
    candidate  this library
Every line is warmed up on every side, and the results of the three sides must be bit-equal (sha256) in every round before
a time is taken.  Time is a host clock around work that ends in a synchronise; a window repeats the call often enough to
last 0.1 s or more.  Round r starts with side r mod 3, so that with 3 rounds every side has had every place in the turn.

Lines (fp32, literal, stock configuration with stock radii):
    a         Stepper N = 262144, diagnostics(potential=True)                              ms per call
    b256, b64 StepperBatch 256 x 1024 / 64 x 4096 after 3 steps: diagnostics() and         ms per call
              diagnostics(potential=True) (lines b256, b256phi, b64, b64phi)
    c         Stepper N = 262144 after 8 steps, record_tracks() with phi on 64 evenly      ms per record
              spread identities
    d...      stepping with record_events and track_ids from a fresh upload: dctx262144    us per step
              (20 steps), dctx1024 (2000), d256x1024 (1000), d64x4096 (500)
    fld, nbr  Stepper N = 262144, field() / neighbors(); ...pts: the same state with 65536  ms per call
              explicit points; ...256: StepperBatch 256 x 1024 after 3 steps, points=None
    grp, prs  the shapes of groups_probe.py and pairs_probe.py: Stepper N = 262144 after 3      ms per call
              steps, groups(0, 1) / pair_counts() over the 32 "sparse" bins; prspts: the same
              bins from 65536 explicit points; ...256: StepperBatch 256 x 1024 after 3 steps
    enc, bin  the shapes of encounter_probe.py and binary_probe.py on the grp state: encounters(h  ms per call
              = the time step) and binaries(128), binaries(1024) for the batch (the probe's sep
              / 8 and sep), each with room for its list: one walk per call
    gpe       group_energy_probe.py's overlap case, group_potential(0, 1), on the grp state     ms per call
    shl, shm  the shapes of shells_probe.py and shell_moments_probe.py on the grp state: shells() ms per call
              / shell_moments() over 8 bins below the prs top edge; shlpts: 32 bins from 65536
              explicit points; shmpts: 8 bins from 65536 moving points; ...256 as above
    tid, tidj the shapes of tides_probe.py: Stepper N = 262144, tides() / tides(jerk=True); tidpts,   ms per call
              tidjpts: the same state with 65536 explicit points, tidjpts' moving; tid256,
              tidj256: StepperBatch 256 x 1024 after 3 steps, points=None
    cel, wth  the shapes of cells_probe.py and within_probe.py: Stepper N = 262144, cells() on the   ms per call
              256 x 256 grid over the field with moments and lists / within(h = that grid's cell
              side) on that grid with lists; wthpts: the same from 65536 explicit points; cel256,
              wth256: StepperBatch 256 x 1024 after 3 steps on 32 x 32 cells, h = the cell side
    ggr       the matched grid of groups_grid_probe.py's overlap case on the grp state: groups(0, 1,        ms per call
              grid=groups_grid(the field widened to the bodies, 0, 1, the median radius)); ggr256: the
              same on StepperBatch 256 x 1024 after 3 steps, one grid of at most 128 x 128 cells
    kng       the shape of knn_grid_probe.py: Stepper N = 262144, knn(8, grid=knn_grid(the field, 8, n));   ms per call
              kng256: StepperBatch 256 x 1024 after 3 steps, knn(8) on 32 x 32 cells over the field
    trc       stepping with 65536 tracers set, from a fresh upload and a fresh set: trc Stepper  ms | us per step
              N = 262144 (8 steps), trc256 StepperBatch 256 x 1024 with 256 tracers in each
              system (500 steps)
    io...     upload followed by download, the host path of nbody_block_pack / _unpack: io Stepper   ms per round trip
              N = 262144 fp32, io64 the same in fp64, io256 StepperBatch 256 x 1024 with every
              system downloaded; the digest is over the downloaded blocks
A line passes when the candidate's median is not above the parent's median by more than max(the parent's round spread
(max - min), |control median - parent median|).  Exit status 1 if a line does not pass.
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
LINES = ("a", "b256", "b256phi", "b64", "b64phi", "c", "dctx262144", "dctx1024", "d256x1024", "d64x4096",
         "fld", "fldpts", "fld256", "nbr", "nbrpts", "nbr256", "grp", "grp256", "prs", "prspts", "prs256",
         "enc", "enc256", "bin", "bin256", "gpe", "gpe256", "shl", "shlpts", "shl256", "shm", "shmpts", "shm256",
         "tid", "tidj", "tidpts", "tidjpts", "tid256", "tidj256", "cel", "cel256", "wth", "wthpts", "wth256", "ggr", "ggr256",
         "kng", "kng256", "trc", "trc256", "io", "io64", "io256")
BATCH = {"b256": (256, 1024), "b64": (64, 4096)}
STEPS = {"dctx262144": 20, "dctx1024": 2000, "d256x1024": 1000, "d64x4096": 500}
IO = {"io": 20, "io64": 12, "io256": 20}     # round trips per window
TRACERS = {"trc": 8, "trc256": 500}     # steps per window with M_POINTS tracers set
ROWS = {"": 3, "pts": 8, "256": 100}    # the row queries' shapes (field_probe.py, neighbor_probe.py): calls per window;
                                        # the tides' too: 51 to 71 ms a call on own rows, 16 to 21 on the points
SCANS = {"grp": 8, "grp256": 100, "prs": 20, "prspts": 30, "prs256": 200,     # the queries on the state after 3 steps:
         "enc": 6, "enc256": 100, "bin": 20, "bin256": 80, "gpe": 6, "gpe256": 80,    # calls per window
         "shl": 20, "shlpts": 20, "shl256": 60, "shm": 20, "shmpts": 20, "shm256": 40,
         "ggr": 200, "ggr256": 100}             # profiles/groups_grid_probe.txt: 0.67 and 1.2 ms a call on the matched grid
# whole cells() / within() calls (profiles/cells_probe.txt, profiles/within_probe.txt): 0.62 and 1.2 ms a call for cel and
# cel256, 1.4 ms for wth and wth256 with their lists; wthpts builds the same cell list for a quarter of the rows
GRIDS = {"cel": 250, "cel256": 120, "wth": 100, "wthpts": 250, "wth256": 100,
         "kng": 60, "kng256": 60}               # profiles/knn_grid_probe.txt: whole knn(8, grid=...) calls, a few ms each
ROW_LINES = ("fld", "nbr", "grp", "prs", "enc", "bin", "gpe", "shl", "shm", "tid", "cel", "wth", "ggr", "kng")
N_BIG = 262144
M_POINTS = 65536


def load_package(root):
    sys.path.insert(0, root)
    try:
        import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    except ImportError:
        pass
    import ppa_nbody_collisions_amd as nb
    assert os.path.abspath(nb.__file__).startswith(os.path.abspath(root) + os.sep), (nb.__file__, root)
    return nb


def digest_of(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
    return h.hexdigest()


def diag_parts(d):
    out = []
    for k in sorted(d):
        out.append(d[k].tobytes() if hasattr(d[k], "tobytes") else repr(d[k]).encode())
    return out


def result_parts(r):
    """What a query returned - an array, a dict, or a list or tuple of those - as the parts of a digest."""
    if isinstance(r, dict):
        return diag_parts(r)
    if isinstance(r, (list, tuple)):
        return [p for e in r for p in result_parts(e)]
    return [r.tobytes()]


class Line:
    """One line of the table: setup() builds the state, window() times the work once and digests what it gave."""

    def __init__(self, nb, name, short=False):
        import numpy as np
        self.nb, self.name, self.np = nb, name, np
        self.batch = None
        if name == "a" or name == "c":
            cfg = nb.stock_config(particleCount=N_BIG)
            self.st = nb.Stepper(cfg, track_ids=(name == "c"))
            self.st.upload(nb.init_bodies(cfg, seed=1))
            self.unit, self.reps = ("ms per call", 5) if name == "a" else ("ms per record", 32)
            if name == "c":
                self.st.step(8)
                self.sel = [int(x) for x in np.unique(np.linspace(0, N_BIG - 1, 64).astype(np.int32))]
        elif name[:3] in ROW_LINES:
            self.unit, self.reps = "ms per call", {**SCANS, **GRIDS}.get(name) or ROWS[name[3:].lstrip("j")]
            self.pts = None
            if name.endswith("256"):
                cfg = nb.stock_config(particleCount=1024)
                self.st = self.batch = nb.StepperBatch(256, 1024, cfg=cfg)
                self.st.upload([nb.init_bodies(cfg, seed=100 + s) for s in range(256)])
                self.st.step(3)
            else:
                cfg = nb.stock_config(particleCount=N_BIG)
                self.st = nb.Stepper(cfg)
                self.st.upload(nb.init_bodies(cfg, seed=1))
                if name in SCANS:
                    self.st.step(3)
                if name.endswith("pts"):
                    self.pts = np.random.default_rng(2).uniform(0, 1, size=(M_POINTS, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
            if name.startswith("grp"):
                self.call = lambda pts: self.st.groups(0.0, 1.0)
            elif name.startswith("gpe"):
                self.call = lambda pts: self.st.group_potential(0.0, 1.0)
            elif name.startswith("ggr"):                                    # groups_grid_probe.py: nothing is outside the grid
                downs = [self.st.download(s) for s in range(256)] if self.batch else [self.st.download()]
                P = [np.abs(np.asarray(d.Positions[:d.numBodies], dtype=np.float64).reshape(-1, 2)) for d in downs]
                median = float(np.median(np.asarray(downs[0].Radii[:downs[0].numBodies], dtype=np.float64)))
                if self.batch:
                    reach = max(float(p.max()) for p in P) * 1.001
                    field = (max(float(cfg.fieldWidth), reach), max(float(cfg.fieldHeight), reach))
                    grid = nb.groups_grid(field, 0.0, 1.0, median, most=int(np.sqrt((1 << 22) // 256)))
                else:
                    field = (max(float(cfg.fieldWidth), float(P[0][:, 0].max()) * 1.001), max(float(cfg.fieldHeight), float(P[0][:, 1].max()) * 1.001))
                    grid = nb.groups_grid(field, 0.0, 1.0, median)
                self.call = lambda pts: self.st.groups(0.0, 1.0, grid=grid)
            elif name[:3] in ("enc", "bin"):
                if name.startswith("enc"):
                    query = lambda cap: self.st.encounters(float(np.float32(cfg.timestep)), cap=cap)
                else:
                    query = lambda cap: self.st.binaries(1024.0 if self.batch else 128.0, cap=cap)
                found = query(None)
                cap = max([g[1]["pairs"] for g in (found if self.batch else [found])] + [1])    # room for the list: one walk
                self.call = lambda pts: query(cap)
            elif name[:3] in ("prs", "shl", "shm"):                         # pairs_probe.py's (a): 1.5 others within the top edge
                down = self.st.download(0) if self.batch else self.st.download()
                P = np.asarray(down.Positions, dtype=np.float64)
                top = float(np.sqrt(1.5 * np.prod(P.max(axis=0) - P.min(axis=0)) / (np.pi * len(P))))
                e2 = np.geomspace(top / 1000.0, top, 9 if name in ("shl", "shl256") or name.startswith("shm") else 33) ** 2
                if name.startswith("prs"):
                    self.call = lambda pts: self.st.pair_counts(e2, points=pts, squared=True)
                elif name.startswith("shl"):
                    self.call = lambda pts: self.st.shells(e2, pts, squared=True)
                else:
                    vel = None
                    if self.pts is not None:
                        vel = np.random.default_rng(3).uniform(-1, 1, size=(M_POINTS, 2)) * np.abs(np.asarray(down.Velocities)).max()
                    self.call = lambda pts: self.st.shell_moments(e2, pts, vel, squared=True)
            elif name[:3] in ("cel", "wth"):
                nx, W = 32 if self.batch else 256, float(cfg.fieldWidth)
                grid = nb.make_grid(nx, nx, (-W, W, -W, W))
                if name.startswith("cel"):
                    self.call = lambda pts: self.st.cells(grid, lists=True)
                else:
                    self.call = lambda pts: self.st.within(2.0 * W / nx, pts, grid=grid, lists=True)
            elif name.startswith("kng"):                                    # knn_grid_probe.py: k = 8 on the matched grid
                W = float(cfg.fieldWidth)
                grid = nb.make_grid(32, 32, (-W, W, -W, W)) if self.batch else nb.knn_grid((W, W), 8, N_BIG)
                self.call = lambda pts: self.st.knn(8, pts, grid=grid)
            elif name.startswith("tid"):
                jerk, vel = name[3:4] == "j", None
                if jerk and self.pts is not None:
                    vel = np.random.default_rng(3).uniform(-1, 1, size=(M_POINTS, 2)) * np.abs(np.asarray(self.st.download().Velocities)).max()
                self.call = lambda pts: self.st.tides(pts, vel, jerk=jerk)
            else:
                self.call = self.st.field if name.startswith("fld") else self.st.neighbors
        elif name in TRACERS:
            self.steps = min(200, TRACERS[name]) if short else TRACERS[name]
            if name.endswith("256"):
                cfg = nb.stock_config(particleCount=1024)
                self.bodies = [nb.init_bodies(cfg, seed=100 + s) for s in range(256)]
                self.st = self.batch = nb.StepperBatch(256, 1024, cfg=cfg)
                self.unit, m = "us per step", M_POINTS // 256           # the one set for every system
            else:
                cfg = nb.stock_config(particleCount=N_BIG)
                self.bodies = nb.init_bodies(cfg, seed=1)
                self.st = nb.Stepper(cfg)
                self.unit, m = "ms per step", M_POINTS
            self.reps = self.steps
            self.pts = np.random.default_rng(2).uniform(0, 1, size=(m, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
        elif name in IO:
            self.unit, self.reps = "ms per round trip", IO[name]
            if name == "io256":
                cfg = nb.stock_config(particleCount=1024)
                self.bodies = [nb.init_bodies(cfg, seed=1 + s) for s in range(256)]
                self.st = self.batch = nb.StepperBatch(256, 1024, cfg=cfg)
            else:
                precision = nb.F64 if name == "io64" else nb.F32
                cfg = nb.stock_config(particleCount=N_BIG)
                self.bodies = nb.init_bodies(cfg, precision, seed=1)
                self.st = nb.Stepper(cfg, precision=precision)
            self.st.upload(self.bodies)
        elif name in STEPS:
            shape = name[1:]
            self.steps = 200 if short else STEPS[name]
            self.unit, self.reps = "us per step", self.steps
            kw = dict(record_events=True, track_ids=True)
            if shape.startswith("ctx"):
                cfg = nb.stock_config(particleCount=int(shape[3:]))
                self.bodies = nb.init_bodies(cfg, seed=1)
                self.st = nb.Stepper(cfg, **kw)
            else:
                S, N = (int(x) for x in shape.split("x"))
                cfg = nb.stock_config(particleCount=N)
                self.bodies = [nb.init_bodies(cfg, seed=1 + s) for s in range(S)]
                self.st = self.batch = nb.StepperBatch(S, N, cfg=cfg, **kw)
        else:
            S, N = BATCH[name.replace("phi", "")]
            cfg = nb.stock_config(particleCount=N)
            self.st = self.batch = nb.StepperBatch(S, N, cfg=cfg)
            self.st.upload([nb.init_bodies(cfg, seed=1 + s) for s in range(S)])
            self.st.step(3)
            self.phi = name.endswith("phi")
            self.unit, self.reps = "ms per call", 200
        self.st.sync()

    def window(self):
        """-> (seconds, digest)"""
        st, name = self.st, self.name
        if name in STEPS:
            st.upload(self.bodies)
            st.sync()
            t0 = time.perf_counter()
            st.step(self.steps)
            st.sync()
            seconds = time.perf_counter() - t0
            parts = []
            for s in range(self.batch.systems if self.batch else 1):
                o, ids = (st.download(s), st.ids(s)) if self.batch else (st.download(), st.ids())
                parts += [b"%d:" % o.numBodies, o.block.tobytes(), ids.tobytes()]
            return seconds, digest_of(parts)
        if name in IO:
            t0 = time.perf_counter()
            for _ in range(self.reps):                                      # both ends synchronise
                st.upload(self.bodies)
                got = [st.download(s) for s in range(self.batch.systems)] if self.batch else [st.download()]
            seconds = time.perf_counter() - t0
            return seconds, digest_of([p for o in got for p in (b"%d:" % o.numBodies, o.block.tobytes())])
        if name in TRACERS:
            st.upload(self.bodies)
            st.set_tracers(self.pts)                                        # zeroes their counters; synchronises
            st.sync()
            t0 = time.perf_counter()
            st.step(self.steps)
            st.sync()
            seconds = time.perf_counter() - t0
            return seconds, digest_of(result_parts(st.tracers()))
        if name[:3] in ROW_LINES:
            t0 = time.perf_counter()
            for _ in range(self.reps):                                      # each call ends in a copy back and a synchronise
                r = self.call(self.pts)
            seconds = time.perf_counter() - t0
            return seconds, digest_of(result_parts(r))
        if name == "c":
            st.reserve_tracks(self.reps, ids=self.sel, potential=True)      # empties the log; synchronises
            t0 = time.perf_counter()
            for _ in range(self.reps):
                st.record_tracks()
            st.sync()
            seconds = time.perf_counter() - t0
            t = st.tracks()
            return seconds, digest_of([t[k].tobytes() for k in sorted(t)])
        t0 = time.perf_counter()
        for _ in range(self.reps):                                          # each call ends in a copy back and a synchronise
            d = st.diagnostics(potential=True) if name == "a" else st.diagnostics(potential=self.phi)
        seconds = time.perf_counter() - t0
        return seconds, digest_of(diag_parts(d) if name == "a" else [p for e in d for p in diag_parts(e)])

    def value(self, seconds):
        return seconds / self.reps * (1e6 if self.unit.startswith("us") else 1e3)

    def close(self):
        self.st.close()


def child(root):
    nb = load_package(root)
    line = None
    for text in sys.stdin:
        cmd = json.loads(text)
        if cmd["op"] == "setup":
            if line is not None:
                line.close()
            line = Line(nb, cmd["line"])
            line.window()                                                   # warm: code objects, lazy buffers
            reply = {"unit": line.unit}
        elif cmd["op"] == "window":
            seconds, digest = line.window()
            reply = {"value": line.value(seconds), "digest": digest}
        else:
            break
        sys.stdout.write(json.dumps(reply) + "\n")
        sys.stdout.flush()
    if line is not None:
        line.close()


class Child:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", root], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        ready, _, _ = select.select([self.p.stdout], [], [], REPLY_TIMEOUT_S)
        text = self.p.stdout.readline() if ready else ""
        if not text:
            self.p.kill()
            raise SystemExit("child process did not answer %r (exit status %r): nothing more is started" % (cmd, self.p.poll()))
        return json.loads(text)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def probe_line(sides, name, rounds):
    unit = [side.ask(op="setup", line=name)["unit"] for side in sides.values()][0]
    t = {k: [] for k in sides}
    order = list(sides)
    for r in range(rounds):                                                 # the sides take turns, the first place too
        got = {k: sides[k].ask(op="window") for k in order[r % 3:] + order[:r % 3]}
        if len({g["digest"] for g in got.values()}) != 1:
            raise SystemExit("%s round %d: the results differ between the sides - no time is reported" % (name, r))
        for k, g in got.items():
            t[k].append(round(g["value"], 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = max(t["parent"]) - min(t["parent"])
    offset = abs(med["control"] - med["parent"])
    margin = max(spread, offset)
    return {"line": name, "unit": unit, "results_bit_equal": True, "parent": t["parent"], "control": t["control"],
            "candidate": t["candidate"], "parent_median": med["parent"], "control_median": med["control"],
            "candidate_median": med["candidate"], "parent_spread": round(spread, 4),
            "control_minus_parent": round(med["control"] - med["parent"], 4), "margin": round(margin, 4),
            "candidate_minus_parent": round(med["candidate"] - med["parent"], 4),
            "within_margin": med["candidate"] - med["parent"] <= margin}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--baseline-root")
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--root", default=ROOT, help="--trace: the checkout whose library is traced (default: this one)")
    ap.add_argument("--out", help="append the result lines to this file as well")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    names = a.lines.split(",")
    unknown = [n for n in names if n not in LINES]
    if unknown:
        ap.error("unknown lines %s (of %s)" % (unknown, ", ".join(LINES)))
    out = []

    def emit(rec):
        text = json.dumps(rec)
        print(text, flush=True)
        out.append(text)

    ok = True
    if a.trace:
        nb = load_package(os.path.abspath(a.root))
        for name in names:
            line = Line(nb, name, short=True)
            seconds, _ = line.window()
            emit({"trace": name, "root": os.path.abspath(a.root), "unit": line.unit, "value": round(line.value(seconds), 4)})
            line.close()
    else:
        if not a.baseline_root:
            ap.error("--baseline-root DIR (a built checkout of the parent commit)")
        if a.rounds < 3:
            ap.error("at least 3 rounds")
        base = os.path.abspath(a.baseline_root)
        sides = {"parent": Child(base), "control": Child(base), "candidate": Child(ROOT)}
        try:
            for name in names:
                rec = probe_line(sides, name, a.rounds)
                ok = ok and rec["within_margin"]
                emit(rec)
        finally:
            for side in sides.values():
                side.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
