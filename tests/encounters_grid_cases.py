"""The numpy model of the encounters on the cell list (nbody_get_encounters_grid, nbody_batch_get_encounters_grid;
include/nbody.h), the model and the check of their window rule, and the states, grids and horizons their tests
share.

The definition is the plain one on a subset: inside_of of the groups on the cell list (cell_cases.cell_index >= 0) picks the
bodies, encounter_cases.model_encounters runs on exactly those in their order, and the indices are mapped back to the state's.
Integers, and a list sorted by (t, i, j) whose t comes from the same fp64 operations whichever end evaluates the pair: the GPU
tests compare with zero tolerance.

The window rule (csrc/nbody_encounters_grid.hpp), all fp64, each operation rounded on its own, on the exactly widened record:
    rho = |R| + (h * (|VX| + |VY|));  +inf where that is NaN;  +inf in an fp64 state where any of X, Y, VX, VY, R is not finite
          or non-zero with a magnitude outside [2^-100, 2^200]
    H = (rho + rho) * (1 + 2^-40);  H2 = H * H
    row i owns (i, j)  <=>  rho_i > rho_j, or rho_i == rho_j and i > j
    row i looks at within_cases._span(t, H_i * sx, nx) x _span(t, H_i * sy, ny) and filters with d2 <= H2_i
reach restates the first two lines bit for bit, loop_encounters_grid walks every owner row's window as the device does, and
window_holds is the property the device relies on: a swept pair has d2 <= H2 of its owner and the other end's cell in the
owner's window."""
import collections
import functools

import numpy as np

import cell_cases as cc
import encounter_cases as ec
import groups_grid_cases as gg
import pairs_grid_cases as pg
import within_cases as wc

INFO_DTYPE = np.dtype(ec.INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])
INF = float("inf")
H = ec.H                                                        # the horizon of the standard state
BODY_COUNTS = pg.BODY_COUNTS                                    # (1, 2, 63, 64, 65, 255, 256, 257, 300, 385)
GRID_SHAPES = wc.GRID_SHAPES
DTYPES = wc.DTYPES
BATCH_COUNTS = (0, 1, 300, 385)
BATCH_CAP = 385
SPEED_SCALE = 4.0                                               # on encounter_cases.standard_state's velocities: at n = 65 the
#                                                                 stock +-40 gives 16 swept pairs at h = 0.5 and twice that 25,
#                                                                 fewer than the 33 the edge tests ask for; four times gives 35.
#                                                                 A power of two keeps the fp32 values exact
TIME_STEP = 0.2
HORIZONS = (0.0, TIME_STEP, 10 * TIME_STEP, INF)                # of the 300-body state
LO, HI = 2.0 ** -100, 2.0 ** 200                                # the fp64 guard's range


def inside_of(P, grid):
    return gg.inside_of(P, grid)


def _state(P, V, R):
    return (np.asarray(P, dtype=np.float64).reshape(-1, 2), np.asarray(V, dtype=np.float64).reshape(-1, 2),
            np.asarray(R, dtype=np.float64).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def reach(P, V, R, h, dtype):
    """(rho, H, H2) of every body, bit for bit what the device computes; dtype: the precision of the state the values were
    widened from (the guard is the fp64 context's only)."""
    P, V, R = _state(P, V, R)
    h = np.float64(h)
    with np.errstate(all="ignore"):
        rho = np.abs(R) + (h * (np.abs(V[:, 0]) + np.abs(V[:, 1])))
        rho = np.where(np.isnan(rho), np.inf, rho)
        if np.dtype(dtype) == np.float64:
            comp = np.abs(np.stack([P[:, 0], P[:, 1], V[:, 0], V[:, 1], R], axis=1))
            ok = ((comp == 0.0) | ((comp >= LO) & (comp <= HI))).all(axis=1)        # a NaN or an infinity is not
            rho = np.where(ok, rho, np.inf)
        Hh = (rho + rho) * (1.0 + 2.0 ** -40)
        return rho, Hh, Hh * Hh


def reach_loop(P, V, R, h, dtype):
    """reach as a scalar loop over Python floats."""
    P, V, R = _state(P, V, R)
    h = float(h)
    out = []
    for k in range(len(R)):
        x, y, vx, vy, r = (float(v) for v in (P[k, 0], P[k, 1], V[k, 0], V[k, 1], R[k]))
        t = abs(vx) + abs(vy)
        m = float("nan") if ((h == INF and t == 0.0) or (t == INF and h == 0.0)) else h * t      # Python has no quiet 0 * inf
        rho = abs(r) + m
        if rho != rho:
            rho = INF
        if np.dtype(dtype) == np.float64:
            for c in (x, y, vx, vy, r):
                a = abs(c)
                if not (a == 0.0 or (LO <= a <= HI)):
                    rho = INF
        Hh = (rho + rho) * (1.0 + 2.0 ** -40)
        try:
            H2 = Hh * Hh
        except OverflowError:
            H2 = INF
        out.append((rho, Hh, H2))
    return tuple(np.array([o[k] for o in out], dtype=np.float64) for k in range(3))


def owner(rho, i, j):
    """True where row i owns the pair (i, j); arrays broadcast."""
    ri, rj = rho[i], rho[j]
    return (ri > rj) | ((ri == rj) & (np.asarray(i) > np.asarray(j)))


def pair_terms(P, V, R, h, i, j):
    """The definition's values of the pair as row i evaluates source j (dx = X_j - X_i), vectorised over j -> a dict."""
    P, V, R = _state(P, V, R)
    h = np.float64(h)
    with np.errstate(all="ignore"):
        dx, dy = P[j, 0] - P[i, 0], P[j, 1] - P[i, 1]
        dvx, dvy = V[j, 0] - V[i, 0], V[j, 1] - V[i, 1]
        d2 = (dx * dx) + (dy * dy)
        s = R[i] + R[j]
        s2 = s * s
        c = d2 - s2
        b = (dx * dvx) + (dy * dvy)
        a = (dvx * dvx) + (dvy * dvy)
        disc = (b * b) - (a * c)
        ex, ey = dx + (dvx * h), dy + (dvy * h)
        e2 = (ex * ex) + (ey * ey)
        now, end = d2 <= s2, e2 <= s2
        mid = (b < 0.0) & ((-b) < (a * h)) & (disc >= 0.0)
    return {"d2": d2, "s2": s2, "e2": e2, "c": c, "b": b, "a": a, "ah": a * h if np.isfinite(h) else None, "disc": disc,
            "now": now, "end": end, "mid": mid, "swept": now | end | mid}


def _windows(P, grid, Hh):
    """The spans of every row's window -> (c0, c1, r0, r1, ix, iy, cell)."""
    x0, y0, sx, sy, nx, ny = cc.grid_tuple(grid)
    fine = not (sx <= 2.0 ** 400 and sy <= 2.0 ** 400)
    with np.errstate(over="ignore", invalid="ignore"):
        wx0, wy0 = (np.full(len(Hh), np.inf),) * 2 if fine else (Hh * sx, Hh * sy)
        tx, ty = (P[:, 0] - x0) * sx, (P[:, 1] - y0) * sy
    c0, c1 = wc._span(tx, wx0, nx)
    r0, r1 = wc._span(ty, wy0, ny)
    cell = cc.cell_index(P, grid)
    return c0, c1, r0, r1, cell % nx, cell // nx, cell


# ---------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------
def model_encounters_grid(P, V, R, grid, h):
    """encounter_cases.model_encounters on the inside bodies, the indices mapped back -> (list, info with n_bodies = n,
    "inside", "outside").  The inside bodies keep their order, so the list stays sorted by (t, i, j)."""
    P, V, R = _state(P, V, R)
    idx = np.flatnonzero(inside_of(P, grid))
    lst, info = ec.model_encounters(P[idx], V[idx], R[idx], h)
    lst = lst.copy()
    lst["i"], lst["j"] = idx[lst["i"]], idx[lst["j"]]
    info.update(n_bodies=len(P), inside=len(idx), outside=len(P) - len(idx))
    return lst, info


def loop_encounters_grid(P, V, R, grid, h, dtype):
    """The device's walk, literally: every inside row i walks the cells of its own window (within_cases._span with H_i), takes
    the members with d2 <= H2_i that are not itself, keeps the pairs it owns and applies the definition as IT sees the pair
    (dx = X_j - X_i, whichever of i and j is lower); the record is {lower, higher}.  -> (list, info), the seen pairs as they
    were found: a pair found twice stays twice."""
    P, V, R = _state(P, V, R)
    n = len(R)
    rho, Hh, H2 = reach(P, V, R, h, dtype)
    c0, c1, r0, r1, ix, iy, cell = _windows(P, grid, Hh)
    rows = []
    for i in np.flatnonzero(cell >= 0):
        cand = np.flatnonzero((cell >= 0) & (c0[i] <= ix) & (ix <= c1[i]) & (r0[i] <= iy) & (iy <= r1[i]))
        t = pair_terms(P, V, R, h, i, cand)
        with np.errstate(invalid="ignore"):
            keep = (t["d2"] <= H2[i]) & (cand != i)             # the hot compare
        keep &= owner(rho, np.full(len(cand), i), cand) & t["swept"]
        for k in np.flatnonzero(keep):
            j = int(cand[k])
            rows.append((min(i, j), max(i, j), int(t["now"][k]) * ec.NOW + int(t["end"][k]) * ec.END, t["c"][k], t["b"][k], t["disc"][k]))
    if rows:
        i, j, flags, c, b, disc = (np.array([r[k] for r in rows]) for k in range(6))
        flags = flags.astype(np.uint32)
    else:
        i = j = np.zeros(0, dtype=np.int64)
        flags = np.zeros(0, dtype=np.uint32)
        c = b = disc = np.zeros(0)
    lst = ec._sorted(ec._time(flags, c, b, disc, np.float64(h)), i, j, flags)
    info = ec._info(n, flags, h)
    k = int((cell >= 0).sum())
    info.update(inside=k, outside=n - k)
    return lst, info


def assert_same(got, want, what=""):
    ec.assert_same(got, want, what)
    if "inside" in got[1] and "inside" in want[1]:
        assert (got[1]["inside"], got[1]["outside"]) == (want[1]["inside"], want[1]["outside"]), what


def swept_pairs(P, V, R, grid, h):
    """(i, j) with i < j of every swept pair of inside bodies, as the definition computes it."""
    lst, _ = model_encounters_grid(P, V, R, grid, h)
    return lst["i"].astype(np.int64), lst["j"].astype(np.int64)


def window_holds(P, V, R, grid, h, dtype):
    """For every swept pair of inside bodies: exactly one end owns it, the owner's computed d2 <= H2_owner and the other
    end's cell lies in the owner's window -> the number of swept pairs."""
    P, V, R = _state(P, V, R)
    i, j = swept_pairs(P, V, R, grid, h)
    if len(i) == 0:
        return 0
    rho, Hh, H2 = reach(P, V, R, h, dtype)
    own_i, own_j = owner(rho, i, j), owner(rho, j, i)
    assert (own_i ^ own_j).all(), "a pair without exactly one owner"
    o, k = np.where(own_i, i, j), np.where(own_i, j, i)
    d2 = pair_terms(P, V, R, h, o, k)["d2"]
    bad = np.flatnonzero(~(d2 <= H2[o]))
    assert bad.size == 0, ("a swept pair beyond its owner's H2", o[bad[:4]], k[bad[:4]], d2[bad[:4]], H2[o[bad[:4]]])
    c0, c1, r0, r1, ix, iy, cell = _windows(P, grid, Hh)
    seen = (cell[k] >= 0) & (c0[o] <= ix[k]) & (ix[k] <= c1[o]) & (r0[o] <= iy[k]) & (iy[k] <= r1[o])
    bad = np.flatnonzero(~seen)
    assert bad.size == 0, ("a swept pair whose other end lies outside its owner's window", o[bad[:4]], k[bad[:4]])
    return len(i)


def owner_rules(P, V, R, grid, h, dtype):
    """Which rule gave every swept pair its owner -> a Counter over "index" (rho ties), "radius" (the owner's |R| is larger
    and its speed is not), "speed" (its |VX| + |VY| is larger and its |R| is not), "both" and "other"."""
    P, V, R = _state(P, V, R)
    i, j = swept_pairs(P, V, R, grid, h)
    rho = reach(P, V, R, h, dtype)[0]
    out = collections.Counter()
    a, sp = np.abs(R), np.abs(V[:, 0]) + np.abs(V[:, 1])
    for p, q in zip(i, j):
        o, k = (p, q) if owner(rho, p, q) else (q, p)
        if rho[o] == rho[k]:
            out["index"] += 1
        elif a[o] > a[k] and not sp[o] > sp[k]:
            out["radius"] += 1
        elif sp[o] > sp[k] and not a[o] > a[k]:
            out["speed"] += 1
        elif a[o] > a[k] and sp[o] > sp[k]:
            out["both"] += 1
        else:
            out["other"] += 1                                   # the guard, a NaN
    return out


def window_cells(P, V, R, grid, h, dtype):
    """The cells in every inside row's window -> int64 per inside row (the probe's "median and widest window")."""
    P, V, R = _state(P, V, R)
    c0, c1, r0, r1, ix, iy, cell = _windows(P, grid, reach(P, V, R, h, dtype)[1])
    m = cell >= 0
    return (np.maximum(c1 - c0 + 1, 0) * np.maximum(r1 - r0 + 1, 0))[m]


# ---------------------------------------------------------------------------------------------------------------------
# the shared states and grids
# ---------------------------------------------------------------------------------------------------------------------
half_of = pg.half_of
standard_grids = pg.standard_grids                              # 8 x 8 and 1 x 1 over the bounding square, and a partial grid


@functools.lru_cache(maxsize=None)
def standard(n, tag):
    """encounter_cases.standard_state(n, dtype) with the velocities times SPEED_SCALE -> (P, V, R), read-only."""
    P, V, R = ec.standard_state(n, DTYPES[tag])
    V = (V * SPEED_SCALE).astype(DTYPES[tag]).astype(np.float64)
    for a in (P, V, R):
        a.setflags(write=False)
    return P, V, R


class Case:
    """name; tag; P, V, R float64 (exact in the dtype of tag); h; asks = [(nx, ny, bounds), ...]; expect: the fields of the
    model's info that the case is built for (on the first ask); rule: the owner rule of its pair (0, 1), or None."""

    def __init__(self, name, tag, P, V, R, h, asks, expect, rule=None):
        dt = DTYPES[tag]
        self.name, self.tag, self.dtype, self.h, self.asks, self.expect, self.rule = name, tag, dt, float(h), asks, expect, rule
        with np.errstate(over="ignore"):
            self.P, self.V, self.R = (np.asarray(a, dtype=np.float64).astype(dt).astype(np.float64) for a in (P, V, R))
        self.P, self.V = self.P.reshape(-1, 2), self.V.reshape(-1, 2)
        for a in (self.P, self.V, self.R):
            a.setflags(write=False)

    @property
    def state(self):
        return self.P, self.V, self.R


FIELD = 64.0
SHAPE_ASKS = [(nx, ny, (0.0, FIELD, 0.0, FIELD)) for nx, ny in GRID_SHAPES]
BYSTANDERS = ([[5.0, 5.0], [60.0, 58.0], [33.0, 3.0]], [[0.0, 0.0], [1.0, -1.0], [0.0, 2.0]], [0.5, 0.25, 1.0])   # far from everything


def _with_bystanders(P, V, R):
    return np.concatenate([P, BYSTANDERS[0]]), np.concatenate([V, BYSTANDERS[1]]), np.concatenate([R, BYSTANDERS[2]])


@functools.lru_cache(maxsize=None)
def cases():
    """Every constructed case of the GPU tests, by name.  Shared, never written to.  Bodies 0 and 1 are the pair a case is
    about; three bystanders follow."""
    out = []

    def add(name, tag, P, V, R, h, expect, rule=None, asks=SHAPE_ASKS, bystanders=True):
        P, V, R = (np.asarray(a, dtype=np.float64) for a in (P, V, R))
        if bystanders:
            P, V, R = _with_bystanders(P, V, R)
        out.append(Case("%s-%s" % (name, tag), tag, P, V, R, h, asks, expect, rule))

    for tag in DTYPES:
        # a small fast body closing on a large slow one: the smaller radius owns the pair, touching at the end
        add("fast-small", tag, [[20, 32], [40, 32]], [[0, 0], [-40, 0]], [3, 0.25], 0.5, dict(pairs=1, now=0, end=1), "speed")
        # the reverse: a large body at rest, a small one drifting in; the larger radius owns
        add("slow-large", tag, [[20, 32], [24.5, 32]], [[0, 0], [-4, 0]], [3, 0.25], 0.5, dict(pairs=1, now=0, end=1), "radius")
        # head-on at equal speed and radius: rho ties, the higher index owns; e2 == s2 at the end
        add("head-on", tag, [[20, 32], [28, 32]], [[10, 0], [-10, 0]], [1, 1], 0.5, dict(pairs=1, now=0, end=1), "index")
        # a bullet that crosses ten cells of the 64 x 64 grid within h and passes a body at rest: overlap at neither end
        add("bullet", tag, [[10, 32.2], [15, 32]], [[20, 0], [0, 0]], [0.25, 0.25], 0.5, dict(pairs=1, now=0, end=0, missed=1), "speed")
        # e2 == s2 exactly: (ex, ey) = (3, 4), s = 5
        add("end-exact", tag, [[20, 30], [27, 34]], [[0, 0], [-8, 0]], [2.5, 2.5], 0.5, dict(pairs=1, now=0, end=1), "speed")
        # disc == 0 exactly: grazing at a perpendicular offset of s
        add("grazing", tag, [[20, 30], [26, 32]], [[0, 0], [-20, 0]], [1, 1], 0.5, dict(pairs=1, now=0, end=0, missed=1), "speed")
        # d2 as near H2 of the owner as a swept pair comes: |d| = rho_0 + rho_1 = 2 rho exactly, touching at the end
        add("at-reach", tag, [[20, 32], [32, 32]], [[10, 0], [-10, 0]], [1, 1], 0.5, dict(pairs=1, now=0, end=1), "index")
        # a large common velocity: windows as wide as the grid, and no swept pair
        add("bulk", tag, [[20, 32], [23, 32]], [[1000, 0], [1000, 0]], [1, 1], 0.5, dict(pairs=0), None, bystanders=False)
        # negative radii: s and s2 as the definition computes them, rho from |R|
        add("negative-radius", tag, [[20, 32], [21.5, 32], [20, 32.5]], [[0, 0], [0, 0], [0, 0]], [-1, 3, 0.25], 0.5,
            dict(pairs=3, now=3), "radius")
        # a NaN velocity on a body that overlaps another: `now` does not read it, t = +0
        add("nan-velocity", tag, [[20, 32], [21, 32]], [[np.nan, 0], [0, 0]], [1, 1], 0.5, dict(pairs=1, now=1, end=0), None)
        # a NaN coordinate: outside the grid, in no pair
        add("nan-coordinate", tag, [[np.nan, 32], [21, 32], [22, 32]], [[0, 0], [0, 0], [0, 0]], [1, 1, 1], 0.5,
            dict(pairs=1, now=1, outside=1), None)
        # an infinite radius: s2 = +inf, every pair with it overlaps now and at the end
        add("infinite-radius", tag, [[20, 32], [40, 40]], [[1, 0], [0, 1]], [np.inf, 1], 0.5, dict(pairs=4, now=4, end=4), None)
        # a body outside the grid that overlaps one inside
        add("outside", tag, [[63.5, 32], [64.5, 32]], [[0, 0], [0, 0]], [1, 1], 0.5, dict(pairs=0, outside=1), None)
        # the horizons on the pair of fast-small: 0, tiny, +inf
        add("h-zero", tag, [[20, 32], [22, 32]], [[0, 0], [-40, 0]], [3, 0.25], 0.0, dict(pairs=1, now=1, end=1), "radius")
        add("h-tiny", tag, [[20, 32], [22, 32]], [[0, 0], [-40, 0]], [3, 0.25], 1e-300, dict(pairs=1, now=1, end=1), "radius")
        add("h-inf", tag, [[20, 32], [40, 32]], [[0, 0], [-40, 0]], [3, 0.25], INF, dict(pairs=1, now=0, end=0, missed=1), "index")
    # fp64 only: a component of 1e-40 is outside the guard's range - the body's window is the whole grid
    add("guard", "f64", [[1e-40, 32], [40, 32]], [[0, 0], [-40, 0]], [3, 0.25], 0.5, dict(pairs=0), None)
    add("guard-hit", "f64", [[20, 32], [22, 32]], [[0, 1e-40], [0, 0]], [3, 0.25], 0.5, dict(pairs=1, now=1), None)
    return {c.name: c for c in out}


def case_names(prefix=""):
    return [k for k in cases() if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def horizon_state(tag):
    """The 300-body standard state, asked at HORIZONS."""
    return standard(300, tag)


def batch_states():
    """Four systems - none, one body, 300 and 385 - of the standard states (fp32: a batch is)."""
    return [tuple(a[:n] for a in standard(max(n, 1), "f32")) for n in BATCH_COUNTS]


batch_grids = pg.batch_grids                                    # one grid that holds every body of the four systems, one that does not
