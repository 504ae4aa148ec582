"""The numpy model of the radius queries (nbody_get_within, nbody_batch_get_within; include/nbody.h), the model
of their window rule, and the states, grids and radii their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance.  The sources are the bodies inside the
grid (cell_cases.cell_index).  A row at (x, y) with radius r (+0 for a probe point), own index i (none for a point):
    dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)
    near(j)  <=>  inside(j) && j != i && d2_j <= h2
    count = #near;  (d2, index) = the lexicographic minimum of (d2_j, j) over the near j, (+inf, -1) where none is below +inf
    overlaps = #near with d2_j <= s*s, s = r + R_j;  cell = the row's own cell, -1 outside
    start = the exclusive prefix sum of count;  list = the near j of every row, ascending
model_within is brute force over all sources; loop_within is the definition as a scalar loop that visits the sources in
DESCENDING j, so that the tie rule and the sorted list are what make the two agree; window_model restates the rule by which
the device picks the cells a row looks at (cells_span of csrc/nbody_cells.hpp, within_window of csrc/nbody_within.hpp) and
returns the sources in those cells: test_within_cases_cpu.py holds that they include every near source, for every case below."""
import functools

import numpy as np

import cell_cases as cc
import neighbor_cases as nc

DTYPE = np.dtype([("d2", np.float64), ("index", np.int32), ("count", np.int32), ("overlaps", np.int32), ("cell", np.int32)])
INFO_FIELDS = ("total", "n", "rows", "inside", "outside", "largest", "largest_row")
ROW_FIELDS = ("index", "count", "overlaps", "cell")


def _rows_of(P, R, points, rows=None):
    if points is None:
        rows = np.arange(len(R)) if rows is None else np.asarray(rows, dtype=np.int64)
        return P[rows, 0], P[rows, 1], R[rows], rows
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return points[:, 0], points[:, 1], np.zeros(len(points)), None


def _info(out, n, inside):
    count = out["count"].astype(np.int64)
    largest = int(count.max()) if len(count) else 0
    return {"total": int(count.sum()), "n": n, "rows": len(count), "inside": inside, "outside": n - inside, "largest": largest,
            "largest_row": int(np.argmax(count)) if len(count) else 0}      # argmax: the lowest row that has it


def model_within(P, R, grid, h2, points=None, chunk=128, rows=None):
    """The definition over the bodies P (n, 2), R (n,), float64 (an fp32 state widened exactly), at the bodies or at explicit
    `points` (m, 2) -> what Stepper.within(lists=True) returns: {"rows": DTYPE (rows,), "info", "start": int64 (rows + 1,),
    "list": int32 (total,)}.  rows: only these bodies as rows (a sample of a large state); info, start and list are then
    the sample's."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    h2 = np.float64(h2)
    n = len(R)
    X, Y = P[:, 0], P[:, 1]
    inside = cc.cell_index(P, grid) >= 0
    px, py, pr, me = _rows_of(P, R, points, rows)
    k = len(px)
    out = np.zeros(k, dtype=DTYPE)
    out["d2"], out["index"] = np.inf, -1
    out["cell"] = cc.cell_index(np.stack([px, py], axis=1), grid) if k else 0
    lists = []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, k if n else 0, chunk):
            sl = slice(a, min(a + chunk, k))
            dx = X[None, :] - px[sl, None]
            dy = Y[None, :] - py[sl, None]
            d2 = (dx * dx) + (dy * dy)
            near = inside[None, :] & (d2 <= h2)                 # a NaN d2 is never near
            if me is not None:
                near[np.arange(sl.stop - sl.start), me[sl]] = False
            s = pr[sl, None] + R[None, :]
            cand = np.where(near, d2, np.inf)
            j = np.argmin(cand, axis=1)                         # the first minimum: ties go to the lowest j
            best = cand[np.arange(len(j)), j]
            out["d2"][sl] = best
            out["index"][sl] = np.where(best < np.inf, j, -1)
            out["count"][sl] = near.sum(axis=1)
            out["overlaps"][sl] = (near & (d2 <= s * s)).sum(axis=1)
            lists.append(np.nonzero(near)[1])                   # row-major: ascending j inside a row
    start = np.zeros(k + 1, dtype=np.int64)
    start[1:] = np.cumsum(out["count"].astype(np.int64))
    lst = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, dtype=np.int32)
    return {"rows": out, "info": _info(out, n, int(inside.sum())), "start": start, "list": lst}


def loop_within(P, R, grid, h2, points=None):
    """The definition as a plain scalar loop over Python floats, the sources visited in DESCENDING j."""
    x0, y0, sx, sy, nx, ny = (float(v) if q < 4 else int(v) for q, v in enumerate(cc.grid_tuple(grid)))
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    n, h2 = len(R), float(h2)
    X, Y, Rr = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]], [float(v) for v in R]

    def cell(x, y):
        tx, ty = (x - x0) * sx, (y - y0) * sy
        return int(ty) * nx + int(tx) if (0.0 <= tx and tx < nx and 0.0 <= ty and ty < ny) else -1
    if points is None:
        todo = [(X[i], Y[i], Rr[i], i) for i in range(n)]
    else:
        todo = [(float(q[0]), float(q[1]), 0.0, -1) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    inside = [cell(X[j], Y[j]) >= 0 for j in range(n)]
    out = np.zeros(len(todo), dtype=DTYPE)
    start, lst = [0], []
    for k, (x, y, r, i) in enumerate(todo):
        best, index, count, overlaps, mine = float("inf"), -1, 0, 0, []
        for j in reversed(range(n)):
            if not inside[j] or j == i:
                continue
            dx = X[j] - x
            dy = Y[j] - y
            try:
                d2 = (dx * dx) + (dy * dy)
            except OverflowError:                                # Python raises where IEEE gives +inf
                d2 = float("inf")
            if not d2 <= h2:
                continue
            count += 1
            mine.append(j)
            if d2 < best or (d2 == best and j < index):
                best, index = d2, j
            s = r + Rr[j]
            if d2 <= s * s:
                overlaps += 1
        out[k] = (best, index, count, overlaps, cell(x, y))
        lst += sorted(mine)
        start.append(start[-1] + count)
    return {"rows": out, "info": _info(out, n, sum(inside)), "start": np.asarray(start, dtype=np.int64),
            "list": np.asarray(lst, dtype=np.int32)}


def _span(t, w0, cells):
    """cells_span: the window along one axis -> (lo, hi) int64 per row; hi < lo: none."""
    with np.errstate(over="ignore", invalid="ignore"):
        w = w0 + (2.0 ** -20 + (np.abs(t) + w0) * 2.0 ** -40)
        lo, hi = t - w, t + w
        whole = ~(np.abs(t) < np.inf) | np.isnan(lo) | np.isnan(hi)
        none = ~whole & ((hi < 0.0) | (lo >= np.float64(cells)))
    take = ~whole & ~none                                        # converted only after the compares
    a = np.where(take & (lo > 0.0), lo, 0.0).astype(np.int64)
    b = np.where(take & (hi < np.float64(cells - 1)), hi, np.float64(cells - 1)).astype(np.int64)
    return np.where(none, 0, a), np.where(none, -1, b)


def window_model(P, grid, h2, rows_xy):
    """The window rule restated: for the rows at rows_xy (k, 2) the sources of P the device looks at -> bool (k, n): source j
    is inside the grid and its cell lies in the row's window."""
    x0, y0, sx, sy, nx, ny = cc.grid_tuple(grid)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    rows_xy = np.asarray(rows_xy, dtype=np.float64).reshape(-1, 2)
    h = np.sqrt(np.float64(h2))
    fine = not (sx <= 2.0 ** 400 and sy <= 2.0 ** 400)
    with np.errstate(over="ignore", invalid="ignore"):
        wx0, wy0 = (np.inf, np.inf) if fine else (h * sx, h * sy)
        tx, ty = (rows_xy[:, 0] - x0) * sx, (rows_xy[:, 1] - y0) * sy
    c0, c1 = _span(tx, wx0, nx)
    r0, r1 = _span(ty, wy0, ny)
    cell = cc.cell_index(P, grid)
    ix, iy = cell % nx, cell // nx
    return ((cell >= 0)[None, :] & (c0[:, None] <= ix[None, :]) & (ix[None, :] <= c1[:, None])
            & (r0[:, None] <= iy[None, :]) & (iy[None, :] <= r1[:, None]))


def info_dict(info):
    return {k: int(info[k]) for k in INFO_FIELDS}


def assert_same(got, want, what="", lists=True, cell=True):
    """Zero tolerance: integers exactly, d2 by its bits.  cell=False leaves the rows' own cells out (two different grids)."""
    g, w = np.asarray(got["rows"]), np.asarray(want["rows"])
    assert g.dtype == DTYPE and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    bad = cc.bits(g["d2"]) != cc.bits(w["d2"])
    for f in ROW_FIELDS if cell else ROW_FIELDS[:-1]:
        bad |= g[f] != w[f]
    bad = np.flatnonzero(bad)
    assert bad.size == 0, (what, "%d rows differ, first %d" % (bad.size, bad[0]), g[bad[:4]], w[bad[:4]])
    assert info_dict(got["info"]) == info_dict(want["info"]), (what, info_dict(got["info"]), info_dict(want["info"]))
    if lists:
        for f, dt in (("start", np.int64), ("list", np.int32)):
            a, b = np.asarray(got[f]), np.asarray(want[f])
            assert a.dtype == dt and a.shape == b.shape, (what, f, a.dtype, a.shape, b.shape)
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, (what, "%d entries of %s differ, first at %d" % (bad.size, f, bad[0]), a[bad[0]], b[bad[0]])


def lists_consistent(res):
    """start is the prefix sum of count, start[rows] is info.total, every row's segment is strictly ascending."""
    rows, start, lst = res["rows"], res["start"], res["list"]
    assert start[0] == 0 and np.array_equal(np.diff(start), rows["count"])
    assert start[-1] == info_dict(res["info"])["total"] == len(lst)
    for k in range(len(rows)):
        seg = lst[start[k]:start[k + 1]]
        assert (np.diff(seg) > 0).all(), k
    return True


# ---------------------------------------------------------------------------------------------------------------------
# the shared cases: a state, and the (nx, ny, bounds, h2) it is asked on
# ---------------------------------------------------------------------------------------------------------------------
BODY_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 300, 385)
GRID_SHAPES = ((1, 7), (7, 1), (3, 3), (64, 64), (257, 3))
DTYPES = {"f32": np.float32, "f64": np.float64}
STATE_SEED = 6121
LATTICE_SIDE = 17                                               # 289 bodies: two workgroups


class Case:
    """name; dtype; P (n, 2) and R (n,) float64, exact in dtype; asks = [(nx, ny, bounds, h2), ...]; points or None."""

    def __init__(self, name, dtype, P, R, asks, points=None):
        self.name, self.dtype, self.P, self.R, self.asks, self.points = name, dtype, P, R, asks, points
        for a in (P, R) + (() if points is None else (points,)):
            a.setflags(write=False)

    def grid(self, ask):
        return cc.grid_of(*ask[:3])

    def rows_xy(self):
        return self.P if self.points is None else self.points


def state(n, dtype, coincident=False):
    """n bodies uniform over tenth_field(n) with radii up to 1.5 -> (P, R, field); coincident: body 7 sits on body n - 100."""
    f = cc.tenth_field(n)
    P, R = nc.random_state(n, dtype, STATE_SEED + n, field=f)
    if coincident:
        P[7] = P[n - 100]
    return P, R, f


def one_cell_state(n, dtype):
    """n bodies inside cell (2, 2) of the 8 x 8 grid over [0, 8)^2."""
    P, R = nc.random_state(n, dtype, STATE_SEED, field=1.0, radius=0.02)
    return (P * 0.5 + 2.25).astype(dtype).astype(np.float64), R


def awkward_points(P, f):
    """neighbor_cases.probe_points - on bodies, inside, far outside, 1e6 fields away - plus a NaN point and a 1e200 point."""
    pts = nc.probe_points(P, 130, 17, f)
    return np.concatenate([pts, [[np.nan, 0.5 * f], [0.5 * f, -1e200], [1e200, 1e200]]])


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the GPU tests, by name.  Shared, never written to."""
    out = []
    for tag, dtype in DTYPES.items():
        for n in BODY_COUNTS:                                   # workgroup and wave edges; h = one cell of the 8 x 8 grid
            P, R, f = state(n, dtype)
            h2 = (f / 8) ** 2
            out.append(Case("bodies-%d-%s" % (n, tag), dtype, P, R,
                            [(8, 8, (0, f, 0, f), h2), (1, 1, (0, f, 0, f), h2), (8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f), h2)]))
        P, R, f = state(300, dtype, coincident=True)
        out.append(Case("shapes-%s" % tag, dtype, P, R, [(nx, ny, (0, f, 0, f), (0.1 * f) ** 2) for nx, ny in GRID_SHAPES]))
        c = f / 16                                              # radii on 16 x 16 cells: 0.3, 3.5 cells, beyond the field, inf
        out.append(Case("radii-%s" % tag, dtype, P, R,
                        [(16, 16, (0, f, 0, f), h2) for h2 in (0.0, (0.3 * c) ** 2, (3.5 * c) ** 2, (2 * f) ** 2, np.inf)]))
        L, LR = nc.lattice(LATTICE_SIDE)                        # spacing = cell side = h = 1: d2 == h2 pairs, bodies on the cell
        s = float(LATTICE_SIDE)                                 # boundaries (offset 0) and a tenth of a cell off them
        out.append(Case("lattice-%s" % tag, dtype, L, LR,
                        [(LATTICE_SIDE, LATTICE_SIDE, (-o, s - o, -o, s - o), 1.0) for o in (0.0, 0.1)]))
        Q, QR = one_cell_state(385, dtype)
        out.append(Case("one-cell-%s" % tag, dtype, Q, QR, [(8, 8, (0, 8, 0, 8), 0.1 ** 2), (8, 8, (0, 8, 0, 8), np.inf)]))
        out.append(Case("points-%s" % tag, dtype, P, R,
                        [(16, 16, (0, f, 0, f), (1.5 * c) ** 2), (8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f), (0.2 * f) ** 2),
                         (4, 4, (0, f, 0, f), np.inf)], awkward_points(P, f)))
    return {c.name: c for c in out}


def case_names(prefix=""):
    return [k for k in cases() if k.startswith(prefix)]


# ---------------------------------------------------------------------------------------------------------------------
# the row scan past one block and past one trip of the block scan.  The device takes the exclusive prefix of the counts in
# blocks of SCAN_BLOCK_ROWS rows (a workgroup each), then one workgroup scans the block sums SCAN_TRIP_BLOCKS at a time.
# Every case: the 8 x 8 grid over its field, h = one cell side.  Each reference is computed once (scan_reference) and must
# stay inside the suite's CPU budget (large_cases.BUDGET_S; test_within_cases_cpu.py holds it).
# ---------------------------------------------------------------------------------------------------------------------
SCAN_BLOCK_ROWS = 1024
SCAN_TRIP_BLOCKS = 256
SCAN_BODIES = (("f32", 1023), ("f32", 1024), ("f32", 1025), ("f32", 2049), ("f64", 1025))   # rows around one and two blocks
SCAN_BATCH = (1025, 3)                                          # stride 1025: the second system's block 1 leaves at once
SCAN_POINTS = SCAN_TRIP_BLOCKS * SCAN_BLOCK_ROWS + 1025         # 258 blocks: a second trip of one full and one partial block
SCAN_POINT_BODIES = 65
SCAN_TIMES = {}                                                 # name -> seconds its reference took


def _scan_ask(f):
    return (8, 8, (0, f, 0, f), (f / 8) ** 2)


@functools.lru_cache(maxsize=None)
def scan_cases():
    """The cases of the row scan, by name; "scan-batch-k-f32" are the systems of the one batch, all on system 0's grid."""
    out = []
    for tag, n in SCAN_BODIES:
        P, R, f = state(n, DTYPES[tag])
        out.append(Case("scan-bodies-%d-%s" % (n, tag), DTYPES[tag], P, R, [_scan_ask(f)]))
    f0 = cc.tenth_field(SCAN_BATCH[0])
    for k, n in enumerate(SCAN_BATCH):
        P, R, _ = state(n, np.float32)
        out.append(Case("scan-batch-%d-f32" % k, np.float32, P, R, [_scan_ask(f0)]))
    P, R, f = state(SCAN_POINT_BODIES, np.float32)
    pts = np.random.default_rng(STATE_SEED).uniform(-0.05 * f, 1.05 * f, size=(SCAN_POINTS, 2))   # a few outside the grid
    out.append(Case("scan-points-f32", np.float32, P, R, [_scan_ask(f)], pts))
    return {c.name: c for c in out}


def scan_case_names(prefix="scan-"):
    return [k for k in scan_cases() if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def scan_reference(name):
    """model_within of the case's one ask, computed once, read-only."""
    import time
    case = scan_cases()[name]
    t0 = time.perf_counter()
    ref = model_within(case.P, case.R, case.grid(case.asks[0]), case.asks[0][3], case.points)
    SCAN_TIMES[name] = time.perf_counter() - t0
    for k in ("rows", "start", "list"):
        ref[k].setflags(write=False)
    return ref


def scan_sample(m):
    """64 rows of m: the first, the last, the rows either side of multiples of SCAN_BLOCK_ROWS - the first two, the last, and
    those around every multiple of SCAN_TRIP_BLOCKS * SCAN_BLOCK_ROWS - and rows evenly spread between."""
    blocks = (m - 1) // SCAN_BLOCK_ROWS
    edges = {1, 2, blocks} | set(range(SCAN_TRIP_BLOCKS - 1, blocks + 1, SCAN_TRIP_BLOCKS)) | set(range(SCAN_TRIP_BLOCKS, blocks + 1, SCAN_TRIP_BLOCKS))
    rows = {0, m - 1}
    for b in sorted(e for e in edges if 0 < e * SCAN_BLOCK_ROWS < m):
        rows |= {b * SCAN_BLOCK_ROWS - 1, b * SCAN_BLOCK_ROWS}
    for r in np.linspace(0, m - 1, 200).astype(np.int64):
        if len(rows) < 64:
            rows.add(int(r))
    return np.array(sorted(rows), dtype=np.int64)
