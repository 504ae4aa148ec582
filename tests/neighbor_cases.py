"""The numpy model of the neighbour queries (nbody_get_neighbors, nbody_batch_get_neighbors; include/nbody.h)
and the states their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance.  A row at (x, y) with radius r (+0 for
a probe point, the body's own for a body), a source j at (X_j, Y_j) with radius R_j:
    dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)
    nearest : best = +inf, index = -1;  for j ascending:  if (d2_j < best) { best = d2_j; index = j; }
    overlaps: the number of j with  d2_j <= s*s,  s = r + R_j
with body i's own term left out by index when the rows are the bodies.

What `overlaps` does with awkward values follows from the two comparisons: a NaN d2 (a NaN coordinate, inf - inf) is never
an overlap; a +inf d2 (a coordinate of 1e200 squared) is an overlap exactly where s*s is +inf too - with finite radii below
1e154 never; a NaN radius makes s*s NaN, never an overlap, and plays no part in the nearest.

exact_check ties the model to the real squared distances with fractions.Fraction: u = 2^-53, dx within 1 u, its square within
3 u, the sum within 4 u (first order, no underflow), so a computed d2 is within 4 u of its exact value and the source the
model picks is within (1 + 8 u) of the true minimum (two computed values, each within 4 u)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
DTYPE = np.dtype([("d2", np.float64), ("index", np.int32), ("overlaps", np.int32)])
EMPTY = (np.inf, -1, 0)                                         # a row with no eligible source


def model_neighbors(P, R, rows=None, points=None, chunk=128):
    """The definition over the sources P (n, 2), R (n,), float64 (an fp32 state widened exactly): at the bodies `rows` (all
    of them by default; the self term left out) or at explicit `points` (k, 2) -> a DTYPE array of k records."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    n = len(R)
    X, Y = P[:, 0], P[:, 1]
    if points is None:
        rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        px, py, pr = X[rows], Y[rows], R[rows]
    else:
        assert rows is None
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py, pr = points[:, 0], points[:, 1], np.zeros(len(points))
    k = len(px)
    out = np.empty(k, dtype=DTYPE)
    out["d2"], out["index"], out["overlaps"] = EMPTY
    if n == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, k, chunk):
            sl = slice(a, min(a + chunk, k))
            dx = X[None, :] - px[sl, None]
            dy = Y[None, :] - py[sl, None]
            d2 = (dx * dx) + (dy * dy)
            s = pr[sl, None] + R[None, :]
            hit = d2 <= s * s
            cand = np.where(np.isnan(d2), np.inf, d2)           # a NaN is never below `best`
            if rows is not None:
                me = (np.arange(sl.stop - sl.start), rows[sl])
                hit[me] = False
                cand[me] = np.inf
            j = np.argmin(cand, axis=1)                         # the first minimum: ties go to the lowest j
            best = cand[np.arange(len(j)), j]
            out["d2"][sl] = best
            out["index"][sl] = np.where(best < np.inf, j, -1)
            out["overlaps"][sl] = hit.sum(axis=1)
    return out


def loop_neighbors(P, R, rows=None, points=None):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation)."""
    n = len(R)
    X, Y, Rr = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]], [float(v) for v in R]
    if points is None:
        rows = range(n) if rows is None else [int(i) for i in rows]
        todo = [(X[i], Y[i], Rr[i], i) for i in rows]
    else:
        todo = [(float(q[0]), float(q[1]), 0.0, -1) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    out = np.empty(len(todo), dtype=DTYPE)
    for k, (x, y, r, i) in enumerate(todo):
        best, index, overlaps = float("inf"), -1, 0
        for j in range(n):
            if j == i:
                continue
            dx = X[j] - x
            dy = Y[j] - y
            try:
                d2 = (dx * dx) + (dy * dy)
            except OverflowError:                                # Python raises where IEEE gives +inf
                d2 = float("inf")
            if d2 < best:
                best, index = d2, j
            s = r + Rr[j]
            if d2 <= s * s:
                overlaps += 1
        out[k] = (best, index, overlaps)
    return out


def same(a, b):
    """Zero tolerance: d2 by bits, index and overlaps exactly."""
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape == b.shape and np.array_equal(np.ascontiguousarray(a["d2"]).view(np.uint64),
                                                  np.ascontiguousarray(b["d2"]).view(np.uint64))
            and np.array_equal(a["index"], b["index"]) and np.array_equal(a["overlaps"], b["overlaps"]))


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((np.ascontiguousarray(got["d2"]).view(np.uint64) != np.ascontiguousarray(want["d2"]).view(np.uint64)).ravel()
                         | (got["index"] != want["index"]).ravel() | (got["overlaps"] != want["overlaps"]).ravel())
    assert bad.size == 0, (what, "%d rows differ, first %d" % (bad.size, bad[0]), got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def exact_check(P, R, res, rows=None, points=None, sample=None):
    """A handful of rows of a model (or device) result against exact rational arithmetic; finite inputs only."""
    P = np.asarray(P, dtype=np.float64)
    n = len(R)
    k = len(res)
    sample = range(k) if sample is None else sample
    FX, FY = [Fraction(float(v)) for v in P[:, 0]], [Fraction(float(v)) for v in P[:, 1]]
    u = Fraction(1, 2 ** 53)
    for q in sample:
        if points is None:
            i = int(q if rows is None else rows[q])
            x, y = FX[i], FY[i]
        else:
            i = -1
            x, y = Fraction(float(points[q][0])), Fraction(float(points[q][1]))
        exact = [None if j == i else (FX[j] - x) ** 2 + (FY[j] - y) ** 2 for j in range(n)]
        live = [e for e in exact if e is not None]
        if not live:
            assert tuple(res[q])[:2] == EMPTY[:2], q
            continue
        true_min = min(live)
        idx = int(res["index"][q])
        assert 0 <= idx < n and idx != i, (q, idx)
        assert exact[idx] <= true_min * (1 + 8 * u), (q, idx, float(exact[idx]), float(true_min))
        assert abs(Fraction(float(res["d2"][q])) - exact[idx]) <= 4 * u * exact[idx], (q, float(res["d2"][q]), float(exact[idx]))


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
def widen(b):
    """A BodiesData (or a download) -> (P, R) float64, exact."""
    return np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Radii, dtype=np.float64)


def random_state(n, dtype, seed, field=100.0, radius=1.5):
    """n bodies uniform over a field x field square with radii up to `radius`, rounded to dtype, as float64."""
    rng = np.random.default_rng(seed)
    P = (rng.uniform(0, field, size=(n, 2))).astype(dtype).astype(np.float64)
    R = (rng.uniform(0, radius, size=n)).astype(dtype).astype(np.float64)
    return P, R


def lattice(side=8, radius=0.25):
    """side x side integer lattice, row-major: an interior body has four nearest neighbours at d2 = 1 - below, left, right,
    above, in ascending index - and the lowest index (the one below, i - side) wins."""
    g = np.arange(side, dtype=np.float64)
    P = np.stack([np.tile(g, side), np.repeat(g, side)], axis=1)
    return P, np.full(side * side, radius)


def lattice_expected(side=8):
    """index of the nearest body for every lattice body, from the tie rule alone."""
    idx = np.empty(side * side, dtype=np.int32)
    for i in range(side * side):
        row, col = divmod(i, side)
        cands = [j for j, ok in ((i - side, row > 0), (i - 1, col > 0), (i + 1, col < side - 1), (i + side, row < side - 1)) if ok]
        idx[i] = min(cands)
    return idx


def probe_points(P, m, seed, field):
    """m points: uniform over the field; where there is room the first ones ON bodies (every 7th body), the last two far
    outside the field, and points 1 and m-2 the same point."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, field, size=(m, 2))
    k = min(len(P), m // 4)
    if k:
        pts[:k] = P[(np.arange(k) * 7) % len(P)]
    if m >= 8:
        pts[-1] = [-7.5 * field, 11.25 * field]
        pts[-3] = [1e6 * field, -3e5 * field]
        pts[-2] = pts[1]
    return pts
