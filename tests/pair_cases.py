"""The numpy model of the pair-separation counts (nbody_get_pair_counts, nbody_batch_get_pair_counts; include/nbody.h,
DESIGN.md 4.11) and the states their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit; the results are integers, so the GPU tests compare with zero tolerance whatever
order the device adds in.  A row at (x, y), a source j at (X_j, Y_j), an fp32 state widened exactly:
    dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)
    counts[k] = the number of counted pairs with  e2[k] <= d2 && d2 < e2[k+1]      k = 0 .. B-1
    below     = the number with  d2 < e2[0]
    rest      = pairs - below - sum(counts)          every counted pair with d2 >= e2[B], or NaN
Own form: the unordered pairs i < j of the bodies, pairs = n (n - 1) / 2 (d2_ij and d2_ji have the same bits).  Points
form: every (point, body) pair, pairs = m n, no self exclusion.

A NaN d2 fails every comparison and a +inf d2 fails `d2 < +inf`: both are in rest, whatever the edges."""
import numpy as np

from neighbor_cases import lattice, random_state, widen  # noqa: F401  (the states the models share)

INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("rows", np.int64), ("pairs", np.int64), ("below", np.int64), ("rest", np.int64)])
FIELDS = ("below", "rest", "pairs", "n_bodies")
CHUNK_BYTES = 32 << 20                                          # of one n-wide float64 temporary of the model


def _result(counts, below, pairs, n, e2):
    counts = np.asarray(counts, dtype=np.uint64)
    return {"counts": counts, "below": int(below), "rest": int(pairs) - int(below) - int(counts.sum()), "pairs": int(pairs),
            "n_bodies": int(n), "edges2": e2}


def model_pair_counts(P, edges2, points=None):
    """The definition over the bodies P (n, 2), float64 (an fp32 state widened exactly) and the B + 1 squared edges: the
    unordered pairs of bodies, or with `points` (m, 2) every (point, body) pair -> {"counts": uint64 (B,), "below", "rest",
    "pairs", "n_bodies", "edges2"}."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    e2 = np.asarray(edges2, dtype=np.float64).reshape(-1)
    B, n = len(e2) - 1, len(P)
    X, Y = P[:, 0], P[:, 1]
    own = points is None
    if own:
        px, py = X, Y
        pairs = n * (n - 1) // 2
    else:
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py = points[:, 0], points[:, 1]
        pairs = len(px) * n
    counts = np.zeros(B, dtype=np.int64)
    below = 0
    chunk = max(1, CHUNK_BYTES // (8 * max(n, 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(px) if n else 0, chunk):
            b = min(a + chunk, len(px))
            dx = X[None, :] - px[a:b, None]                     # [row, j] = X_j - x
            dy = Y[None, :] - py[a:b, None]
            d2 = (dx * dx) + (dy * dy)
            if own:                                             # row i with the sources j > i: each unordered pair once
                d2 = d2[np.triu(np.ones((b - a, n), dtype=bool), 1 + a)]
            else:
                d2 = d2.ravel()
            below += int((d2 < e2[0]).sum())
            for k in range(B):
                counts[k] += int(((e2[k] <= d2) & (d2 < e2[k + 1])).sum())
    return _result(counts, below, pairs, n, e2)


def loop_pair_counts(P, edges2, points=None):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    e2 = [float(v) for v in np.asarray(edges2, dtype=np.float64).reshape(-1)]
    B, n = len(e2) - 1, len(P)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    if points is None:
        todo = [(X[i], Y[i], i + 1) for i in range(n)]          # row i with the sources j > i
    else:
        todo = [(float(q[0]), float(q[1]), 0) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    counts, below, pairs = [0] * B, 0, 0
    for x, y, start in todo:
        for j in range(start, n):
            pairs += 1
            dx = X[j] - x
            dy = Y[j] - y
            try:
                d2 = (dx * dx) + (dy * dy)
            except OverflowError:                                # Python raises where IEEE gives +inf
                d2 = float("inf")
            if d2 < e2[0]:
                below += 1
            for k in range(B):
                if e2[k] <= d2 and d2 < e2[k + 1]:
                    counts[k] += 1
    return _result(counts, below, pairs, n, np.asarray(e2, dtype=np.float64))


def window_pair_counts(P, edges2):
    """model_pair_counts, own form, for states too large for an n x n matrix (finite values and a finite top edge): the
    bodies sorted by x, and body a paired with its k-th successor for k = 1, 2, ... as long as any successor lies within
    sqrt(top) (1 + 2^-40) in x.  Every candidate pair goes through the definition's own float64 arithmetic (the same bits:
    dx only changes sign with the order of the pair); a pair left out has dx*dx >= top after rounding, so d2 >= top: it is
    in rest, which is derived."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    e2 = np.asarray(edges2, dtype=np.float64).reshape(-1)
    B, n = len(e2) - 1, len(P)
    assert np.isfinite(P).all() and np.isfinite(e2[-1])
    counts = np.zeros(B, dtype=np.int64)
    below = 0
    order = np.argsort(P[:, 0], kind="stable")
    X, Y = P[order, 0], P[order, 1]
    reach = np.sqrt(e2[-1]) * (1 + 2.0 ** -40)
    for k in range(1, n):
        dx = X[k:] - X[:-k]
        near = dx <= reach
        if not near.any():
            break
        a = np.flatnonzero(near)
        dxa = dx[a]
        dy = Y[a + k] - Y[a]
        d2 = (dxa * dxa) + (dy * dy)
        d2 = d2[d2 < e2[-1]]
        below += int((d2 < e2[0]).sum())
        for b in range(B):
            counts[b] += int(((e2[b] <= d2) & (d2 < e2[b + 1])).sum())
    return _result(counts, below, n * (n - 1) // 2, n, e2)


def assert_same(got, want, what=""):
    """Zero tolerance on every field; the squared edges by bits."""
    g, w = np.asarray(got["counts"]), np.asarray(want["counts"])
    assert g.dtype == np.uint64 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, "%d bins differ, first at %d" % (bad.size, bad[0]), g[bad[:4]], w[bad[:4]])
    for f in FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    ge, we = (np.ascontiguousarray(r["edges2"], dtype=np.float64).view(np.uint64) for r in (got, want))
    assert np.array_equal(ge, we), (what, "edges2")


def check_sum(res, pairs, what=""):
    """below + sum(counts) + rest == pairs, with the pairs the caller expects."""
    assert res["pairs"] == pairs, (what, res["pairs"], pairs)
    assert res["below"] >= 0 and res["rest"] >= 0, (what, res["below"], res["rest"])
    assert res["below"] + int(res["counts"].sum()) + res["rest"] == pairs, what
