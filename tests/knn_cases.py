"""The numpy model of the k-nearest-neighbour queries (nbody_get_knn, nbody_batch_get_knn; include/nbody.h)
and what their tests share.  The states are those of the neighbour queries (neighbor_cases.py).

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance.  A row at (x, y), a source j at
(X_j, Y_j):
    dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)                  the d2 of nbody_get_neighbors
    eligible: d2_j < +inf (own form: and j is not the row, by index)
    the result: the first k eligible sources under (d2, j) ascending, then {+inf, -1} up to k
A stable sort of d2 along j - NaN and the self term set to +inf first - IS that order: equal d2 keep their ascending j, and
whatever sorts at +inf is an entry the definition leaves empty."""
import numpy as np

from neighbor_cases import lattice, probe_points, random_state  # noqa: F401  (the states the tests of both queries share)

KNN_MAX = 32


def model_knn(P, k, rows=None, points=None, chunk=128):
    """The definition over the sources P (n, 2) float64 (an fp32 state widened exactly): at the bodies `rows` (all of them by
    default; the self term left out) or at explicit `points` (m, 2) -> {"d2": float64 (rows, k), "index": int32 (rows, k)}."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    n = len(P)
    X, Y = P[:, 0], P[:, 1]
    if points is None:
        rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        px, py = X[rows], Y[rows]
    else:
        assert rows is None
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py = points[:, 0], points[:, 1]
    m = len(px)
    d2_out = np.full((m, k), np.inf, dtype=np.float64)
    idx_out = np.full((m, k), -1, dtype=np.int32)
    if n == 0:
        return {"d2": d2_out, "index": idx_out}
    take = min(k, n)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, m, chunk):
            sl = slice(a, min(a + chunk, m))
            dx = X[None, :] - px[sl, None]
            dy = Y[None, :] - py[sl, None]
            d2 = (dx * dx) + (dy * dy)
            cand = np.where(np.isnan(d2), np.inf, d2)           # a NaN is never eligible
            if rows is not None:
                cand[np.arange(sl.stop - sl.start), rows[sl]] = np.inf
            order = np.argsort(cand, axis=1, kind="stable")[:, :take]
            best = np.take_along_axis(cand, order, axis=1)
            d2_out[sl, :take] = best
            idx_out[sl, :take] = np.where(best < np.inf, order, -1)
    return {"d2": d2_out, "index": idx_out}


def loop_knn(P, k, rows=None, points=None):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation): every eligible
    (d2, j), sorted as tuples, the first k."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    n = len(P)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    if points is None:
        rows = range(n) if rows is None else [int(i) for i in rows]
        todo = [(X[i], Y[i], i) for i in rows]
    else:
        todo = [(float(q[0]), float(q[1]), -1) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    d2_out = np.full((len(todo), k), np.inf, dtype=np.float64)
    idx_out = np.full((len(todo), k), -1, dtype=np.int32)
    for p, (x, y, i) in enumerate(todo):
        found = []
        for j in range(n):
            if j == i:
                continue
            dx = X[j] - x
            dy = Y[j] - y
            try:
                d2 = (dx * dx) + (dy * dy)
            except OverflowError:                                # Python raises where IEEE gives +inf
                d2 = float("inf")
            if d2 < float("inf"):                                # false for NaN too
                found.append((d2, j))
        found.sort()
        for c, (d2, j) in enumerate(found[:k]):
            d2_out[p, c], idx_out[p, c] = d2, j
    return {"d2": d2_out, "index": idx_out}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Zero tolerance: d2 by bits, index exactly."""
    return (a["d2"].shape == b["d2"].shape and a["index"].shape == b["index"].shape
            and np.array_equal(bits(a["d2"]), bits(b["d2"])) and np.array_equal(a["index"], b["index"]))


def assert_same(got, want, what=""):
    gd, gi, wd, wi = np.asarray(got["d2"]), np.asarray(got["index"]), np.asarray(want["d2"]), np.asarray(want["index"])
    assert gd.dtype == np.float64 and gi.dtype == np.int32, (what, gd.dtype, gi.dtype)
    assert gd.shape == wd.shape and gi.shape == wi.shape and gd.shape == gi.shape, (what, gd.shape, gi.shape, wd.shape)
    bad = np.argwhere((bits(gd) != bits(wd)) | (gi != wi))
    if bad.size:
        r, c = bad[0][-2], bad[0][-1]
        lead = tuple(bad[0][:-2])
        raise AssertionError((what, "%d entries differ, first at %s" % (len(bad), tuple(bad[0])),
                              "got", gd[lead + (r,)].tolist(), gi[lead + (r,)].tolist(),
                              "want", wd[lead + (r,)].tolist(), wi[lead + (r,)].tolist(), "column %d" % c))


def sliced(res, sl):
    """Rows `sl` of a result."""
    return {"d2": res["d2"][sl], "index": res["index"][sl]}


def check_invariants(res, rows=None):
    """What the header states follows from the definition, on any result: d2 non-decreasing along a row, empty entries
    {+inf, -1} and only at the end, indices distinct and (own form, `rows` the rows' own indices) not the row's own."""
    d2, idx = res["d2"], res["index"]
    assert not np.isnan(d2).any()
    assert (d2[..., 1:] >= d2[..., :-1]).all()
    assert ((idx == -1) == (d2 == np.inf)).all()
    flat_i = idx.reshape(-1, idx.shape[-1])
    for r in range(len(flat_i)):
        live = flat_i[r][flat_i[r] >= 0]
        assert len(np.unique(live)) == len(live), r
    if rows is not None:
        assert (idx != np.asarray(rows).reshape(-1, 1)).all()
