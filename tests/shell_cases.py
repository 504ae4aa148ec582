"""The numpy model of the shell sums (nbody_get_shells, nbody_batch_get_shells; include/nbody.h) and the
states their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance: count exactly, mass by its bits.  A row
at (x, y), a source j at (X_j, Y_j) with mass M_j, an fp32 state widened exactly:
    dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)
    in(k, j)  <=>  e2[k] <= d2_j && d2_j < e2[k+1]
    count[row, k] = the number of sources with in(k, j)
    mass [row, k] = acc after:  acc = +0.0;  for j ascending:  if in(k, j)  acc = acc + M_j
with body i's own term left out by index when the rows are the bodies.  A NaN d2 fails every comparison and a +inf d2 fails
`d2 < +inf`: neither is counted anywhere, whatever the edges.

The ORDER of the mass sum is part of the contract.  model_shells takes it with np.cumsum along j, which adds one element
after the other (np.sum and np.add.reduce add pairwise and are not used); a source outside the bin enters as +0.0, which
leaves an accumulator that started at +0.0 as it is, bit for bit: such an accumulator is never -0.0, since a sum is -0.0 only
where both terms are.  loop_shells is the definition as written, and test_shell_cases_cpu.py holds the one against the other."""
import numpy as np

from neighbor_cases import lattice, probe_points, random_state, widen  # noqa: F401  (the states the models share)

SHELLS_MAX = 32
CHUNK_BYTES = 32 << 20                                          # of one n-wide float64 temporary of the model
ORDER_SEED = 11                                                 # order_sensitive_state: see test_shell_cases_cpu.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def widen_mass(b):
    """A BodiesData (or a download) -> (P, M) float64, exact."""
    return np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Masses, dtype=np.float64)


def model_shells(P, M, edges2, points=None, descending=False, rows=None):
    """The definition over the bodies P (n, 2) with masses M (n,), float64 (an fp32 state widened exactly), and the B + 1
    squared edges: at the bodies `rows` (all of them by default; the self term left out), or at explicit `points` (m, 2) ->
    {"mass": float64 (rows, B), "count": int32 (rows, B), "edges2"}.  descending=True adds the masses in descending j
    instead: NOT the contract, only what the tests hold a state's sensitivity to the order against."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    M = np.asarray(M, dtype=np.float64).reshape(-1)
    e2 = np.asarray(edges2, dtype=np.float64).reshape(-1)
    B, n = len(e2) - 1, len(P)
    X, Y = P[:, 0], P[:, 1]
    own = points is None
    if own:
        me = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        px, py = X[me], Y[me]
    else:
        assert rows is None
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py = points[:, 0], points[:, 1]
    rows = len(px)
    mass = np.zeros((rows, B), dtype=np.float64)
    count = np.zeros((rows, B), dtype=np.int32)
    chunk = max(1, CHUNK_BYTES // (8 * max(n, 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, rows if n else 0, chunk):
            b = min(a + chunk, rows)
            dx = X[None, :] - px[a:b, None]                     # [row, j] = X_j - x
            dy = Y[None, :] - py[a:b, None]
            d2 = (dx * dx) + (dy * dy)
            for k in range(B):
                inside = (e2[k] <= d2) & (d2 < e2[k + 1])
                if own:
                    inside[np.arange(b - a), me[a:b]] = False
                count[a:b, k] = inside.sum(axis=1)
                terms = np.where(inside, M[None, :], 0.0)
                if descending:
                    terms = terms[:, ::-1]
                mass[a:b, k] = np.cumsum(terms, axis=1)[:, -1]  # one after the other along j
    return {"mass": mass, "count": count, "edges2": e2}


def loop_shells(P, M, edges2, points=None):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    e2 = [float(v) for v in np.asarray(edges2, dtype=np.float64).reshape(-1)]
    B, n = len(e2) - 1, len(P)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    Mm = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
    if points is None:
        todo = [(X[i], Y[i], i) for i in range(n)]
    else:
        todo = [(float(q[0]), float(q[1]), -1) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    mass = np.zeros((len(todo), B), dtype=np.float64)
    count = np.zeros((len(todo), B), dtype=np.int32)
    for row, (x, y, i) in enumerate(todo):
        for k in range(B):
            acc, cnt = 0.0, 0
            for j in range(n):
                if j == i:
                    continue
                dx = X[j] - x
                dy = Y[j] - y
                try:
                    d2 = (dx * dx) + (dy * dy)
                except OverflowError:                            # Python raises where IEEE gives +inf
                    d2 = float("inf")
                if e2[k] <= d2 and d2 < e2[k + 1]:
                    acc = acc + Mm[j]
                    cnt += 1
            mass[row, k], count[row, k] = acc, cnt
    return {"mass": mass, "count": count, "edges2": np.asarray(e2, dtype=np.float64)}


def sliced(res, rows):
    return {"mass": res["mass"][rows], "count": res["count"][rows], "edges2": res["edges2"]}


def same(a, b):
    """Zero tolerance: mass by bits, count exactly."""
    return (a["mass"].shape == b["mass"].shape and a["count"].shape == b["count"].shape
            and np.array_equal(bits(a["mass"]), bits(b["mass"])) and np.array_equal(a["count"], b["count"]))


def assert_same(got, want, what=""):
    gm, wm, gc, wc = (np.asarray(got["mass"]), np.asarray(want["mass"]), np.asarray(got["count"]), np.asarray(want["count"]))
    assert gm.dtype == np.float64 and gc.dtype == np.int32, (what, gm.dtype, gc.dtype)
    assert gm.shape == wm.shape and gc.shape == wc.shape and gm.shape == gc.shape, (what, gm.shape, wm.shape, gc.shape, wc.shape)
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, (what, "%d counts differ, first at %s" % (len(bad), bad[0]), gc[tuple(bad[0])], wc[tuple(bad[0])])
    bad = np.argwhere(bits(gm) != bits(wm))
    assert len(bad) == 0, (what, "%d masses differ by bits, first at %s" % (len(bad), bad[0]), repr(gm[tuple(bad[0])]),
                           repr(wm[tuple(bad[0])]))
    if "edges2" in got and "edges2" in want:
        assert np.array_equal(bits(got["edges2"]), bits(want["edges2"])), (what, "edges2")


# ---------------------------------------------------------------------------------------------------------------------
# states and edges
# ---------------------------------------------------------------------------------------------------------------------
def tenth_field(n):
    return 5.0 * np.sqrt(n)


def tenth_edges(field):
    """Eight bins up to the squared radius of a disc of a tenth of the field: pi t^2 = 0.1 with t = r / field, about 0.085 of
    the sources of an average row once the borders of the square are taken off (test_gpu_pairs.py sizes its edges so)."""
    return np.linspace(0.0, 0.1 * field * field / np.pi, 9)


def order_sensitive_state(n, dtype, seed=ORDER_SEED, field=None):
    """Positions as random_state over tenth_field(n), masses log-uniform over 1e4 .. 1e17 - the stock range - rounded to
    dtype -> (P, M) float64.  Thirteen decades: a sum of a handful of such masses depends on the order it is taken in, which
    test_shell_cases_cpu.py asserts for ORDER_SEED, both dtypes, n = 300 and tenth_edges."""
    field = tenth_field(n) if field is None else field
    P, _ = random_state(n, dtype, seed, field=field)
    rng = np.random.default_rng(seed + 7919)
    M = (10.0 ** rng.uniform(4.0, 17.0, size=n)).astype(dtype).astype(np.float64)
    return P, M


def order_matters(P, M, edges2, points=None):
    """How many (row, bin) masses of the model differ by bits from the same sums taken in descending j."""
    up, down = model_shells(P, M, edges2, points), model_shells(P, M, edges2, points, descending=True)
    assert np.array_equal(up["count"], down["count"])
    return int((bits(up["mass"]) != bits(down["mass"])).sum())
