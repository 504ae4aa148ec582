"""The numpy model of the k nearest neighbours on the cell list (nbody_get_knn_grid, nbody_batch_get_knn_grid; include/nbody.h,
DESIGN.md 4.23), the model of their widening rule, and the states, grids and asks their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance.  The sources are the bodies inside the
grid (cell_cases.cell_index).  A row at (x, y), own index i (none for a probe point):
    dx = X_j - x;  dy = Y_j - y;  d2_j = (dx*dx) + (dy*dy)
    eligible(j)  <=>  inside(j) && j != i && d2_j < +inf && d2_j <= h2_max
    the result: the first k eligible sources under (d2, j) ascending, then {+inf, -1} up to k
model_knn_grid is brute force over all sources (a stable sort along j, as knn_cases.model_knn); loop_knn_grid is a scalar loop
that hands the sources over in DESCENDING j to an insertion that compares (d2, j), so that the order of the visit cannot
show; rule_model restates the widening rule round by round on within_cases._span - the rounds every row takes, the sources
it looks at in each, and the list it ends with: test_knn_grid_cases_cpu.py holds, for every case below, that the rule ends
with the brute-force result and that no eligible source it never looked at could have changed it."""
import functools

import numpy as np

import cell_cases as cc
import neighbor_cases as nc
import within_cases as wc

KNN_MAX = 32
ROUNDS_MAX = 48                                                 # from this round on the radius is +inf
H0_MIN = 2.0 ** -500
INFO_FIELDS = ("n", "rows", "inside", "outside", "widened", "rounds")


def _rows_of(P, points, rows=None):
    if points is None:
        rows = np.arange(len(P)) if rows is None else np.asarray(rows, dtype=np.int64)
        return P[rows, 0], P[rows, 1], rows
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return points[:, 0], points[:, 1], None


def _pairs(P, grid, h2_max, points, rows):
    """d2 (rows, n) and which of its entries are eligible."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    px, py, me = _rows_of(P, points, rows)
    inside = cc.cell_index(P, grid) >= 0
    with np.errstate(over="ignore", invalid="ignore"):
        dx = P[None, :, 0] - px[:, None]
        dy = P[None, :, 1] - py[:, None]
        d2 = (dx * dx) + (dy * dy)
        elig = inside[None, :] & (d2 < np.inf) & (d2 <= np.float64(h2_max))     # a NaN d2 passes neither compare
    if me is not None and len(P):
        elig[np.arange(len(me)), me] = False
    return d2, elig, inside, np.stack([px, py], axis=1)


def _first_k(d2, elig, k):
    """The first k of every row's eligible sources under (d2, j): a stable sort along j."""
    m, n = d2.shape
    out_d = np.full((m, k), np.inf, dtype=np.float64)
    out_i = np.full((m, k), -1, dtype=np.int32)
    if n:
        cand = np.where(elig, d2, np.inf)
        take = min(k, n)
        order = np.argsort(cand, axis=1, kind="stable")[:, :take]
        best = np.take_along_axis(cand, order, axis=1)
        out_d[:, :take] = best
        out_i[:, :take] = np.where(best < np.inf, order, -1)
    return out_d, out_i


def model_knn_grid(P, grid, k, h2_max=np.inf, points=None, rows=None):
    """The definition over the bodies P (n, 2) float64 (an fp32 state widened exactly), at the bodies (`rows`: only these) or
    at explicit `points` (m, 2) -> {"d2": float64 (rows, k), "index": int32 (rows, k), "info": n, rows, inside, outside}."""
    d2, elig, inside, _ = _pairs(P, grid, h2_max, points, rows)
    out_d, out_i = _first_k(d2, elig, k)
    n = len(inside)
    return {"d2": out_d, "index": out_i, "info": {"n": n, "rows": len(out_d), "inside": int(inside.sum()), "outside": n - int(inside.sum())}}


def model_knn_grid_sample(P, grid, k, h2_max, rows, chunk=32):
    """model_knn_grid for the bodies `rows` of a LARGE state, without the sort of every row's n candidates: the k-th smallest
    d2 by a partition, then the (d2, j) order among the candidates at or below it -> {"d2", "index"}."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    rows = np.asarray(rows, dtype=np.int64)
    out_d = np.full((len(rows), k), np.inf, dtype=np.float64)
    out_i = np.full((len(rows), k), -1, dtype=np.int32)
    for a in range(0, len(rows), chunk):
        d2, elig, _, _ = _pairs(P, grid, h2_max, None, rows[a:a + chunk])
        cand = np.where(elig, d2, np.inf)
        kth = np.partition(cand, k - 1, axis=1)[:, k - 1] if cand.shape[1] >= k else np.full(len(cand), np.inf)
        for r in range(len(cand)):
            j = np.flatnonzero((cand[r] <= kth[r]) & (cand[r] < np.inf))
            j = j[np.lexsort((j, cand[r, j]))][:k]
            out_d[a + r, :len(j)], out_i[a + r, :len(j)] = cand[r, j], j
    return {"d2": out_d, "index": out_i}


def loop_knn_grid(P, grid, k, h2_max=np.inf, points=None, rows=None):
    """The definition as a plain scalar loop over Python floats, the sources handed over in DESCENDING j to a sorted list
    whose insertion compares (d2, j): an entry moves down where d2 > v or (d2 == v and index > j)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    n, h2_max = len(P), float(h2_max)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    inside = [bool(v) for v in cc.cell_index(P, grid) >= 0]
    if points is None:
        todo = [(X[i], Y[i], i) for i in (range(n) if rows is None else [int(r) for r in rows])]
    else:
        todo = [(float(q[0]), float(q[1]), -1) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    out_d = np.full((len(todo), k), np.inf, dtype=np.float64)
    out_i = np.full((len(todo), k), -1, dtype=np.int32)
    inf = float("inf")
    for p, (x, y, i) in enumerate(todo):
        d, ix = [inf] * k, [-1] * k
        for j in reversed(range(n)):
            if not inside[j] or j == i:
                continue
            dx = X[j] - x
            dy = Y[j] - y
            try:
                v = (dx * dx) + (dy * dy)
            except OverflowError:                                # Python raises where IEEE gives +inf
                v = inf
            if not (v < inf and v <= h2_max):
                continue
            c = k
            while c > 0 and (d[c - 1] > v or (d[c - 1] == v and ix[c - 1] > j)):
                c -= 1
            if c < k:
                d[c + 1:], ix[c + 1:] = d[c:k - 1], ix[c:k - 1]
                d[c], ix[c] = v, j
        out_d[p], out_i[p] = d, ix
    return {"d2": out_d, "index": out_i}


def default_h0(grid):
    """What the wrapper takes for h0=None: the larger cell side."""
    _, _, sx, sy, _, _ = cc.grid_tuple(grid)
    return max(1.0 / float(sx), 1.0 / float(sy))


def _join(lo, hi, plo, phi):
    """Per axis a span is never narrower than the round before."""
    had, has = plo <= phi, lo <= hi
    both = had & has
    return (np.where(both, np.minimum(lo, plo), np.where(has, lo, plo)), np.where(both, np.maximum(hi, phi), np.where(has, hi, phi)))


def rule_model(P, grid, k, h0, h2_max=np.inf, points=None, rows=None):
    """The widening rule restated (knn_grid_walk of csrc/nbody_knn_grid.hpp) -> {"d2", "index": the list every row ends with,
    "rounds": int (rows,), "H2": float64 (rows,) the H2 of the round a row stopped in, "final": bool (rows,) whether that
    round was final, "looked": per round a bool (rows, n) of the sources first looked at in it, "seen": their union,
    "eligible": bool (rows, n), "pairs": d2 (rows, n), "info": every field of nbody_knn_grid_info}."""
    x0, y0, sx, sy, nx, ny = cc.grid_tuple(grid)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    d2, elig, inside, xy = _pairs(P, grid, h2_max, points, rows)
    m, n = d2.shape
    h0, h2_max = np.float64(h0), np.float64(h2_max)
    with np.errstate(over="ignore"):
        h02, h_max = h0 * h0, np.sqrt(h2_max)
    fine = not (sx <= 2.0 ** 400 and sy <= 2.0 ** 400)
    cell = cc.cell_index(P, grid)
    ix, iy = cell % nx, cell // nx
    with np.errstate(over="ignore", invalid="ignore"):
        tx, ty = (xy[:, 0] - x0) * sx, (xy[:, 1] - y0) * sy
    active = np.ones(m, dtype=bool)
    rounds = np.zeros(m, dtype=np.int64)
    stop_h2 = np.zeros(m)
    stop_final = np.zeros(m, dtype=bool)
    seen = np.zeros((m, n), dtype=bool)
    looked = []
    pc0, pc1 = np.zeros(m, dtype=np.int64), np.full(m, -1, dtype=np.int64)
    pr0, pr1 = pc0.copy(), pc1.copy()
    t = 0
    while active.any():
        with np.errstate(over="ignore", invalid="ignore"):
            h, H2 = (np.float64(np.inf),) * 2 if t >= ROUNDS_MAX else (np.ldexp(h0, t), np.ldexp(h02, 2 * t))
            last = bool(H2 >= h2_max)
            if last:
                h, H2 = h_max, h2_max
            every = fine and t == 0
            wx0, wy0 = (np.inf, np.inf) if every else (h * sx, h * sy)
        c0, c1 = _join(*wc._span(tx, wx0, nx), pc0, pc1)
        r0, r1 = _join(*wc._span(ty, wy0, ny), pr0, pr1)
        whole = (c0 == 0) & (c1 == nx - 1) & (r0 == 0) & (r1 == ny - 1)
        window = (inside[None, :] & (c0[:, None] <= ix[None, :]) & (ix[None, :] <= c1[:, None])
                  & (r0[:, None] <= iy[None, :]) & (iy[None, :] <= r1[:, None]))
        new = window & ~seen & active[:, None]
        looked.append(new)
        seen |= new
        if n >= k:
            kth = np.partition(np.where(seen & elig, d2, np.inf), k - 1, axis=1)[:, k - 1]
        else:
            kth = np.full(m, np.inf)
        done = last | whole | ((kth < np.inf) & (kth <= H2))
        rounds[active] += 1
        stop_h2[active & done] = H2
        stop_final[active & done] = (last | whole)[active & done]
        pc0, pc1 = np.where(active, c0, pc0), np.where(active, c1, pc1)
        pr0, pr1 = np.where(active, r0, pr0), np.where(active, r1, pr1)
        active &= ~done
        t += 1
    out_d, out_i = _first_k(d2, elig & seen, k)
    info = {"n": n, "rows": m, "inside": int(inside.sum()), "outside": n - int(inside.sum()),
            "widened": int((rounds > 1).sum()), "rounds": int(rounds.max()) if m else 0}
    return {"d2": out_d, "index": out_i, "rounds": rounds, "H2": stop_h2, "final": stop_final, "looked": looked, "seen": seen,
            "eligible": elig, "pairs": d2, "info": info}


def info_dict(info):
    return {f: int(info[f]) for f in INFO_FIELDS}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what="", info=True):
    """Zero tolerance: d2 by its bits, indices and info exactly.  info=False: d2 and index only."""
    gd, gi, wd, wi = np.asarray(got["d2"]), np.asarray(got["index"]), np.asarray(want["d2"]), np.asarray(want["index"])
    assert gd.dtype == np.float64 and gi.dtype == np.int32, (what, gd.dtype, gi.dtype)
    assert gd.shape == wd.shape == gi.shape == wi.shape, (what, gd.shape, gi.shape, wd.shape, wi.shape)
    bad = np.argwhere((bits(gd) != bits(wd)) | (gi != wi))
    if bad.size:
        r = bad[0][0]
        raise AssertionError((what, "%d entries differ, first at %s" % (len(bad), tuple(bad[0])), "got", gd[r].tolist(), gi[r].tolist(),
                              "want", wd[r].tolist(), wi[r].tolist()))
    if info:
        w = want["info"]
        g = {f: int(got["info"][f]) for f in w}
        assert g == {f: int(v) for f, v in w.items()}, (what, g, w)


# ---------------------------------------------------------------------------------------------------------------------
# the shared cases: a state, and the asks (nx, ny, bounds, k, h0 (None: the larger cell side), h2_max) it is put to
# ---------------------------------------------------------------------------------------------------------------------
BODY_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
TIERS = (1, 4, 5, 8, 9, 16, 17, 32)
DTYPES = wc.DTYPES
LATTICE_SIDE = 16
STACK = 40
CLUMP, SCATTER = 200, 57


class Case:
    """name; dtype; P (n, 2) float64, exact in dtype, and R (n,); asks = [(nx, ny, bounds, k, h0, h2_max), ...]; points or None."""

    def __init__(self, name, dtype, P, R, asks, points=None):
        self.name, self.dtype, self.P, self.R, self.asks, self.points = name, dtype, P, R, asks, points
        for a in (P, R) + (() if points is None else (points,)):
            a.setflags(write=False)

    def grid(self, ask):
        return cc.grid_of(*ask[:3])

    def h0(self, ask):
        return default_h0(self.grid(ask)) if ask[4] is None else ask[4]


def stack_state(dtype):
    """STACK bodies on one point - bodies 0 .. STACK - 1, d2 = 0 between any two - and 60 around it, over tenth_field(100)."""
    P, R, f = wc.state(100, dtype)
    P[:STACK] = P[0]
    return P, R, f


def clump_state(dtype):
    """CLUMP bodies inside cell (10, 10) of the 64 x 64 grid over [0, 64)^2 and SCATTER bodies over the whole field."""
    rng = np.random.default_rng(wc.STATE_SEED + 64)
    clump = 10.1 + 0.8 * rng.uniform(size=(CLUMP, 2))
    far = rng.uniform(0, 64, size=(SCATTER, 2))
    P = np.concatenate([clump, far])[rng.permutation(CLUMP + SCATTER)].astype(dtype).astype(np.float64)
    return P, np.full(len(P), 0.01)


@functools.lru_cache(maxsize=None)
def cases():
    """Every case of the GPU tests, by name.  Shared, never written to."""
    out = []
    inf = np.inf
    for tag, dtype in DTYPES.items():
        for n in BODY_COUNTS:                                   # wave and workgroup edges; k = 8 on 8 x 8, 1 x 1, and a grid
            P, R, f = wc.state(n, dtype)                        # that leaves bodies - rows - outside
            full, part = (0, f, 0, f), (0.25 * f, 0.75 * f, 0.25 * f, f)
            out.append(Case("bodies-%d-%s" % (n, tag), dtype, P, R,
                            [(8, 8, full, 8, None, inf), (1, 1, full, 8, None, inf), (8, 8, part, 8, None, inf)]))
        P, R, f = wc.state(300, dtype, coincident=True)
        full = (0, f, 0, f)
        out.append(Case("tiers-%s" % tag, dtype, P, R, [(8, 8, full, k, None, inf) for k in TIERS]))
        Q, QR, qf = wc.state(20, dtype)                         # k > n - 1: the padding
        out.append(Case("padding-%s" % tag, dtype, Q, QR, [(4, 4, (0, qf, 0, qf), k, None, inf) for k in (19, 20, 32)]))
        L, LR = nc.lattice(LATTICE_SIDE)                        # spacing = cell side = h0 = 1: the 4-neighbours at d2 == H2_0
        s = float(LATTICE_SIDE)
        out.append(Case("lattice-%s" % tag, dtype, L, LR,
                        [(LATTICE_SIDE, LATTICE_SIDE, (-o, s - o, -o, s - o), k, 1.0, inf) for o in (0.0, 0.1) for k in (4, 5)]))
        S, SR, sf = stack_state(dtype)
        out.append(Case("stack-%s" % tag, dtype, S, SR, [(8, 8, (0, sf, 0, sf), k, None, inf) for k in (8, 32)]))
        C, CR = clump_state(dtype)
        out.append(Case("clump-%s" % tag, dtype, C, CR, [(nx, ny, (0, 64, 0, 64), 8, 1.0, inf) for nx, ny in ((64, 64), (1, 7), (7, 1))]))
        out.append(Case("points-%s" % tag, dtype, P, R,
                        [(16, 16, full, 8, None, inf), (8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f), 8, None, inf), (4, 4, full, 3, None, inf)],
                        wc.awkward_points(P, f)))
        out.append(Case("first-radius-%s" % tag, dtype, P, R, [(8, 8, full, 8, h0, inf) for h0 in (None, H0_MIN, 1e300)]))
        with np.errstate(over="ignore"):
            third = np.sort(((P[1:, 0] - P[0, 0]) * (P[1:, 0] - P[0, 0])) + ((P[1:, 1] - P[0, 1]) * (P[1:, 1] - P[0, 1])))[2]
        out.append(Case("cut-%s" % tag, dtype, P, R,       # 0; one that leaves rows short of k; row 0's third d2 exactly; none
                        [(8, 8, full, 8, None, h2) for h2 in (0.0, (0.09 * f) ** 2, float(third), inf)]))
    return {c.name: c for c in out}


def case_names(prefix=""):
    return [k for k in cases() if k.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def reference(name, a):
    """rule_model of ask a of the case, computed once, read-only: what every test of that ask compares with."""
    case = cases()[name]
    ask = case.asks[a]
    ref = rule_model(case.P, case.grid(ask), ask[3], case.h0(ask), ask[5], case.points)
    for f in ("d2", "index", "rounds", "H2", "final", "seen", "eligible", "pairs"):
        ref[f].setflags(write=False)
    return ref
