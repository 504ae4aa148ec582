"""The numpy model of the shell moments (nbody_get_shell_moments, nbody_batch_get_shell_moments; include/nbody.h, DESIGN.md
4.19) and the states their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma, no divide, no square root - numpy's
elementwise float64 arithmetic - so the model restates it bit for bit and the GPU tests compare with zero tolerance: the nine
sums by their bits (a NaN as a NaN, see sum_bits), count and pad exactly.  A row at (x, y) with velocity (vx, vy), a source
j with (X_j, Y_j, VX_j, VY_j, M_j), an fp32 state widened exactly:
    dx = X_j - x;  dy = Y_j - y;  d2 = (dx*dx) + (dy*dy)
    in(k, j)  <=>  e2[k] <= d2 && d2 < e2[k+1]
    ux = VX_j - vx;  uy = VY_j - vy;  w2 = (ux*ux) + (uy*uy);  s = (dx*ux) + (dy*uy);  c = (dx*uy) - (dy*ux)
    mass: M_j   px: M_j*ux   py: M_j*uy   ke: M_j*w2   mr2: M_j*d2   rad: M_j*s   ang: M_j*c   rad2: M_j*(s*s)   ang2: M_j*(c*c)
each summed as  acc = +0.0;  for j ascending:  if in(k, j)  acc = acc + term,  with body i's own term left out by index when
the rows are the bodies.  A point without a velocity is at rest: (vx, vy) = (+0.0, +0.0).

The ORDER of every sum is part of the contract.  model_shell_moments takes it with np.cumsum along j, which adds one element
after the other; a source outside the bin enters as +0.0, which leaves an accumulator that started at +0.0 as it is, bit for
bit, also where the terms are signed: such an accumulator is never -0.0, since a sum is -0.0 only where both terms are.
loop_shell_moments is the definition as written, and test_shell_moment_cases_cpu.py holds the one against the other."""
import numpy as np

import shell_cases as shc
from shell_cases import ORDER_SEED, bits, probe_points, tenth_edges, tenth_field  # noqa: F401  (what the tests share)

SHELL_MOMENTS_MAX = 8                                           # of one library call
FIELDS = ("mass", "px", "py", "ke", "mr2", "rad", "ang", "rad2", "ang2")
VELOCITY_FIELDS = ("px", "py", "ke", "rad", "ang", "rad2", "ang2")
DTYPE = np.dtype([(f, np.float64) for f in FIELDS] + [("count", np.int32), ("pad", np.int32)])
CHUNK_BYTES = 16 << 20                                          # of one n-wide float64 temporary of the model
VELOCITY_SEED_OFFSET = 104729


def widen_state(b):
    """A BodiesData (or a download) -> (P, V, M) float64, exact."""
    return (np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Velocities, dtype=np.float64),
            np.asarray(b.Masses, dtype=np.float64))


def model_shell_moments(P, V, M, edges2, points=None, point_vel=None, descending=False, rows=None):
    """The definition over the bodies P (n, 2) with velocities V (n, 2) and masses M (n,), float64 (an fp32 state widened
    exactly), and the B + 1 squared edges: at the bodies `rows` (all of them by default; the self term left out) with their
    own velocities, or at explicit `points` (m, 2) moving with `point_vel` (m, 2; None: at rest) -> {"moments": DTYPE
    (rows, B), "edges2"}.  descending=True adds in descending j instead: NOT the contract, only what the tests hold a state's
    sensitivity to the order against."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 2)
    M = np.asarray(M, dtype=np.float64).reshape(-1)
    e2 = np.asarray(edges2, dtype=np.float64).reshape(-1)
    B, n = len(e2) - 1, len(P)
    X, Y, VX, VY = P[:, 0], P[:, 1], V[:, 0], V[:, 1]
    own = points is None
    if own:
        assert point_vel is None
        me = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
        px, py, pvx, pvy = X[me], Y[me], VX[me], VY[me]
    else:
        assert rows is None
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py = points[:, 0], points[:, 1]
        vel = np.zeros_like(points) if point_vel is None else np.asarray(point_vel, dtype=np.float64).reshape(-1, 2)
        pvx, pvy = vel[:, 0], vel[:, 1]
    rows = len(px)
    out = np.zeros((rows, B), dtype=DTYPE)
    chunk = max(1, CHUNK_BYTES // (8 * max(n, 1)))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, rows if n else 0, chunk):
            b = min(a + chunk, rows)
            dx = X[None, :] - px[a:b, None]                     # [row, j] = X_j - x
            dy = Y[None, :] - py[a:b, None]
            d2 = (dx * dx) + (dy * dy)
            ux = VX[None, :] - pvx[a:b, None]
            uy = VY[None, :] - pvy[a:b, None]
            w2 = (ux * ux) + (uy * uy)
            s = (dx * ux) + (dy * uy)
            c = (dx * uy) - (dy * ux)
            Mj = np.broadcast_to(M[None, :], d2.shape)
            terms = {"mass": Mj, "px": Mj * ux, "py": Mj * uy, "ke": Mj * w2, "mr2": Mj * d2, "rad": Mj * s, "ang": Mj * c,
                     "rad2": Mj * (s * s), "ang2": Mj * (c * c)}
            for k in range(B):
                inside = (e2[k] <= d2) & (d2 < e2[k + 1])
                if own:
                    inside[np.arange(b - a), me[a:b]] = False
                out["count"][a:b, k] = inside.sum(axis=1)
                for f in FIELDS:
                    t = np.where(inside, terms[f], 0.0)
                    if descending:
                        t = t[:, ::-1]
                    t[:, 0] = 0.0 + t[:, 0]                     # acc starts at +0.0: a first term of -0.0 gives +0.0
                    out[f][a:b, k] = np.cumsum(t, axis=1)[:, -1]    # one after the other along j
    return {"moments": out, "edges2": e2}


def loop_shell_moments(P, V, M, edges2, points=None, point_vel=None):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 2)
    e2 = [float(v) for v in np.asarray(edges2, dtype=np.float64).reshape(-1)]
    B, n = len(e2) - 1, len(P)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    VX, VY = [float(v) for v in V[:, 0]], [float(v) for v in V[:, 1]]
    Mm = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
    if points is None:
        todo = [(X[i], Y[i], VX[i], VY[i], i) for i in range(n)]
    else:
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        vel = np.zeros_like(points) if point_vel is None else np.asarray(point_vel, dtype=np.float64).reshape(-1, 2)
        todo = [(float(q[0]), float(q[1]), float(v[0]), float(v[1]), -1) for q, v in zip(points, vel)]
    out = np.zeros((len(todo), B), dtype=DTYPE)
    for row, (x, y, vx, vy, i) in enumerate(todo):
        for k in range(B):
            acc = dict.fromkeys(FIELDS, 0.0)
            cnt = 0
            for j in range(n):
                if j == i:
                    continue
                dx = X[j] - x
                dy = Y[j] - y
                d2 = (dx * dx) + (dy * dy)
                if e2[k] <= d2 and d2 < e2[k + 1]:
                    ux = VX[j] - vx
                    uy = VY[j] - vy
                    w2 = (ux * ux) + (uy * uy)
                    s = (dx * ux) + (dy * uy)
                    c = (dx * uy) - (dy * ux)
                    m = Mm[j]
                    acc["mass"] = acc["mass"] + m
                    acc["px"] = acc["px"] + m * ux
                    acc["py"] = acc["py"] + m * uy
                    acc["ke"] = acc["ke"] + m * w2
                    acc["mr2"] = acc["mr2"] + m * d2
                    acc["rad"] = acc["rad"] + m * s
                    acc["ang"] = acc["ang"] + m * c
                    acc["rad2"] = acc["rad2"] + m * (s * s)
                    acc["ang2"] = acc["ang2"] + m * (c * c)
                    cnt += 1
            for f in FIELDS:
                out[f][row, k] = acc[f]
            out["count"][row, k] = cnt
    return {"moments": out, "edges2": np.asarray(e2, dtype=np.float64)}


def sum_bits(a):
    """The bits of fp64 sums with every NaN as the one quiet NaN: IEEE 754 leaves the sign and the payload of a NaN result
    open, and they do differ - the device subtracts by adding the negated operand, which flips the sign of a NaN operand
    where numpy's subtraction keeps it.  Everything that is no NaN is compared by its bits, -0.0 against +0.0 included."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def differing(a, b, field):
    """How many entries of `field` differ by bits (sum_bits) between two moment arrays of one shape."""
    return int((sum_bits(a[field]) != sum_bits(b[field])).sum())


def same(a, b):
    """Zero tolerance: the nine sums by bits, count and pad exactly."""
    a, b = np.asarray(a), np.asarray(b)
    return (a.shape == b.shape and all(differing(a, b, f) == 0 for f in FIELDS)
            and np.array_equal(a["count"], b["count"]) and np.array_equal(a["pad"], b["pad"]))


def assert_same(got, want, what=""):
    """got, want: results ({"moments", ["edges2"]}) or moment arrays."""
    g = np.asarray(got["moments"] if isinstance(got, dict) else got)
    w = np.asarray(want["moments"] if isinstance(want, dict) else want)
    assert g.dtype == DTYPE and w.dtype == DTYPE, (what, g.dtype, w.dtype)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g["count"] != w["count"])
    assert len(bad) == 0, (what, "%d counts differ, first at %s" % (len(bad), bad[0]), g["count"][tuple(bad[0])],
                           w["count"][tuple(bad[0])])
    assert not g["pad"].any(), (what, "pad is not 0")
    for f in FIELDS:
        bad = np.argwhere(sum_bits(g[f]) != sum_bits(w[f]))
        assert len(bad) == 0, (what, "%d %s differ by bits, first at %s" % (len(bad), f, bad[0]), repr(g[f][tuple(bad[0])]),
                               repr(w[f][tuple(bad[0])]))
    if isinstance(got, dict) and isinstance(want, dict) and "edges2" in got and "edges2" in want:
        assert np.array_equal(bits(got["edges2"]), bits(want["edges2"])), (what, "edges2")


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
def velocities(n, dtype, seed=ORDER_SEED):
    """n velocities uniform in +-10, rounded to dtype, as float64."""
    rng = np.random.default_rng(seed + VELOCITY_SEED_OFFSET)
    return rng.uniform(-10.0, 10.0, size=(n, 2)).astype(dtype).astype(np.float64)


def moment_state(n, dtype, seed=ORDER_SEED, field=None):
    """shell_cases.order_sensitive_state - positions over tenth_field(n), masses log-uniform over 1e4 .. 1e17 - with
    velocities() -> (P, V, M) float64.  test_shell_moment_cases_cpu.py asserts that every one of the nine sums depends on
    the order for ORDER_SEED, both dtypes, n = 300 and tenth_edges."""
    P, M = shc.order_sensitive_state(n, dtype, seed, field)
    return P, velocities(n, dtype, seed), M


def point_velocities(m, seed):
    """m point velocities uniform in +-10 (fp64: points are always nbody_vec2)."""
    return np.random.default_rng(seed + VELOCITY_SEED_OFFSET).uniform(-10.0, 10.0, size=(m, 2))
