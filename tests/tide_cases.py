"""The oracle and the error bounds of the tidal tensor and the jerk (nbody_get_tides, nbody_batch_get_tides).

The oracle evaluates every term in np.longdouble (x86-64 80-bit: eps 2^-63), in the style of field_cases.exact_field, and is
called "exact".  With d = x_j - x, r = |d| > 0, dv = v_j - v:
    T_ab(x)     = G sum_j m_j (3 d_a d_b / r^5 - delta_ab / r^3)                 -> txx, txy, tyy
    adot_a(x,v) = G sum_j m_j (dv_a / r^3 - 3 (d . dv) d_a / r^5)                -> jx, jy
a source at distance exactly 0 left out of every sum and counted.

The tolerances are summation error bounds with u = 2^-53, not fitted to runs:
    |error of T_ab|   <= (TIDE_K n + TIDE_C) u B_ab        B_ab = G sum_j m_j (3 |d_a d_b| / r^2 + delta_ab) / r^3
    |error of adot_a| <= (JERK_K n + JERK_C) u B_a         B_a  = G sum_j m_j (|dv_a| + 3 (|dx dvx| + |dy dvy|) |d_a| / r^2) / r^3
The library's chain (csrc/nbody_tides.hpp) keeps six running sums per row with w = m_j y^3, u_a = d_a y, y = diag_rinv(d2):
sw = sum w, s_ab = sum (3 w u_a) u_b, j_a = sum (w dv_a - (3 w (u . dv)) u_a), and reports G (sxx - sw), G sxy, G (syy - sw),
G jx, G jy.  First order in u, every rounding at most u, the inputs exact (DESIGN.md 4.17 has the same table):
    dx  = fl(x_j - x)                                                                 1 u
    y   = diag_rinv(d2)              within 3 u of 1 / r              3 u
    y2  = fl(y y)                    3 + 3 + 1                                        7 u
    y3  = fl(y2 y)                   7 + 3 + 1                                       11 u
    w   = fl(m_j y3)                 11 + 1                                          12 u      the term of sw
    w3  = fl(3 w)                    12 + 1                                          13 u
    ux  = fl(dx y)                   1 + 3 + 1                                        5 u
    px  = fl(w3 ux)                  13 + 5 + 1                                      19 u
    px ub inside the fma             exact product: 19 + 5                           24 u      the term of s_ab
    dvx = fl(vx_j - vx)                                                               1 u
    ru  = fma(ux, dvx, fl(uy dvy))   ux dvx 5 + 1 = 6; fl(uy dvy) 5 + 1 + 1 = 7; the fma's rounding 1 u of |ru|:
                                                                                      8 u of |ux dvx| + |uy dvy|
    k   = fl(w3 ru)                  13 + 8 + 1                                      22 u
    w dva inside the fma             12 + 1                                          13 u      the first term of j_a
    k ua inside the fma              22 + 5                                          27 u      the second term of j_a
Tensor: s_ab takes one rounding per pair, at most u of a partial sum, which is at most sum |term|: with the terms,
(n + 24) u sum |3 w u_a u_b|; sw likewise (n + 12) u sum w.  The difference sxx - sw rounds once, u |sxx - sw| <= u B / G, and
the product with G once more:
    |error of T_ab| <= (n + 24 + 2) u B_ab                 TIDE_K = 1, TIDE_C = 26.
Jerk: j_a takes TWO roundings per pair (one per fma), each at most u of a partial sum <= B_a / G; the terms are within
max(13, 27) u; the product with G one more:
    |error of adot_a| <= (2 n + 27 + 1) u B_a              JERK_K = 2, JERK_C = 28.
The general code of a flagged sum feeds the same sums with q = ((m / d) / d) / d and u_a = d_a / d in place of w and d_a y:
d = sqrt(d2) is within 2 + 1 = 3 u (hypot: 1 + 1), q within 3 + 1, + 3 + 1, + 3 + 1 = 12 u - w's 12; d_a / d within 1 + 3 + 1 = 5 u -
ux's 5.  Every line below them is the same line: it reaches the same 24, 13 and 27, so the same constants hold.
"""
import numpy as np

from field_cases import G, LD, U, require_long_double  # noqa: F401  (re-exported: the tests take them from here)

TIDE_K, TIDE_C = 1, 26
JERK_K, JERK_C = 2, 28


def exact_tides(P, V, M, rows=None, points=None, point_vel=None):
    """The tidal tensor and the jerk of the sources (P (n, 2), V (n, 2) or None for sources at rest, M (n,), float64) at the
    bodies `rows` (self term left out, not counted; their own velocities) or at explicit `points` (k, 2) with velocities
    `point_vel` (k, 2; None: at rest) -> tide (k, 3) txx, txy, tyy; jerk (k, 2); the number of sources at distance 0 (left
    out); B_ab (k, 3) and B_a (k, 2), the magnitude sums the bounds refer to.  All long double."""
    assert (rows is None) != (points is None)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    V = np.zeros_like(P) if V is None else np.asarray(V, dtype=np.float64).reshape(-1, 2)
    x, y, m = P[:, 0].astype(LD), P[:, 1].astype(LD), np.asarray(M, dtype=np.float64).astype(LD)
    vx, vy = V[:, 0].astype(LD), V[:, 1].astype(LD)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        px, py, pvx, pvy = x[rows], y[rows], vx[rows], vy[rows]
    else:
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        pv = np.zeros_like(points) if point_vel is None else np.asarray(point_vel, dtype=np.float64).reshape(-1, 2)
        assert pv.shape == points.shape
        px, py, pvx, pvy = points[:, 0].astype(LD), points[:, 1].astype(LD), pv[:, 0].astype(LD), pv[:, 1].astype(LD)
    k = len(px)
    tide, bt = np.zeros((k, 3), dtype=LD), np.zeros((k, 3), dtype=LD)
    jerk, bj = np.zeros((k, 2), dtype=LD), np.zeros((k, 2), dtype=LD)
    coincident = 0
    for a in range(0, k, 16):
        sl = slice(a, min(a + 16, k))
        dx, dy = x[None, :] - px[sl, None], y[None, :] - py[sl, None]
        dvx, dvy = vx[None, :] - pvx[sl, None], vy[None, :] - pvy[sl, None]
        out = (dx == 0) & (dy == 0)
        coincident += int(out.sum())
        if rows is not None:
            own = np.zeros_like(out)
            own[np.arange(sl.stop - sl.start), rows[sl]] = True
            coincident -= int((out & own).sum())                # the self term: left out by index, not counted
            out |= own
        d = np.hypot(dx, dy)                                    # long double hypot: no overflow of dx^2 for |dx| <= 2^600
        d[out] = 1
        q = LD(G) * np.where(out, LD(0), m[None, :]) / d / d / d    # G m / r^3
        ux, uy = dx / d, dy / d
        ru = ux * dvx + uy * dvy                                # (d . dv) / r
        tide[sl, 0] = (q * (3 * ux * ux - 1)).sum(axis=1)
        tide[sl, 1] = (q * 3 * ux * uy).sum(axis=1)
        tide[sl, 2] = (q * (3 * uy * uy - 1)).sum(axis=1)
        bt[sl, 0] = (q * (3 * ux * ux + 1)).sum(axis=1)
        bt[sl, 1] = (q * 3 * np.abs(ux * uy)).sum(axis=1)
        bt[sl, 2] = (q * (3 * uy * uy + 1)).sum(axis=1)
        jerk[sl, 0] = (q * (dvx - 3 * ru * ux)).sum(axis=1)
        jerk[sl, 1] = (q * (dvy - 3 * ru * uy)).sum(axis=1)
        mag = np.abs(ux * dvx) + np.abs(uy * dvy)
        bj[sl, 0] = (q * (np.abs(dvx) + 3 * mag * np.abs(ux))).sum(axis=1)
        bj[sl, 1] = (q * (np.abs(dvy) + 3 * mag * np.abs(uy))).sum(axis=1)
    return tide, jerk, coincident, bt, bj


def _ratio(got, want, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(np.asarray(got).astype(LD) - want)
        return np.where(e == 0, LD(0), e / bound)


def tide_errors(got_tide, tide, bt, n):
    """-> tensor error / bound, elementwise; a bound of 0 asks for an exact 0."""
    return _ratio(got_tide, tide, (TIDE_K * n + TIDE_C) * LD(U) * bt)


def jerk_errors(got_jerk, jerk, bj, n):
    return _ratio(got_jerk, jerk, (JERK_K * n + JERK_C) * LD(U) * bj)


def check_tides(got_tide, got_jerk, tide, jerk, bt, bj, n, what=""):
    """got_jerk None: the tensor alone."""
    rt = tide_errors(got_tide, tide, bt, n)
    rj = jerk_errors(got_jerk, jerk, bj, n) if got_jerk is not None else np.zeros((0, 2), dtype=LD)
    print("%s: n %d, %d rows, worst tensor error %.3f of its bound, worst jerk error %.3f of its bound"
          % (what, n, len(tide), float(rt.max()) if rt.size else 0.0, float(rj.max()) if rj.size else 0.0))
    assert not (rt > 1).any() and not np.isnan(rt.astype(np.float64)).any(), (what, "tide", np.argwhere(rt > 1)[:8])
    assert not (rj > 1).any() and not np.isnan(rj.astype(np.float64)).any(), (what, "jerk", np.argwhere(rj > 1)[:8])


# The fp64 states far outside the usual range (test_gpu_tides.py; checked without a device in test_tide_cases_cpu.py): three
# bodies 2^e apart with masses 2^me (1, 3, 5 times), velocities 2^ve.  e: the separations of test_gpu_field.py; me and ve so
# that every exact term - m / r^3 times a factor within [1/8, 16], the jerk's times |dv| - is a normal double.
FAR_CASES = [(-300, 0, 60), (300, 0, -40), (-520, -600, 20), (520, 600, 30), (-345, -100, 20)]


def far_state(e, me, ve):
    d, m, v = 2.0 ** e, 2.0 ** me, 2.0 ** ve
    P = np.array([[0.0, 0.0], [d, 0.0], [0.0, -d]])
    V = np.array([[v, -2 * v], [-3 * v, v], [0.5 * v, 4 * v]])
    M = np.array([m, 3 * m, 5 * m])
    pts = np.array([[-d, 0.0], [d, d]])
    pv = np.array([[v, v], [-2 * v, 0.25 * v]])
    return P, V, M, pts, pv
