"""The oracle and the error bound of the field evaluation (nbody_get_field, nbody_batch_get_field).

The oracle evaluates every term in np.longdouble (x86-64 80-bit: eps 2^-63), in the style of exact_phi in
test_gpu_diagnostics.py, and is called "exact":
    phi(x) = -G sum_j m_j / r_j          a(x) = -G sum_j m_j (x - x_j) / r_j^3          r_j = |x - x_j| > 0,
a source at distance exactly 0 left out of all three sums and counted.

The tolerances are summation error bounds with u = 2^-53, not fitted to runs:
  * phi: every term is within 4 u of its exact value and has one sign: (n + 4) u |phi|  (test_gpu_diagnostics.py);
  * each acceleration component: (n + ACC_C) u sum_j |G m_j (x - x_j) / r_j^3|.
ACC_C, first order in u, every rounding at most u (DESIGN.md 4.8 has the same derivation):
    dx = fl(x_j - x)                 inputs exact                                     1 u
    y  = diag_rinv(d2)               within 3 u of 1 / r              3 u
    y2 = fl(y y)                     3 + 3 + 1                                        7 u
    y3 = fl(y2 y)                    7 + 3 + 1                                       11 u
    w  = fl(m_j y3)                  11 + 1                                          12 u
    w dx inside the fma              exact product of the two: 12 + 1                13 u
so a term is within 13 u of m_j (x_j - x) / r_j^3.  The general code of a flagged sum has the same 13: d = sqrt(d2) 2 + 1 = 3 u
(hypot: 1 + 1), m / d 4 u, / d 8 u, dx / d 1 + 3 + 1 = 5 u, their exact product in the fma 13 u.  The n fmas of the running
sum (the first adds to +0 and only rounds the product) add at most n u of sum |term|, the product with G one more:
    |error| <= (n + 13 + 1) u sum |term|          ACC_C = 14.
"""
import numpy as np

U = 2.0 ** -53
G = float(np.float32(6.67408e-11))
LD = np.longdouble
ACC_C = 14
PHI_C = 4


def require_long_double():
    assert np.finfo(np.longdouble).eps < 1e-18, "the oracle needs an 80-bit long double (x86-64)"


def exact_field(P, M, rows=None, points=None):
    """The field of the sources (P (n, 2), M (n,), float64) at the bodies `rows` (self term left out, not counted) or
    at explicit `points` (k, 2) -> acc (k, 2), phi (k,), sum_j |term| per acceleration component (k, 2), all long
    double, and the number of sources at distance 0 (left out)."""
    assert (rows is None) != (points is None)
    x, y, m = P[:, 0].astype(LD), P[:, 1].astype(LD), M.astype(LD)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        px, py = x[rows], y[rows]
    else:
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        px, py = points[:, 0].astype(LD), points[:, 1].astype(LD)
    k = len(px)
    acc, mag, phi = np.zeros((k, 2), dtype=LD), np.zeros((k, 2), dtype=LD), np.zeros(k, dtype=LD)
    coincident = 0
    for a in range(0, k, 16):
        sl = slice(a, min(a + 16, k))
        dx = x[None, :] - px[sl, None]                          # x_j - x: a = +G sum m_j (x_j - x) / r^3
        dy = y[None, :] - py[sl, None]
        out = (dx == 0) & (dy == 0)
        coincident += int(out.sum())
        if rows is not None:
            own = np.zeros_like(out)
            own[np.arange(sl.stop - sl.start), rows[sl]] = True
            coincident -= int((out & own).sum())                # the self term: left out by index, not counted
            out |= own
        d = np.sqrt(dx * dx + dy * dy)
        d[out] = 1
        mm = np.where(out, LD(0), m[None, :])
        w = LD(G) * mm / d / d / d
        phi[sl] = -(LD(G) * mm / d).sum(axis=1)
        acc[sl, 0], acc[sl, 1] = (w * dx).sum(axis=1), (w * dy).sum(axis=1)
        mag[sl, 0], mag[sl, 1] = np.abs(w * dx).sum(axis=1), np.abs(w * dy).sum(axis=1)
    return acc, phi, mag, coincident


def field_errors(got_acc, got_phi, acc, phi, mag, n):
    """-> (acceleration error / bound, phi error / bound), elementwise; a bound of 0 asks for an exact 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.abs(np.asarray(got_acc).astype(LD) - acc)
        ba = (n + ACC_C) * LD(U) * mag
        ep = np.abs(np.asarray(got_phi).astype(LD) - phi)
        bp = (n + PHI_C) * LD(U) * np.abs(phi)
        ra = np.where(ea == 0, LD(0), ea / ba)
        rp = np.where(ep == 0, LD(0), ep / bp)
    return ra, rp


def check_field(got_acc, got_phi, acc, phi, mag, n, what=""):
    ra, rp = field_errors(got_acc, got_phi, acc, phi, mag, n)
    print("%s: n %d, %d points, worst acceleration error %.3f of its bound, worst phi error %.3f of its bound"
          % (what, n, len(phi), float(ra.max()) if ra.size else 0.0, float(rp.max()) if rp.size else 0.0))
    assert not (ra > 1).any() and not np.isnan(ra.astype(np.float64)).any(), (what, "acc", np.argwhere(ra > 1)[:8])
    assert not (rp > 1).any() and not np.isnan(rp.astype(np.float64)).any(), (what, "phi", np.argwhere(rp > 1)[:8])
