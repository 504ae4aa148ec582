"""The numpy model of the bound-pair query (nbody_get_binaries, nbody_batch_get_binaries, nbody_binary_finish;
include/nbody.h) and the states its tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic,
its sqrt and its division are correctly rounded - so the model restates it bit for bit and the GPU tests compare with zero
tolerance.  A pair i < j of bodies (X, Y, M, R) with velocities (VX, VY), an fp32 state widened exactly, sep2 >= 0:
    dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
    d2 = (dx*dx) + (dy*dy);   coincident = d2 == 0;   near = 0 < d2 and d2 <= sep2
    v2 = (dvx*dvx) + (dvy*dvy);   mu = G2 * (M_i + M_j);   w = (v2*v2) * d2;   k = mu * mu
    bound = near and 0 < mu and k < inf and w < k
    hz = (dx*dvy) - (dy*dvx);   b = (dx*dvx) + (dy*dvy);   s = R_i + R_j
    flags: OVERLAP = 1 where d2 <= s*s, APPROACHING = 2 where b < 0
and per bound pair (finish)
    r = sqrt(d2);  gm = 0.5*mu;  eps = (0.5*v2) - (gm/r)
    a = gm / (-(eps+eps)) if eps < 0 else inf
    e2 = 1.0 + (((eps+eps) * (hz*hz)) / (gm*gm));   ecc = sqrt(e2) if e2 > 0 else +0.0
    period = 6.283185307179586 * sqrt(((a*a)*a) / gm) if a < inf else inf;   sep = r
The list is sorted by (i, j)."""
import math

import numpy as np

OVERLAP, APPROACHING = 1, 2
G2 = 2.0 * float(np.float32(6.67408e-11))
TWO_PI = 6.283185307179586
ORBIT = ("a", "ecc", "period", "sep")
BIN_DTYPE = np.dtype([("a", np.float64), ("ecc", np.float64), ("period", np.float64), ("sep", np.float64), ("i", np.int32),
                      ("j", np.int32), ("flags", np.uint32)])
RECORD_DTYPE = np.dtype([("a", np.float64), ("ecc", np.float64), ("period", np.float64), ("sep", np.float64), ("i", np.int32),
                         ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32)])
RAW_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32), ("d2", np.float64),
                      ("v2", np.float64), ("mu", np.float64), ("hz", np.float64)])
INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("pairs", np.int64), ("near", np.int64), ("coincident", np.int64),
                       ("overlapping", np.int64), ("approaching", np.int64), ("sep2", np.float64)])
COUNTS = ("n_bodies", "pairs", "near", "coincident", "overlapping", "approaching")
CHUNK_BYTES = 16 << 20                                          # of one n-wide float64 temporary of the model
SEP = 15.0                                                      # the largest separation of the standard state
STANDARD_N = (63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1500)
DTYPE_OF = {0: np.float32, 1: np.float64}


def widen(bodies):
    """(P (n, 2), V (n, 2), M (n,), R (n,)) of a BodiesData as float64 (exact)."""
    n = bodies.numBodies
    return (np.asarray(bodies.Positions[:n], dtype=np.float64).reshape(n, 2), np.asarray(bodies.Velocities[:n], dtype=np.float64).reshape(n, 2),
            np.asarray(bodies.Masses[:n], dtype=np.float64).reshape(n), np.asarray(bodies.Radii[:n], dtype=np.float64).reshape(n))


def standard_state(n, dtype, seed=None):
    """Positions uniform in +-7 sqrt(n), velocities uniform in +-40, masses 10**uniform(11, 15), radii uniform in [0.5, 2.5],
    drawn in that order from default_rng(n), each cast to `dtype` and widened back: at SEP about 1.6 n near pairs, of them
    about 0.7 n bound (v2 * r < 2 G (m_i + m_j): at r = 10 and |dv| = 40 the boundary is m_i + m_j = 1.2e14)."""
    rng = np.random.default_rng(n if seed is None else seed)
    half = 7.0 * np.sqrt(n)
    P = rng.uniform(-half, half, size=(n, 2)).astype(dtype).astype(np.float64)
    V = rng.uniform(-40.0, 40.0, size=(n, 2)).astype(dtype).astype(np.float64)
    M = (10.0 ** rng.uniform(11.0, 15.0, size=n)).astype(dtype).astype(np.float64)
    R = rng.uniform(0.5, 2.5, size=n).astype(dtype).astype(np.float64)
    return P, V, M, R


def _state(P, V, M, R):
    P, V = (np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in (P, V))
    M, R = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (M, R))
    return P, V, M, R


def _define(dx, dy, dvx, dvy, msum, s, sep2):
    """The definition on arrays of pairs -> (coincident, near, bound, flags, d2, v2, mu, hz)."""
    d2 = (dx * dx) + (dy * dy)
    coincident = d2 == 0.0
    near = (0.0 < d2) & (d2 <= sep2)
    v2 = (dvx * dvx) + (dvy * dvy)
    mu = G2 * msum
    w = (v2 * v2) * d2
    k = mu * mu
    bound = near & (0.0 < mu) & (k < np.inf) & (w < k)
    hz = (dx * dvy) - (dy * dvx)
    b = (dx * dvx) + (dy * dvy)
    flags = (d2 <= s * s).astype(np.uint32) * OVERLAP + (b < 0.0).astype(np.uint32) * APPROACHING
    return coincident, near, bound, flags, d2, v2, mu, hz


def finish_values(d2, v2, mu, hz):
    """(a, ecc, period, sep, eps, e2) of bound pairs from their raw values: what nbody_binary_finish computes."""
    d2, v2, mu, hz = (np.asarray(x, dtype=np.float64) for x in (d2, v2, mu, hz))
    with np.errstate(all="ignore"):
        r = np.sqrt(d2)
        gm = 0.5 * mu
        eps = (0.5 * v2) - (gm / r)
        a = np.where(eps < 0.0, gm / (-(eps + eps)), np.inf)
        e2 = 1.0 + (((eps + eps) * (hz * hz)) / (gm * gm))
        ecc = np.where(e2 > 0.0, np.sqrt(e2), 0.0)
        period = np.where(a < np.inf, TWO_PI * np.sqrt(((a * a) * a) / gm), np.inf)
    return a, ecc, period, r, eps, e2


def _sorted(i, j, flags, orbit):
    order = np.lexsort((j, i))
    out = np.zeros(len(order), dtype=BIN_DTYPE)
    out["i"], out["j"], out["flags"] = i[order], j[order], flags[order]
    for f, v in zip(ORBIT, orbit):
        out[f] = v[order]
    return out


def model_finish(raw):
    """nbody_binary_finish on RAW_DTYPE records."""
    i, j = np.minimum(raw["i"], raw["j"]), np.maximum(raw["i"], raw["j"])
    return _sorted(i, j, raw["flags"] & (OVERLAP | APPROACHING), finish_values(raw["d2"], raw["v2"], raw["mu"], raw["hz"])[:4])


def _info(n, flags, near, coincident, sep2):
    flags = np.asarray(flags, dtype=np.uint32)
    return {"n_bodies": int(n), "pairs": int(len(flags)), "near": int(near), "coincident": int(coincident),
            "overlapping": int(((flags & OVERLAP) != 0).sum()), "approaching": int(((flags & APPROACHING) != 0).sum()),
            "sep2": float(sep2)}


def _collect(n, parts, near, coincident, sep2, want_raw):
    if parts:
        i, j, flags, d2, v2, mu, hz = (np.concatenate([p[k] for p in parts]) for k in range(7))
    else:
        i = j = np.zeros(0, dtype=np.int64)
        flags = np.zeros(0, dtype=np.uint32)
        d2 = v2 = mu = hz = np.zeros(0)
    out = _sorted(i, j, flags, finish_values(d2, v2, mu, hz)[:4])
    info = _info(n, flags, near, coincident, sep2)
    if not want_raw:
        return out, info
    raw = np.zeros(len(i), dtype=RAW_DTYPE)
    raw["i"], raw["j"], raw["flags"], raw["d2"], raw["v2"], raw["mu"], raw["hz"] = i, j, flags, d2, v2, mu, hz
    return out, info, raw


def model_binaries(P, V, M, R, sep2, want_raw=False):
    """The definition over every pair i < j -> (the BIN_DTYPE list sorted by (i, j), the info dict[, the RAW_DTYPE records of
    the bound pairs in the order found])."""
    P, V, M, R = _state(P, V, M, R)
    n, sep2 = len(P), np.float64(sep2)
    X, Y, VX, VY = P[:, 0], P[:, 1], V[:, 0], V[:, 1]
    parts, near_n, coin_n = [], 0, 0
    chunk = max(1, CHUNK_BYTES // (8 * max(n, 1)))
    with np.errstate(all="ignore"):
        for a0 in range(0, n, chunk):
            a1 = min(a0 + chunk, n)
            lo = a0 + 1                                         # columns j > i >= a0
            if lo >= n:
                break
            upper = np.arange(lo, n)[None, :] > np.arange(a0, a1)[:, None]
            coincident, near, bound, flags, d2, v2, mu, hz = _define(
                X[None, lo:] - X[a0:a1, None], Y[None, lo:] - Y[a0:a1, None], VX[None, lo:] - VX[a0:a1, None],
                VY[None, lo:] - VY[a0:a1, None], M[a0:a1, None] + M[None, lo:], R[a0:a1, None] + R[None, lo:], sep2)
            near_n += int((near & upper).sum())
            coin_n += int((coincident & upper).sum())
            ii, jj = np.nonzero(bound & upper)
            parts.append((ii + a0, jj + lo, flags[ii, jj], d2[ii, jj], v2[ii, jj], mu[ii, jj], hz[ii, jj]))
    return _collect(n, parts, near_n, coin_n, sep2, want_raw)


def window_binaries(P, V, M, R, sep):
    """model_binaries at sep2 = sep * sep for finite states too large for an n x n matrix, and a finite sep: the bodies sorted
    by x, body a paired with its k-th successor for k = 1, 2, ... as long as any successor lies within sep (1 + 1e-6) in x (a
    near or coincident pair has |dx| <= sqrt(d2) <= sep up to rounding).  Every candidate goes through the definition's own
    float64 arithmetic, oriented i < j."""
    P, V, M, R = _state(P, V, M, R)
    n, sep = len(P), float(sep)
    sep2 = np.float64(sep * sep)
    assert np.isfinite(P).all() and np.isfinite(V).all() and np.isfinite(sep)
    order = np.argsort(P[:, 0], kind="stable")
    Xs = P[order, 0]
    reach = sep * (1.0 + 1e-6)
    parts, near_n, coin_n = [], 0, 0
    with np.errstate(all="ignore"):
        for k in range(1, n):
            cand = np.flatnonzero(Xs[k:] - Xs[:-k] <= reach)
            if cand.size == 0:
                break
            p, q = order[cand], order[cand + k]
            i, j = np.minimum(p, q), np.maximum(p, q)
            coincident, near, bound, flags, d2, v2, mu, hz = _define(P[j, 0] - P[i, 0], P[j, 1] - P[i, 1], V[j, 0] - V[i, 0],
                                                                     V[j, 1] - V[i, 1], M[i] + M[j], R[i] + R[j], sep2)
            near_n += int(near.sum())
            coin_n += int(coincident.sum())
            hit = np.flatnonzero(bound)
            parts.append((i[hit], j[hit], flags[hit], d2[hit], v2[hit], mu[hit], hz[hit]))
    return _collect(n, parts, near_n, coin_n, sep2, False)


def loop_binaries(P, V, M, R, sep2):
    """The definition and the finish as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation;
    math.sqrt is the C library's)."""
    P, V, M, R = _state(P, V, M, R)
    n, sep2 = len(P), float(sep2)
    X, Y, VX, VY, M, R = ([float(v) for v in col] for col in (P[:, 0], P[:, 1], V[:, 0], V[:, 1], M, R))
    inf = math.inf
    rows, near_n, coin_n = [], 0, 0
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy, dvx, dvy = X[j] - X[i], Y[j] - Y[i], VX[j] - VX[i], VY[j] - VY[i]
            d2 = (dx * dx) + (dy * dy)
            if d2 == 0.0:
                coin_n += 1
            if not (0.0 < d2 and d2 <= sep2):
                continue
            near_n += 1
            v2 = (dvx * dvx) + (dvy * dvy)
            mu = G2 * (M[i] + M[j])
            w = (v2 * v2) * d2
            k = mu * mu
            if not (0.0 < mu and k < inf and w < k):
                continue
            hz = (dx * dvy) - (dy * dvx)
            b = (dx * dvx) + (dy * dvy)
            s = R[i] + R[j]
            flags = (OVERLAP if d2 <= s * s else 0) | (APPROACHING if b < 0.0 else 0)
            r = math.sqrt(d2)
            gm = 0.5 * mu
            eps = (0.5 * v2) - (gm / r)
            a = gm / (-(eps + eps)) if eps < 0.0 else inf
            e2 = 1.0 + (((eps + eps) * (hz * hz)) / (gm * gm))
            ecc = math.sqrt(e2) if e2 > 0.0 else 0.0
            period = TWO_PI * math.sqrt(((a * a) * a) / gm) if a < inf else inf
            rows.append((a, ecc, period, r, i, j, flags))
    out = np.array(rows, dtype=BIN_DTYPE) if rows else np.zeros(0, dtype=BIN_DTYPE)
    return out, _info(n, out["flags"], near_n, coin_n, sep2)


def assert_same(got, want, what=""):
    """(list, info) against (list, info): a, ecc, period and sep by bits, i, j and flags exactly, every field of info (sep2 by
    bits)."""
    (gb, gi), (wb, wi) = got, want
    for f in COUNTS:
        assert int(gi[f]) == int(wi[f]), (what, f, gi[f], wi[f])
    assert np.float64(gi["sep2"]).view(np.uint64) == np.float64(wi["sep2"]).view(np.uint64), (what, "sep2")
    assert len(gb) == len(wb) == int(wi["pairs"]), (what, len(gb), len(wb), wi["pairs"])
    for f in ("i", "j", "flags"):
        bad = np.flatnonzero(np.asarray(gb[f]) != np.asarray(wb[f]))
        assert bad.size == 0, (what, f, "%d records differ, first at %d" % (bad.size, bad[0]), gb[bad[:3]], wb[bad[:3]])
    for f in ORBIT:
        g, w = (np.ascontiguousarray(e[f], dtype=np.float64).view(np.uint64) for e in (gb, wb))
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, f, "%d records differ, first at %d" % (bad.size, bad[0]), gb[bad[:3]], wb[bad[:3]])


def reversed_back(lst, n):
    """A list taken on the state with the body order reversed, mapped back to the original indices and sorted again."""
    i, j = n - 1 - lst["j"].astype(np.int64), n - 1 - lst["i"].astype(np.int64)
    return _sorted(i, j, lst["flags"], [lst[f] for f in ORBIT])
