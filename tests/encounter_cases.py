"""The numpy model of the encounter query (nbody_get_encounters, nbody_batch_get_encounters, nbody_encounter_finish;
include/nbody.h) and the states its tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic,
its sqrt and its division are correctly rounded - so the model restates it bit for bit and the GPU tests compare with zero
tolerance.  A pair i < j of bodies (X, Y, R) with velocities (VX, VY), an fp32 state widened exactly, a horizon h >= 0:
    dx = X_j - X_i;  dy = Y_j - Y_i;  dvx = VX_j - VX_i;  dvy = VY_j - VY_i
    d2 = (dx*dx) + (dy*dy);   s = R_i + R_j;   s2 = s*s;   c = d2 - s2
    b  = (dx*dvx) + (dy*dvy); a = (dvx*dvx) + (dvy*dvy);   disc = (b*b) - (a*c)
    ex = dx + (dvx*h);        ey = dy + (dvy*h);            e2 = (ex*ex) + (ey*ey)
    now = d2 <= s2;  end = e2 <= s2;  mid = b < 0 and (-b) < (a*h) and disc >= 0;  swept = now or end or mid
    t = +0 if now else (min(c / (sqrt(disc) - b), h) if b < 0 and disc >= 0 else h)          min(x, h) = x if x < h else h
flags: NOW = 1 where now, END = 2 where end; a swept pair with neither is missed.  The list is sorted by (t, i, j)."""
import math

import numpy as np

NOW, END = 1, 2
ENC_DTYPE = np.dtype([("t", np.float64), ("i", np.int32), ("j", np.int32), ("flags", np.uint32)])
RECORD_DTYPE = np.dtype([("t", np.float64), ("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32)])
RAW_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("flags", np.uint32), ("reserved", np.uint32), ("c", np.float64),
                      ("b", np.float64), ("disc", np.float64)])
INFO_DTYPE = np.dtype([("n_bodies", np.int64), ("pairs", np.int64), ("now", np.int64), ("end", np.int64), ("missed", np.int64),
                       ("horizon", np.float64)])
COUNTS = ("n_bodies", "pairs", "now", "end", "missed")
CHUNK_BYTES = 16 << 20                                          # of one n-wide float64 temporary of the model
H = 0.5                                                         # the horizon of the standard state
STANDARD_N = (63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1500)
DTYPE_OF = {0: np.float32, 1: np.float64}


def widen(bodies):
    """(P (n, 2), V (n, 2), R (n,)) of a BodiesData as float64 (exact)."""
    n = bodies.numBodies
    return (np.asarray(bodies.Positions[:n], dtype=np.float64).reshape(n, 2), np.asarray(bodies.Velocities[:n], dtype=np.float64).reshape(n, 2),
            np.asarray(bodies.Radii[:n], dtype=np.float64).reshape(n))


def standard_state(n, dtype, seed=None):
    """Positions uniform in +-7 sqrt(n), velocities uniform in +-40, radii uniform in [0.5, 2.5], drawn in that order from
    default_rng(n), each cast to `dtype` and widened back: about 0.4 n swept pairs at h = 0.5."""
    rng = np.random.default_rng(n if seed is None else seed)
    half = 7.0 * np.sqrt(n)
    P = rng.uniform(-half, half, size=(n, 2)).astype(dtype).astype(np.float64)
    V = rng.uniform(-40.0, 40.0, size=(n, 2)).astype(dtype).astype(np.float64)
    R = rng.uniform(0.5, 2.5, size=n).astype(dtype).astype(np.float64)
    return P, V, R


def _info(n, flags, h):
    flags = np.asarray(flags, dtype=np.uint32)
    return {"n_bodies": int(n), "pairs": int(len(flags)), "now": int(((flags & NOW) != 0).sum()), "end": int(((flags & END) != 0).sum()),
            "missed": int((flags == 0).sum()), "horizon": float(h)}


def _time(flags, c, b, disc, h):
    """t of swept pairs from their raw values: what nbody_encounter_finish computes."""
    with np.errstate(all="ignore"):
        x = c / (np.sqrt(disc) - b)
        x = np.where(x < h, x, h)
        t = np.where((b < 0.0) & (disc >= 0.0), x, h)
    return np.where((flags & NOW) != 0, 0.0, t)


def _sorted(t, i, j, flags):
    order = np.lexsort((j, i, t))
    out = np.zeros(len(order), dtype=ENC_DTYPE)
    out["t"], out["i"], out["j"], out["flags"] = t[order], i[order], j[order], flags[order]
    return out


def model_encounters(P, V, R, h, want_raw=False):
    """The definition over every pair i < j -> (the ENC_DTYPE list sorted by (t, i, j), the info dict[, the RAW_DTYPE records
    of the swept pairs in (i, j) order])."""
    P, V = (np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in (P, V))
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    n, h = len(P), np.float64(h)
    X, Y, VX, VY = P[:, 0], P[:, 1], V[:, 0], V[:, 1]
    parts = []
    chunk = max(1, CHUNK_BYTES // (8 * max(n, 1)))
    with np.errstate(all="ignore"):
        for a0 in range(0, n, chunk):
            a1 = min(a0 + chunk, n)
            lo = a0 + 1                                         # columns j > i >= a0
            if lo >= n:
                break
            dx = X[None, lo:] - X[a0:a1, None]
            dy = Y[None, lo:] - Y[a0:a1, None]
            dvx = VX[None, lo:] - VX[a0:a1, None]
            dvy = VY[None, lo:] - VY[a0:a1, None]
            d2 = (dx * dx) + (dy * dy)
            s = R[a0:a1, None] + R[None, lo:]
            s2 = s * s
            c = d2 - s2
            b = (dx * dvx) + (dy * dvy)
            a = (dvx * dvx) + (dvy * dvy)
            disc = (b * b) - (a * c)
            ex = dx + (dvx * h)
            ey = dy + (dvy * h)
            e2 = (ex * ex) + (ey * ey)
            now = d2 <= s2
            end = e2 <= s2
            mid = (b < 0.0) & ((-b) < (a * h)) & (disc >= 0.0)
            upper = np.arange(lo, n)[None, :] > np.arange(a0, a1)[:, None]
            ii, jj = np.nonzero((now | end | mid) & upper)
            flags = now[ii, jj].astype(np.uint32) * NOW + end[ii, jj].astype(np.uint32) * END
            parts.append((ii + a0, jj + lo, flags, c[ii, jj], b[ii, jj], disc[ii, jj]))
    if parts:
        i, j, flags, c, b, disc = (np.concatenate([p[k] for p in parts]) for k in range(6))
    else:
        i = j = np.zeros(0, dtype=np.int64)
        flags = np.zeros(0, dtype=np.uint32)
        c = b = disc = np.zeros(0)
    enc = _sorted(_time(flags, c, b, disc, h), i, j, flags)
    info = _info(n, flags, h)
    if not want_raw:
        return enc, info
    raw = np.zeros(len(i), dtype=RAW_DTYPE)
    raw["i"], raw["j"], raw["flags"], raw["c"], raw["b"], raw["disc"] = i, j, flags, c, b, disc
    return enc, info, raw


def window_encounters(P, V, R, h):
    """model_encounters for finite states too large for an n x n matrix, and a finite h: the bodies sorted by x, body a paired
    with its k-th successor for k = 1, 2, ... as long as any successor lies within reach in x.  A pair is swept only if the
    centres come within s at some time in [0, h], and then |dx| <= s + |dvx| h: reach = (2 max R + 2 max |VX| h) (1 + 1e-6)
    leaves out no swept pair.  Every candidate goes through the definition's own float64 arithmetic, oriented i < j."""
    P, V = (np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in (P, V))
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    n, h = len(P), np.float64(h)
    assert np.isfinite(P).all() and np.isfinite(V).all() and np.isfinite(R).all() and np.isfinite(h)
    order = np.argsort(P[:, 0], kind="stable")
    Xs = P[order, 0]
    reach = (2.0 * R.max() + 2.0 * np.abs(V[:, 0]).max() * h) * (1.0 + 1e-6) if n else 0.0
    parts = []
    for k in range(1, n):
        near = np.flatnonzero(Xs[k:] - Xs[:-k] <= reach)
        if near.size == 0:
            break
        p, q = order[near], order[near + k]
        i, j = np.minimum(p, q), np.maximum(p, q)
        dx, dy = P[j, 0] - P[i, 0], P[j, 1] - P[i, 1]
        dvx, dvy = V[j, 0] - V[i, 0], V[j, 1] - V[i, 1]
        d2 = (dx * dx) + (dy * dy)
        sr = R[i] + R[j]
        s2 = sr * sr
        c = d2 - s2
        b = (dx * dvx) + (dy * dvy)
        a = (dvx * dvx) + (dvy * dvy)
        disc = (b * b) - (a * c)
        ex = dx + (dvx * h)
        ey = dy + (dvy * h)
        e2 = (ex * ex) + (ey * ey)
        now, end = d2 <= s2, e2 <= s2
        mid = (b < 0.0) & ((-b) < (a * h)) & (disc >= 0.0)
        hit = np.flatnonzero(now | end | mid)
        flags = now[hit].astype(np.uint32) * NOW + end[hit].astype(np.uint32) * END
        parts.append((i[hit], j[hit], flags, c[hit], b[hit], disc[hit]))
    if parts:
        i, j, flags, c, b, disc = (np.concatenate([p[k] for p in parts]) for k in range(6))
    else:
        i = j = np.zeros(0, dtype=np.int64)
        flags = np.zeros(0, dtype=np.uint32)
        c = b = disc = np.zeros(0)
    return _sorted(_time(flags, c, b, disc, h), i, j, flags), _info(n, flags, h)


def loop_encounters(P, V, R, h):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation; math.sqrt is the C
    library's)."""
    P, V = (np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in (P, V))
    n, h = len(P), float(h)
    X, Y, VX, VY = ([float(v) for v in col] for col in (P[:, 0], P[:, 1], V[:, 0], V[:, 1]))
    R = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)]
    rows = []
    for i in range(n):
        for j in range(i + 1, n):
            dx, dy, dvx, dvy = X[j] - X[i], Y[j] - Y[i], VX[j] - VX[i], VY[j] - VY[i]
            d2 = (dx * dx) + (dy * dy)
            s = R[i] + R[j]
            s2 = s * s
            c = d2 - s2
            b = (dx * dvx) + (dy * dvy)
            a = (dvx * dvx) + (dvy * dvy)
            disc = (b * b) - (a * c)
            ex = dx + (dvx * h)
            ey = dy + (dvy * h)
            e2 = (ex * ex) + (ey * ey)
            now, end = d2 <= s2, e2 <= s2
            mid = b < 0.0 and (-b) < (a * h) and disc >= 0.0
            if not (now or end or mid):
                continue
            if now:
                t = 0.0
            elif b < 0.0 and disc >= 0.0:
                x = c / (math.sqrt(disc) - b)
                t = x if x < h else h
            else:
                t = h
            rows.append((t, i, j, (NOW if now else 0) | (END if end else 0)))
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    enc = np.array(rows, dtype=ENC_DTYPE) if rows else np.zeros(0, dtype=ENC_DTYPE)
    return enc, _info(n, enc["flags"], h)


def first_contacts(enc, n):
    """Per body: the earliest t (+inf: none), its partner (-1; ties go to the earlier record) and the number of encounters."""
    t = np.full(n, np.inf)
    partner = np.full(n, -1, dtype=np.int32)
    count = np.zeros(n, dtype=np.int64)
    for k in range(len(enc)):
        for a, b in ((int(enc["i"][k]), int(enc["j"][k])), (int(enc["j"][k]), int(enc["i"][k]))):
            count[a] += 1
            if partner[a] < 0:                                  # the list is sorted by t: the first record is the earliest
                t[a], partner[a] = enc["t"][k], b
    return {"t": t, "partner": partner, "count": count}


def assert_same(got, want, what=""):
    """(list, info) against (list, info): t by bits, i, j and flags exactly, every field of info (the horizon by bits)."""
    (ge, gi), (we, wi) = got, want
    for f in COUNTS:
        assert int(gi[f]) == int(wi[f]), (what, f, gi[f], wi[f])
    assert np.float64(gi["horizon"]).view(np.uint64) == np.float64(wi["horizon"]).view(np.uint64), (what, "horizon")
    assert len(ge) == len(we) == int(wi["pairs"]), (what, len(ge), len(we), wi["pairs"])
    for f in ("i", "j", "flags"):
        bad = np.flatnonzero(np.asarray(ge[f]) != np.asarray(we[f]))
        assert bad.size == 0, (what, f, "%d records differ, first at %d" % (bad.size, bad[0]), ge[bad[:3]], we[bad[:3]])
    gt, wt = (np.ascontiguousarray(e["t"], dtype=np.float64).view(np.uint64) for e in (ge, we))
    bad = np.flatnonzero(gt != wt)
    assert bad.size == 0, (what, "t", "%d records differ, first at %d" % (bad.size, bad[0]), ge[bad[:3]], we[bad[:3]])


def classes(info_or_enc):
    """(now, end without now, missed) of a list."""
    f = np.asarray(info_or_enc["flags"])
    return int(((f & NOW) != 0).sum()), int((f == END).sum()), int((f == 0).sum())


def reversed_back(enc, n):
    """A list taken on the state with the body order reversed, mapped back to the original indices and sorted again."""
    i, j = n - 1 - enc["j"].astype(np.int64), n - 1 - enc["i"].astype(np.int64)
    return _sorted(enc["t"], i, j, enc["flags"])
