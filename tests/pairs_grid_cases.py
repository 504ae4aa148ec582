"""The numpy model of the pair counts and the bound pairs on the cell list (nbody_get_pair_counts_grid,
nbody_get_binaries_grid and their batch forms; include/nbody.h), the check of their window rule, and the states,
grids and values their tests share.

The definition is the plain one on a subset: inside_of of the groups on the cell list (cell_cases.cell_index >= 0) picks the
sources, pair_cases.model_pair_counts / binary_cases.model_binaries run on exactly those bodies in their order, and the binaries'
indices are mapped back to the state's.  Integers, and a list sorted by (i, j) whose orbit values come from the same fp64
operations whatever the visiting order: the GPU tests compare with zero tolerance.

window_holds restates what the device relies on (csrc/nbody_pairs_grid.hpp): the fixed-radius window of the radius queries
(within_cases.window_model) with h2 = the top edge, or sep2, holds every inside source that a row counts or finds near."""
import functools

import numpy as np

import binary_cases as bc
import groups_grid_cases as gg
import pair_cases as pc
import within_cases as wc

PAIR_INFO_DTYPE = np.dtype(pc.INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])
BINARY_INFO_DTYPE = np.dtype(bc.INFO_DTYPE.descr + [("inside", np.int64), ("outside", np.int64)])
INF = float("inf")

EDGES2 = np.array([0.0, 4.0, 25.0, 100.0, 225.0])              # the standard state's: the top edge is SEP squared
SEP = bc.SEP
SEP2 = SEP * SEP
BODY_COUNTS = wc.BODY_COUNTS                                    # (1, 2, 63, 64, 65, 255, 256, 257, 300, 385)
GRID_SHAPES = wc.GRID_SHAPES
DTYPES = wc.DTYPES
BATCH_COUNTS = (0, 1, 300, 385)
BATCH_CAP = 385


def inside_of(P, grid):
    return gg.inside_of(P, grid)


def model_pair_counts_grid(P, grid, edges2, points=None):
    """pair_cases.model_pair_counts on the inside bodies -> its dict with n_bodies = n, "inside" and "outside"."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    inside = inside_of(P, grid)
    out = pc.model_pair_counts(P[inside], edges2, points)
    k = int(inside.sum())
    out.update(n_bodies=len(P), inside=k, outside=len(P) - k)
    return out


def model_binaries_grid(P, V, M, R, grid, sep2):
    """binary_cases.model_binaries on the inside bodies, the indices mapped back -> (list, info with n_bodies = n, "inside",
    "outside").  The inside bodies keep their order, so the list stays sorted by (i, j)."""
    P, V, M, R = bc._state(P, V, M, R)
    idx = np.flatnonzero(inside_of(P, grid))
    lst, info = bc.model_binaries(P[idx], V[idx], M[idx], R[idx], sep2)
    lst = lst.copy()
    lst["i"], lst["j"] = idx[lst["i"]], idx[lst["j"]]
    info.update(n_bodies=len(P), inside=len(idx), outside=len(P) - len(idx))
    return lst, info


def loop_pair_counts_grid(P, grid, edges2, points=None):
    """The definition as a plain double loop over every pair of the WHOLE state, the inside test per pair."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    e2 = [float(v) for v in np.asarray(edges2, dtype=np.float64)]
    B, n = len(e2) - 1, len(P)
    inside = inside_of(P, grid)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    rows = [(X[i], Y[i], i + 1) for i in range(n) if inside[i]] if points is None else \
        [(float(q[0]), float(q[1]), 0) for q in np.asarray(points, dtype=np.float64).reshape(-1, 2)]
    counts, below, pairs = [0] * B, 0, 0
    for x, y, start in rows:
        for j in range(start, n):
            if not inside[j]:
                continue
            pairs += 1
            dx, dy = X[j] - x, Y[j] - y
            try:
                d2 = (dx * dx) + (dy * dy)
            except OverflowError:
                d2 = INF
            below += d2 < e2[0]
            for k in range(B):
                counts[k] += e2[k] <= d2 and d2 < e2[k + 1]
    k = int(inside.sum())
    out = pc._result(counts, below, pairs, n, np.asarray(e2))
    out.update(inside=k, outside=n - k)
    return out


def loop_binaries_grid(P, V, M, R, grid, sep2):
    """binary_cases.loop_binaries over the whole state, then every pair with an outside end removed - the definition read the
    other way round: near, coincident and the flags' counts are recounted from the pairs that stay."""
    P, V, M, R = bc._state(P, V, M, R)
    inside = inside_of(P, grid)
    n = len(P)
    Pm = P.copy()
    Pm[~inside] = np.nan                                         # a NaN position is in no pair of the plain definition
    lst, info = bc.loop_binaries(Pm, V, M, R, sep2)
    info.update(n_bodies=n, inside=int(inside.sum()), outside=n - int(inside.sum()))
    return lst, info


def pair_assert_same(got, want, what=""):
    pc.assert_same(got, want, what)
    if "inside" in got and "inside" in want:
        assert (got["inside"], got["outside"]) == (want["inside"], want["outside"]), (what, got["inside"], want["inside"])


def binary_assert_same(got, want, what=""):
    bc.assert_same(got, want, what)
    if "inside" in got[1] and "inside" in want[1]:
        assert (got[1]["inside"], got[1]["outside"]) == (want[1]["inside"], want[1]["outside"]), what


def window_holds(P, grid, h2, rows_xy=None, strict=False):
    """Every inside source with d2 <= h2 (strict: d2 < h2) of a row lies in that row's window of within_cases.window_model
    -> the number of such (row, source) pairs.  rows_xy=None: the inside bodies themselves (a pair from both ends)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    inside = inside_of(P, grid)
    rows = P[inside] if rows_xy is None else np.asarray(rows_xy, dtype=np.float64).reshape(-1, 2)
    if len(rows) == 0 or len(P) == 0:
        return 0
    seen = wc.window_model(P, grid, h2, rows)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = P[None, :, 0] - rows[:, None, 0], P[None, :, 1] - rows[:, None, 1]
        d2 = (dx * dx) + (dy * dy)
        need = ((d2 < h2) if strict else (d2 <= h2)) & inside[None, :]
    assert not (need & ~seen).any(), ("a needed source outside its row's window", np.argwhere(need & ~seen)[:4])
    return int(need.sum())


# ---------------------------------------------------------------------------------------------------------------------
# the shared states and grids
# ---------------------------------------------------------------------------------------------------------------------
def half_of(n):
    return 7.0 * np.sqrt(n)                                      # the half-width of binary_cases.standard_state


def standard_grids(n):
    """The three grids of the edge cases: 8 x 8 over the bounding square, 1 x 1, and 8 x 8 over |x| < half / 2,
    y > -half / 2, which leaves bodies outside -> [(nx, ny, bounds)]."""
    h = float(half_of(n))
    return [(8, 8, (-h, h, -h, h)), (1, 1, (-h, h, -h, h)), (8, 8, (-0.5 * h, 0.5 * h, -0.5 * h, h))]


@functools.lru_cache(maxsize=None)
def standard(n, tag):
    """binary_cases.standard_state(n, dtype), read-only."""
    S = bc.standard_state(n, DTYPES[tag])
    for a in S:
        a.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def shapes_state(tag):
    """within_cases.state(300, dtype, coincident=True) with the standard state's velocities and masses -> (P, V, M, R, field):
    body 7 sits on body 200."""
    P, R, f = wc.state(300, DTYPES[tag], coincident=True)
    _, V, M, _ = bc.standard_state(300, DTYPES[tag])
    for a in (P, V, M, R):
        a.setflags(write=False)
    return P, V, M, R, f


def lattice_state():
    """The 17 x 17 lattice with spacing 1 (289 bodies), at rest with equal masses (2^40: exact in fp32): every near pair is
    bound."""
    L, LR = wc.nc.lattice(wc.LATTICE_SIDE)
    n = len(LR)
    return L, np.zeros((n, 2)), np.full(n, 2.0 ** 40), LR


def lattice_grids():
    s = float(wc.LATTICE_SIDE)
    return [(wc.LATTICE_SIDE, wc.LATTICE_SIDE, (-o, s - o, -o, s - o)) for o in (0.0, 0.1)]


LATTICE_TIES = 2 * wc.LATTICE_SIDE * (wc.LATTICE_SIDE - 1)      # 544 pairs at d2 == 1


def one_cell_state(tag):
    """385 bodies inside cell (2, 2) of the 8 x 8 grid over [0, 8)^2, with the standard velocities and masses."""
    Q, QR = wc.one_cell_state(385, DTYPES[tag])
    _, V, M, _ = bc.standard_state(385, DTYPES[tag])
    return Q, V, M, QR


def batch_states():
    """Four systems - none, one body, 300 and 385 - of the standard states (fp32: a batch is)."""
    return [tuple(a[:n] for a in bc.standard_state(max(n, 1), np.float32)) if n else
            (np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.zeros(0)) for n in BATCH_COUNTS]


def batch_grids():
    """One grid that holds every body of the four systems and one that does not."""
    h = float(half_of(385))
    return [(8, 8, (-h, h, -h, h)), (6, 5, (-0.5 * h, 0.4 * h, -0.3 * h, h))]


def bins_edges(bins, top=SEP2):
    """bins + 1 squared edges from 0 up to `top`, evenly spaced in d2 (top = inf: the last edge alone is +inf)."""
    if np.isinf(top):
        return np.concatenate([np.linspace(0.0, SEP2, bins), [INF]]) if bins > 1 else np.array([0.0, INF])
    return np.linspace(0.0, top, bins + 1)
