"""The numpy model of the groups on the cell list (nbody_get_groups_grid, nbody_batch_get_groups_grid; include/nbody.h,
DESIGN.md 4.22), the model of their window rule, and the states, grids and links their tests share.

The definition is group_cases.adjacency - IEEE fp64, every operation rounded on its own, no fma - restricted to pairs whose
bodies are both inside the grid (cell_cases.cell_index >= 0); a label is the lowest index of its connected component.  An
integer function of the set of links: the GPU tests compare with zero tolerance.

window_holds restates the rule by which the device picks the cells a row looks at (csrc/nbody_groups_grid.hpp): row i, with
a = |R_i|, S_i = (radius_scale * (a + a)) + link and h2_i = S_i * S_i, looks at within_cases._span(t, S_i * sx, nx) per axis
and filters with d2 <= h2_i.  A link has to be seen from one end only: the end with the larger |radius|, both on a tie."""
import functools

import numpy as np

import cell_cases as cc
import group_cases as gc
import neighbor_cases as nc
import within_cases as wc

INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32),
                       ("inside", np.int32), ("outside", np.int32)])


def inside_of(P, grid):
    return cc.cell_index(P, grid) >= 0


def adjacency_grid(P, R, grid, link, radius_scale):
    """group_cases.adjacency masked by `inside` on both ends."""
    inside = inside_of(P, grid)
    return gc.adjacency(P, R, link, radius_scale) & inside[:, None] & inside[None, :]


def model_groups_grid(P, R, grid, link, radius_scale=1.0):
    """-> {"label": int32 (n,), "n_groups", "largest", "inside", "outside"}: the definition over the bodies P (n, 2), R (n,),
    float64 (an fp32 state widened exactly)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    label = gc.labels_of(adjacency_grid(P, R, grid, link, radius_scale)) if len(P) else np.zeros(0, dtype=np.int32)
    n_groups, largest = gc.summary(label)
    inside = int(inside_of(P, grid).sum())
    return {"label": label, "n_groups": n_groups, "largest": largest, "inside": inside, "outside": len(P) - inside}


def assert_same(got, want, what=""):
    """Zero tolerance: every label, the two counts that follow from them, and inside / outside where both sides have them."""
    gc.assert_same(got, want, what)
    if "inside" in got and "inside" in want:
        assert (got["inside"], got["outside"]) == (want["inside"], want["outside"]), what


def window_holds(P, R, grid, link, radius_scale=1.0):
    """For every linked inside pair (i, j) with |R_j| <= |R_i|: j's cell lies in row i's window and d2 <= h2_i, so the walk of
    row i tests the exact predicate on j.  Every link has such an end; on a tie both ends are held to it.  -> the number of
    links (unordered pairs)."""
    x0, y0, sx, sy, nx, ny = cc.grid_tuple(grid)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    link, radius_scale = np.float64(link), np.float64(radius_scale)
    if len(P) == 0:
        return 0
    fine = not (sx <= 2.0 ** 400 and sy <= 2.0 ** 400)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.abs(R)
        S = (radius_scale * (a + a)) + link                     # per row
        h2 = S * S
        wx0, wy0 = (np.full(len(S), np.inf),) * 2 if fine else (S * sx, S * sy)
        tx, ty = (P[:, 0] - x0) * sx, (P[:, 1] - y0) * sy
        dx = P[None, :, 0] - P[:, None, 0]
        dy = P[None, :, 1] - P[:, None, 1]
        d2 = (dx * dx) + (dy * dy)
        smaller = a[None, :] <= a[:, None]                      # [i, j]: |R_j| <= |R_i|; False with a NaN
    c0, c1 = wc._span(tx, wx0, nx)
    r0, r1 = wc._span(ty, wy0, ny)
    cell = cc.cell_index(P, grid)
    ix, iy = cell % nx, cell // nx
    walks = ~np.isnan(S)                                        # a row with a NaN S leaves at once
    seen = (walks[:, None] & (cell >= 0)[None, :] & (c0[:, None] <= ix[None, :]) & (ix[None, :] <= c1[:, None])
            & (r0[:, None] <= iy[None, :]) & (iy[None, :] <= r1[:, None]) & (d2 <= h2[:, None]))
    A = adjacency_grid(P, R, grid, link, radius_scale)
    need = A & smaller
    missed = np.argwhere(need & ~seen)
    assert len(missed) == 0, ("%d links not seen from their larger end, first %s" % (len(missed), missed[0]))
    assert not (A & ~need & ~need.T).any()                      # every link has an end that must see it
    return int(A.sum()) // 2


def tightest_apart(P, R, link, radius_scale, i, j):
    """The largest link below `link` at which bodies i and j are not linked any more: the doubles below `link` one after the
    other (the sum that forms s can round back up, so it need not be the very next one) -> (that link, the doubles it took)."""
    below, steps = np.float64(link), 0
    while gc.adjacency(P[[i, j]], R[[i, j]], below, radius_scale)[0, 1]:
        below, steps = np.nextafter(below, 0.0), steps + 1
    return float(below), steps


# ---------------------------------------------------------------------------------------------------------------------
# the shared cases: a state, and the (nx, ny, bounds, link, radius_scale) it is asked on
# ---------------------------------------------------------------------------------------------------------------------
EDGE_LINK = 1.5                                                 # on within_cases.state: groups from 1 to some tens of bodies
CHAIN_N = 300
ONE_CELL_LINK = 0.004
SMALL_R, BIG_R, PAIR_R = 0.01, 6.0, 1.5
BATCH_COUNTS = (0, 1, 300, 257)
BATCH_CAP = 300
BATCH_LINK = 0.5


class Case:
    """name; dtype; P (n, 2) and R (n,) float64, exact in dtype; asks = [(nx, ny, bounds, link, radius_scale), ...]."""

    def __init__(self, name, dtype, P, R, asks):
        self.name, self.dtype, self.P, self.R, self.asks = name, dtype, P, R, asks
        for a in (P, R):
            a.setflags(write=False)

    def grid(self, ask):
        return cc.grid_of(*ask[:3])


def chain_links(dtype):
    """shuffled_chain: spacing 1, radius 0.25, so link = spacing - 2 * radius = 0.5 gives s = 1 = d exactly -> (0.5, the
    largest link below it at which neighbours are apart)."""
    P, R = gc.shuffled_chain(CHAIN_N)
    order = np.argsort(P[:, 0])
    apart, steps = tightest_apart(P, R, 0.5, 1.0, order[0], order[1])
    assert 1 <= steps <= 2                                      # 0.5 + (0.5 - 2^-54) rounds to 1: the second double below
    return 0.5, apart


def asymmetric_state(dtype, big_first, negative=False, nan=False):
    """200 small bodies (r = 0.01) over [0, 20)^2, cells 1 wide; one body of r = 6 at (10.5, 10.5), at index 0 or at the
    highest index of those, whose disc reaches bodies five cells away; two equal bodies of r = 1.5 that touch each other
    across three cells; negative: one more body with r = -6, whose s*s is as large as the big body's; nan: a last body with a
    NaN radius in the middle of the big body's disc."""
    rng = np.random.default_rng(977)
    P = rng.uniform(0.0, 20.0, size=(200, 2))
    R = np.full(200, SMALL_R)
    pair = np.array([[2.2, 17.5], [5.1, 17.5]])
    big = np.array([[10.5, 10.5]])
    P = np.concatenate([big, P, pair] if big_first else [P, pair, big])
    R = np.concatenate([[BIG_R], R, [PAIR_R] * 2] if big_first else [R, [PAIR_R] * 2, [BIG_R]])
    if negative:
        P, R = np.concatenate([P, [[4.5, 5.5]]]), np.concatenate([R, [-BIG_R]])
    if nan:
        P, R = np.concatenate([P, [[10.25, 10.75]]]), np.concatenate([R, [np.nan]])
    return P.astype(dtype).astype(np.float64), R.astype(dtype).astype(np.float64)


def batch_states():
    """The systems of the batch test, fp32: none, one body, the shuffled chain (a label travels far: many sweeps) and a
    random state (a few)."""
    out = []
    for s, n in enumerate(BATCH_COUNTS):
        if n == CHAIN_N:
            out.append(gc.shuffled_chain(CHAIN_N))
        else:
            out.append(nc.random_state(n, np.float32, 60 + s, field=80.0))
    return out


BATCH_GRIDS = ((32, 8, (0.0, 300.0, 0.0, 81.0)), (16, 4, (20.0, 120.0, 0.0, 40.0)))    # holds every body; leaves some outside


@functools.lru_cache(maxsize=None)
def cases():
    """Every constructed case of the GPU tests, by name.  Shared, never written to."""
    out = []
    for tag, dtype in wc.DTYPES.items():
        for n in wc.BODY_COUNTS:                                # workgroup and wave edges
            P, R, f = wc.state(n, dtype)
            out.append(Case("bodies-%d-%s" % (n, tag), dtype, P, R,
                            [(8, 8, (0, f, 0, f), EDGE_LINK, 1.0), (1, 1, (0, f, 0, f), EDGE_LINK, 1.0),
                             (8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f), EDGE_LINK, 1.0)]))
        P, R, f = wc.state(300, dtype, coincident=True)
        out.append(Case("shapes-%s" % tag, dtype, P, R, [(nx, ny, (0, f, 0, f), EDGE_LINK, 1.0) for nx, ny in wc.GRID_SHAPES]))
        C, CR = gc.shuffled_chain(CHAIN_N)                      # cell side = spacing on 300 x 1: every body on a boundary
        out.append(Case("chain-%s" % tag, dtype, C, CR,
                        [(nx, 1, (0.0, float(CHAIN_N), 0.0, 6.0), link, 1.0) for nx in (64, CHAIN_N) for link in chain_links(dtype)]))
        L, LR = nc.lattice(wc.LATTICE_SIDE)                     # spacing = cell side = link, centres only: d2 == s*s across
        s = float(wc.LATTICE_SIDE)                              # a cell boundary, at offsets 0 and a tenth of a cell
        out.append(Case("lattice-%s" % tag, dtype, L, LR,
                        [(wc.LATTICE_SIDE, wc.LATTICE_SIDE, (-o, s - o, -o, s - o), link, 0.0)
                         for o in (0.0, 0.1) for link in (1.0, float(np.nextafter(1.0, 0.0)))]))
        for big_first in (True, False):
            for extra in ("", "negative", "nan"):
                A, AR = asymmetric_state(dtype, big_first, extra == "negative", extra == "nan")
                name = "asymmetric-%s%s-%s" % ("first" if big_first else "last", "-" + extra if extra else "", tag)
                out.append(Case(name, dtype, A, AR, [(20, 20, (0, 20, 0, 20), 0.0, 1.0)]))
        Q, QR = wc.one_cell_state(385, dtype)
        out.append(Case("one-cell-%s" % tag, dtype, Q, QR, [(8, 8, (0, 8, 0, 8), ONE_CELL_LINK, 1.0), (3, 3, (0, 8, 0, 8), np.inf, 1.0)]))
    for s, (P, R) in enumerate(batch_states()):
        out.append(Case("batch-%d" % s, np.float32, P, R, [g + (BATCH_LINK, 1.0) for g in BATCH_GRIDS]))
    return {c.name: c for c in out}


def case_names(prefix=""):
    return [k for k in cases() if k.startswith(prefix)]
