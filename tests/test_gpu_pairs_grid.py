"""Pair counts and bound pairs on the cell list (nbody_get_pair_counts_grid, nbody_get_binaries_grid and their batch forms;
pair_counts(grid=...) and binaries(grid=...) of Stepper, StepperGroup and StepperBatch) on the MI355X.

The counts are integers and the list is sorted by (i, j) on the host from values that do not depend on the visiting order: zero
tolerance throughout - against the numpy model of pairs_grid_cases.py (the plain models on the inside bodies) and product
against product (the plain calls, another grid, a Stepper holding only the inside bodies, a batch against a Stepper, another
rank).  test_pairs_grid_cases_cpu.py holds, for every constructed case used here, that every counted or near pair lies inside
its row's window; the tests on stepped states hold it on the downloaded state before they ask."""
import numpy as np
import pytest

import binary_cases as bc
import cell_cases as cc
import groups_grid_cases as gg
import knn_grid_cases as kg
import neighbor_cases as nc
import pair_cases as pc
import pairs_grid_cases as pg
import sharded_cases as sc
import within_cases as wc
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
INF = float("inf")
PREC = {"f32": 0, "f64": 1}
TAGS = tuple(PREC)


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=1000000,
                      fieldHeight=1000000)


def bodies_of(nb, P, V, M, R, precision):
    return nb.BodiesData.from_arrays(P, V, M, R, precision) if len(R) else nb.BodiesData(0, precision)


def pair_bytes(r):
    return (r["counts"].tobytes(), r["below"], r["rest"], r["pairs"])


def binary_bytes(r):
    lst, info = r
    return (lst.tobytes(), tuple(info[f] for f in bc.COUNTS[1:]))


def ask_pairs(st, P, grid, edges2, points=None, what=""):
    got = st.pair_counts(edges2, points, squared=True, grid=grid)
    want = pg.model_pair_counts_grid(P, got["grid"], edges2, points)
    print("%s pairs: inside %d, below %d, counts sum %d, rest %d" % (what, got["inside"], got["below"], int(got["counts"].sum()),
                                                                    got["rest"]))
    pg.pair_assert_same(got, want, what)
    pc.check_sum(got, want["pairs"], what)
    return got


def ask_binaries(st, S, grid, sep2, what="", cap=None):
    got = st.binaries(sep2, squared=True, grid=grid, cap=cap)
    want = pg.model_binaries_grid(*S, got[1]["grid"], sep2)
    print("%s binaries: %s" % (what, {k: v for k, v in got[1].items() if k != "grid"}))
    pg.binary_assert_same(got, want, what)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. workgroup and wave edges: 8 x 8, 1 x 1 and a grid that leaves bodies outside
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", pg.BODY_COUNTS)
def test_body_edges(nb, n, tag):
    S = pg.standard(n, tag)
    P = S[0]
    grids = [nb.make_grid(*a) for a in pg.standard_grids(n)]
    with small_stepper(nb, PREC[tag], n) as st, small_stepper(nb, PREC[tag], n) as sub:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        pairs = [ask_pairs(st, P, g, pg.EDGES2, what="n %d grid %d" % (n, k)) for k, g in enumerate(grids)]
        bins = [ask_binaries(st, S, g, pg.SEP2, what="n %d grid %d" % (n, k)) for k, g in enumerate(grids)]
        plain_p, plain_b = st.pair_counts(pg.EDGES2, squared=True), st.binaries(pg.SEP)
        assert pairs[0]["outside"] == 0 == pairs[1]["outside"] and bins[0][1]["inside"] == n
        assert pair_bytes(pairs[0]) == pair_bytes(pairs[1]) == pair_bytes(plain_p)
        assert binary_bytes(bins[0]) == binary_bytes(bins[1]) == binary_bytes(plain_b)
        # the partial grid: what the plain calls give on a context holding exactly the inside bodies
        idx = np.flatnonzero(pg.inside_of(P, grids[2][0]))
        assert pairs[2]["inside"] == len(idx) == bins[2][1]["inside"]
        sub.upload(bodies_of(nb, *[a[idx] for a in S], PREC[tag]))
        assert pair_bytes(sub.pair_counts(pg.EDGES2, squared=True)) == pair_bytes(pairs[2])
        lst, info = sub.binaries(pg.SEP)
        lst = lst.copy()
        lst["i"], lst["j"] = idx[lst["i"]], idx[lst["j"]]
        assert binary_bytes((lst, info)) == binary_bytes(bins[2])
        if n >= 63:
            assert 0 < len(idx) < n and 0 < bins[2][1]["pairs"] < bins[0][1]["pairs"] and bins[0][1]["pairs"] >= 33


# ---------------------------------------------------------------------------------------------------------------------
# 2. grid shapes with a coincident pair; ties on cell boundaries and at the top edge; bins
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_grid_shapes(nb, tag):
    P, V, M, R, f = pg.shapes_state(tag)
    S = (P, V, M, R)
    h2 = (0.1 * f) ** 2
    zero, off = np.array([0.0, h2 / 16, h2 / 4, h2]), np.array([h2 / 64, h2 / 16, h2 / 4, h2])
    with small_stepper(nb, PREC[tag], 300) as st:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        plain = (pair_bytes(st.pair_counts(zero, squared=True)), pair_bytes(st.pair_counts(off, squared=True)),
                 binary_bytes(st.binaries(h2, squared=True)))
        for nx, ny in pg.GRID_SHAPES:
            grid = nb.make_grid(nx, ny, (0, f, 0, f))
            what = "%d x %d" % (nx, ny)
            a, b = ask_pairs(st, P, grid, zero, what=what), ask_pairs(st, P, grid, off, what=what)
            c = ask_binaries(st, S, grid, h2, what=what)
            assert a["outside"] == 0 and (pair_bytes(a), pair_bytes(b), binary_bytes(c)) == plain, what
            # the coincident pair (7, 200): in counts[0] with edges2[0] == 0, in below otherwise, counted and never listed
            assert a["below"] == 0 and b["below"] >= 1 and int(a["counts"][0]) == b["below"] + int(b["counts"][0])
            assert c[1]["coincident"] == 1 and c[1]["pairs"] > 0 and not ((c[0]["i"] == 7) & (c[0]["j"] == 200)).any()


@pytest.mark.parametrize("tag", TAGS)
def test_ties_on_cell_boundaries_and_at_the_top_edge(nb, tag):
    """Spacing = cell side = 1 at offsets 0 and 0.1: the 544 pairs at d2 == 1 cross a cell boundary; `<` at the top edge of
    the counts, `<=` at sep2."""
    S = pg.lattice_state()
    P = S[0]
    pairs = 289 * 288 // 2
    above, under = np.nextafter(1.0, INF), np.nextafter(1.0, 0.0)
    with small_stepper(nb, PREC[tag], 289) as st:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        for ask in pg.lattice_grids():
            grid = nb.make_grid(*ask)
            at = ask_pairs(st, P, grid, np.array([0.0, 1.0]), what="lattice %r" % (ask,))
            over = ask_pairs(st, P, grid, np.array([0.0, above]), what="lattice %r" % (ask,))
            assert (int(at["counts"][0]), at["rest"]) == (0, pairs)
            assert (int(over["counts"][0]), over["rest"]) == (pg.LATTICE_TIES, pairs - pg.LATTICE_TIES)
            assert pair_bytes(at) == pair_bytes(st.pair_counts([0.0, 1.0], squared=True))
            near = ask_binaries(st, S, grid, 1.0, what="lattice %r" % (ask,))
            none = ask_binaries(st, S, grid, under, what="lattice %r" % (ask,))
            assert near[1]["near"] == pg.LATTICE_TIES == near[1]["pairs"] and (none[1]["near"], none[1]["pairs"]) == (0, 0)
            assert binary_bytes(near) == binary_bytes(st.binaries(1.0, squared=True))


@pytest.mark.parametrize("bins", (1, 2, 255, 256))
def test_bins(nb, bins):
    """The trip counts of the edge search, and a last edge of +inf (the whole grid)."""
    n = 300
    S = pg.standard(n, "f32")
    full, _, part = (nb.make_grid(*a) for a in pg.standard_grids(n))
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, *S, 0))
        for top in (pg.SEP2, INF):
            e2 = pg.bins_edges(bins, top)
            a = ask_pairs(st, S[0], full, e2, what="%d bins top %g" % (bins, top))
            ask_pairs(st, S[0], part, e2, what="%d bins top %g partial" % (bins, top))
            assert pair_bytes(a) == pair_bytes(st.pair_counts(e2, squared=True))
            assert a["rest"] == 0 or top < INF


# ---------------------------------------------------------------------------------------------------------------------
# 3. extremes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_extremes(nb, tag):
    P, V, M, R, f = pg.shapes_state(tag)
    S = (P, V, M, R)
    grid = nb.make_grid(8, 8, (0, f, 0, f))
    with small_stepper(nb, PREC[tag], 385) as st:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        lst, info = ask_binaries(st, S, grid, 0.0, what="sep2 0")               # the coincident pair only
        assert (info["near"], info["pairs"], info["coincident"], len(lst)) == (0, 0, 1, 0)
        everything = ask_binaries(st, S, grid, INF, what="sep2 inf")
        assert binary_bytes(everything) == binary_bytes(st.binaries(INF)) and everything[1]["near"] == 300 * 299 // 2 - 1
        # a NaN velocity and a NaN mass: the body's pairs stay near and are never bound; a NaN position: the body is outside
        h2 = (0.1 * f) ** 2
        base = ask_binaries(st, S, grid, h2, what="base")
        k = int(base[0]["i"][len(base[0]) // 2])
        mine = (base[0]["i"] == k) | (base[0]["j"] == k)
        for which, name in ((1, "velocity"), (2, "mass"), (0, "position")):
            T = [a.copy() for a in S]
            T[which][(k, 1) if which < 2 else k] = np.nan
            st.upload(bodies_of(nb, *T, PREC[tag]))
            lst, info = ask_binaries(st, T, grid, h2, what="NaN " + name)
            assert np.array_equal(lst, base[0][~mine]) and len(lst) < len(base[0])
            assert (info["near"] < base[1]["near"]) == (which == 0) and info["outside"] == (which == 0)
            got = ask_pairs(st, T[0], grid, np.array([0.0, h2]), what="NaN " + name)
            assert got["outside"] == (which == 0) and got["pairs"] == (299 * 298 // 2 if which == 0 else 300 * 299 // 2)
        # every body in one cell of an 8 x 8 grid
        Q = pg.one_cell_state(tag)
        st.upload(bodies_of(nb, *Q, PREC[tag]))
        cell = nb.make_grid(8, 8, (0, 8, 0, 8))
        for h2 in (0.01, INF):
            a = ask_pairs(st, Q[0], cell, np.array([0.0, h2 / 4 if h2 < INF else 0.01, h2]), what="one cell")
            b = ask_binaries(st, Q, cell, h2, what="one cell")
            assert pair_bytes(a) == pair_bytes(st.pair_counts(a["edges2"], squared=True))
            assert binary_bytes(b) == binary_bytes(st.binaries(h2, squared=True)) and b[1]["near"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_points(nb, tag):
    """Points on bodies, inside, far outside, at NaN and at 1e200, on a grid that holds every body and on one that does not;
    summed over the points, within()'s count is the count below nextafter(h2)."""
    P, V, M, R, f = pg.shapes_state(tag)
    pts = wc.awkward_points(P, f)
    with small_stepper(nb, PREC[tag], 300) as st:
        st.upload(bodies_of(nb, P, V, M, R, PREC[tag]))
        for ask, h2 in (((16, 16, (0, f, 0, f)), (1.5 * f / 16) ** 2), ((8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f)), (0.2 * f) ** 2),
                        ((4, 4, (0, f, 0, f)), INF)):
            grid = nb.make_grid(*ask)
            e2 = np.array([0.0, h2 / 9, h2]) if h2 < INF else np.array([0.0, 1.0, INF])
            got = ask_pairs(st, P, grid, e2, pts, what="points %r" % (ask,))
            assert got["pairs"] == len(pts) * got["inside"] and got["n_bodies"] == 300
            if got["outside"] == 0:
                assert pair_bytes(got) == pair_bytes(st.pair_counts(e2, pts, squared=True))
            if h2 < INF:
                one = ask_pairs(st, P, grid, np.array([0.0, np.nextafter(h2, INF)]), pts, what="points, one bin")
                assert int(one["counts"][0]) == int(st.within(h2, pts, grid=grid, squared=True)["rows"]["count"].sum()) > 0
        # own rows: 2 * counts[0] is the sum of within()'s count
        grid = nb.make_grid(16, 16, (0, f, 0, f))
        h2 = (1.5 * f / 16) ** 2
        own = ask_pairs(st, P, grid, np.array([0.0, np.nextafter(h2, INF)]), what="own rows, one bin")
        assert 2 * int(own["counts"][0]) == int(st.within(h2, grid=grid, squared=True)["rows"]["count"].sum()) > 0
        b = ask_binaries(st, (P, V, M, R), grid, h2, what="own rows")
        assert b[1]["near"] + b[1]["coincident"] == int(own["counts"][0])


# ---------------------------------------------------------------------------------------------------------------------
# 5. caps
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity(nb):
    n = 300
    S = pg.standard(n, "f32")
    full, _, part = (nb.make_grid(*a) for a in pg.standard_grids(n))
    call = nb.lib.nbody_get_binaries_grid
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, *S, 0))
        for grid in (full, part):
            want, winfo = pg.model_binaries_grid(*S, grid[0], pg.SEP2)
            pairs = winfo["pairs"]
            counts = tuple(winfo[f] for f in bc.COUNTS) + (pg.SEP2, winfo["inside"], winfo["outside"])
            out = np.frombuffer(bytes([0x77]) * (48 * (pairs + 4)), dtype=bc.RECORD_DTYPE).copy()
            before = out.tobytes()
            info = np.full(1, -7, dtype=nb.BINARY_GRID_INFO_DTYPE)
            assert call(st._ctx, grid.ctypes.data, pg.SEP2, out.ctypes.data, pairs - 1, info.ctypes.data) == CAPACITY_ERR
            assert out.tobytes() == before and tuple(info[0]) == counts   # out untouched, info complete
            info[:] = -7
            assert call(st._ctx, grid.ctypes.data, pg.SEP2, None, 0, info.ctypes.data) == 0   # the counts only
            assert tuple(info[0]) == counts
            info[:] = -7
            assert call(st._ctx, grid.ctypes.data, pg.SEP2, out.ctypes.data, pairs, info.ctypes.data) == 0   # it still answers
            assert tuple(info[0]) == counts and out[pairs:].tobytes() == before[48 * pairs:]
            for f in ("i", "j", "flags"):
                assert np.array_equal(out[f][:pairs], want[f])
            for f in bc.ORBIT:
                assert np.array_equal(out[f][:pairs].view(np.uint64), want[f].view(np.uint64))
            # the wrapper: a guess that is too small is repeated once with info.pairs
            for cap in (3 * n, 1, 0, pairs):
                ask_binaries(st, S, grid, pg.SEP2, what="cap %d" % cap, cap=cap)


# ---------------------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_equals_steppers_and_model(nb):
    cap, Sn = pg.BATCH_CAP, len(pg.BATCH_COUNTS)
    states = pg.batch_states()
    bodies = [bodies_of(nb, *s, 0) for s in states]
    pts = np.array([[0.0, 0.0], [3.0, -4.0], [1e200, 0.0], [np.nan, 1.0]])
    with nb.StepperBatch(Sn, cap, params=[(0.2, 0.1, 1000000, 1000000)] * Sn) as batch, small_stepper(nb, 0, cap) as one:
        batch.upload(bodies)
        assert batch.counts().tolist() == list(pg.BATCH_COUNTS)
        for k, ask in enumerate(pg.batch_grids()):
            grid = nb.make_grid(*ask)
            gp, gq = batch.pair_counts(pg.EDGES2, squared=True, grid=grid), batch.pair_counts(pg.EDGES2, pts, squared=True, grid=grid)
            gb = batch.binaries(pg.SEP, grid=grid)
            assert len(gp) == len(gq) == len(gb) == Sn
            worst = max(b[1]["pairs"] for b in gb)
            # the C calls into prefilled buffers: the tails stay
            raw = np.full((Sn, 6), 77, dtype=np.uint64)
            infos = np.zeros(Sn, dtype=nb.PAIR_GRID_INFO_DTYPE)
            e2 = pg.EDGES2
            assert nb.lib.nbody_batch_get_pair_counts_grid(batch._b, grid.ctypes.data, None, 0, e2.ctypes.data, 4, raw.ctypes.data,
                                                          infos.ctypes.data) == 0
            flat = raw.reshape(-1)                                # system s's counts at s * bins
            assert np.array_equal(flat[:4 * Sn].reshape(Sn, 4), np.array([g["counts"] for g in gp])) and (flat[4 * Sn:] == 77).all()
            out = np.frombuffer(bytes([0x77]) * (48 * Sn * (worst + 3)), dtype=bc.RECORD_DTYPE).copy().reshape(Sn, worst + 3)
            binfo = np.zeros(Sn, dtype=nb.BINARY_GRID_INFO_DTYPE)
            assert nb.lib.nbody_batch_get_binaries_grid(batch._b, grid.ctypes.data, pg.SEP2, out.ctypes.data, worst + 3,
                                                       binfo.ctypes.data) == 0
            if worst > 0:
                assert nb.lib.nbody_batch_get_binaries_grid(batch._b, grid.ctypes.data, pg.SEP2, out.ctypes.data, worst - 1,
                                                           binfo.ctypes.data) == CAPACITY_ERR
            for s, S in enumerate(states):
                n = pg.BATCH_COUNTS[s]
                what = "system %d (n %d) grid %r" % (s, n, ask)
                pg.pair_assert_same(gp[s], pg.model_pair_counts_grid(S[0], grid[0], e2), what)
                pg.pair_assert_same(gq[s], pg.model_pair_counts_grid(S[0], grid[0], e2, pts), what + " points")
                pg.binary_assert_same(gb[s], pg.model_binaries_grid(*S, grid[0], pg.SEP2), what)
                assert tuple(infos[s]) == (n, n, gp[s]["pairs"], gp[s]["below"], gp[s]["rest"], gp[s]["inside"], gp[s]["outside"]), what
                p = gb[s][1]["pairs"]
                assert int(binfo["pairs"][s]) == p and (out[s, p:].view(np.uint8) == 0x77).all(), what
                assert np.array_equal(out[s, :p]["i"], gb[s][0]["i"]) and np.array_equal(out[s, :p]["j"], gb[s][0]["j"]), what
                if n == 0:
                    assert (gp[s]["pairs"], gp[s]["inside"], gp[s]["outside"], gb[s][1]["pairs"]) == (0, 0, 0, 0)
                    continue
                one.upload(bodies[s])                             # a Stepper holding the same state
                assert pair_bytes(one.pair_counts(e2, squared=True, grid=grid)) == pair_bytes(gp[s]), what
                assert pair_bytes(one.pair_counts(e2, pts, squared=True, grid=grid)) == pair_bytes(gq[s]), what
                assert binary_bytes(one.binaries(pg.SEP, grid=grid)) == binary_bytes(gb[s]), what
            if k == 0:
                assert all(g["outside"] == 0 for g in gp)
                plain_p, plain_b = batch.pair_counts(e2, squared=True), batch.binaries(pg.SEP)
                assert all(pair_bytes(a) == pair_bytes(b) for a, b in zip(gp, plain_p))
                assert all(binary_bytes(a) == binary_bytes(b) for a, b in zip(gb, plain_b))
            else:
                assert gp[2]["outside"] > 0 and gp[3]["outside"] > 0 and gb[3][1]["pairs"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. a stepped state, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
def test_resident_state_after_collisions(nb):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=7011)
    w = float(dense_field(n))
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as twin:
        st.upload(b)
        twin.upload(b)
        st.step(3)
        twin.step(3)
        S = bc.widen(st.download())
        P, R = S[0], S[3]
        assert len(R) < n                                        # compaction has run
        typical = float(np.median(R))
        edges = np.array([0.0, typical, 2.0 * typical, 4.0 * typical])
        e2, sep = edges * edges, 4.0 * typical
        matched = nb.within_grid((w, w), sep)
        lo, hi = P.min(axis=0) - 1.0, P.max(axis=0) + 1.0
        fitted = nb.make_grid(int(matched["nx"][0]), int(matched["ny"][0]), (lo[0], hi[0], lo[1], hi[1]))
        plain_p, plain_b = st.pair_counts(e2, squared=True), st.binaries(sep)
        for grid in (matched, fitted):
            assert pg.window_holds(P, grid[0], e2[-1]) > len(R)  # on the downloaded state first
            gp = ask_pairs(st, P, grid, e2, what="stepped")
            gb = ask_binaries(st, S, grid, sep * sep, what="stepped")
            assert gp["outside"] == 0 == gb[1]["outside"], grid      # both grids hold every body: the plain calls' bytes
            assert pair_bytes(gp) == pair_bytes(plain_p) and binary_bytes(gb) == binary_bytes(plain_b), grid
            assert int(gp["counts"].sum()) > 0 and gb[1]["near"] > 0
        st.step(2)
        twin.step(2)
        assert st.download().block.tobytes() == twin.download().block.tobytes()
        assert int(st.stats().pairs) == int(twin.stats().pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 8. ranks
# ---------------------------------------------------------------------------------------------------------------------
def test_either_rank_of_a_sharded_group(nb):
    world, n = 2, 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    w = float(dense_field(n))
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    try:
        grp.upload(b)
        grp.step(sc.LAG + 2)                                      # past the exchange lag
        P, R = nc.widen(grp.download())
        assert len(R) < n
        top = 4.0 * float(np.median(R))
        e2 = np.array([0.0, 0.25 * top * top, top * top])
        grid = nb.within_grid((w, w), top)
        assert pg.window_holds(P, grid[0], e2[-1]) > len(R)
        want = pg.model_pair_counts_grid(P, grid[0], e2)
        rank1 = grp.pair_counts(e2, squared=True, grid=grid, rank=1)      # each on its own: not collective
        rank0 = grp.pair_counts(e2, squared=True, grid=grid, rank=0)
        pg.pair_assert_same(rank0, want, "rank 0")
        assert pair_bytes(rank1) == pair_bytes(rank0) and int(rank0["counts"].sum()) > 0
        out, info = np.zeros(64, dtype=nb.BINARY_RECORD_DTYPE), np.zeros(1, dtype=nb.BINARY_GRID_INFO_DTYPE)
        for r in grp.ranks:                                       # a rank holds only its own velocities
            assert nb.lib.nbody_get_binaries_grid(r._ctx, grid.ctypes.data, top * top, out.ctypes.data, 64, info.ctypes.data) == STATE_ERR
            assert b"single-rank" in nb.lib.nbody_last_error_string()
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors on a live handle, and the buffers shared with the other queries
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_shared_buffers(nb):
    P, V, M, R, f = pg.shapes_state("f32")
    S = (P, V, M, R)
    grid = nb.make_grid(8, 8, (0, f, 0, f))
    other = nb.make_grid(5, 3, (0.25 * f, f, 0, f))
    h = 0.1 * f
    e2 = np.array([0.0, 0.25 * h * h, h * h])
    counts, pinfo = np.full(2, 7, dtype=np.uint64), np.full(1, -7, dtype=nb.PAIR_GRID_INFO_DTYPE)
    out, binfo = np.zeros(8, dtype=nb.BINARY_RECORD_DTYPE), np.full(1, -7, dtype=nb.BINARY_GRID_INFO_DTYPE)
    pcall, bcall = nb.lib.nbody_get_pair_counts_grid, nb.lib.nbody_get_binaries_grid

    def others(s):
        w = s.within(h, grid=other, lists=True)
        c = s.cells(other, lists=True)
        g = s.groups(gg.EDGE_LINK, grid=other)
        k = s.knn(4, grid=other)
        return (w["rows"].tobytes(), w["list"].tobytes(), c["cells"].tobytes(), c["order"].tobytes(), g["label"].tobytes(),
                kg.bits(k["d2"]).tobytes(), k["index"].tobytes())

    with small_stepper(nb, 0, 300) as st, small_stepper(nb, 0, 300) as fresh:
        assert pcall(st._ctx, grid.ctypes.data, None, 0, e2.ctypes.data, 2, counts.ctypes.data, pinfo.ctypes.data) == STATE_ERR
        assert b"before" in nb.lib.nbody_last_error_string()
        assert bcall(st._ctx, grid.ctypes.data, h * h, out.ctypes.data, 8, binfo.ctypes.data) == STATE_ERR
        assert (counts == 7).all() and (pinfo["pairs"] == -7).all() and (binfo["pairs"] == -7).all()
        st.upload(bodies_of(nb, *S, 0))
        fresh.upload(bodies_of(nb, *S, 0))
        want = others(fresh)
        assert others(st) == want                                 # before the new calls
        gp = ask_pairs(st, P, grid, e2, what="shared")
        gb = ask_binaries(st, S, grid, h * h, what="shared")
        assert others(st) == want                                 # and after them, on another grid
        # the plain calls share PairsState and the binary log: after the grid forms they give their own bytes
        assert pair_bytes(st.pair_counts(e2, squared=True)) == pair_bytes(fresh.pair_counts(e2, squared=True)) == pair_bytes(gp)
        assert binary_bytes(st.binaries(h)) == binary_bytes(fresh.binaries(h)) == binary_bytes(gb)
        enc = st.encounters(1.0), fresh.encounters(1.0)
        assert enc[0][0].tobytes() == enc[1][0].tobytes() and enc[0][1] == enc[1][1]
        pg.pair_assert_same(st.pair_counts(e2, squared=True, grid=grid), gp, "again")
        pg.binary_assert_same(st.binaries(h, grid=grid), gb, "again")
        st.upload(nb.BodiesData(0))                               # no bodies: nothing launched
        assert pcall(st._ctx, grid.ctypes.data, None, 0, e2.ctypes.data, 2, counts.ctypes.data, pinfo.ctypes.data) == 0
        assert tuple(pinfo[0]) == (0,) * 7 and not counts.any()
        assert bcall(st._ctx, grid.ctypes.data, h * h, None, 0, binfo.ctypes.data) == 0
        assert tuple(binfo[0]) == (0, 0, 0, 0, 0, 0, h * h, 0, 0)
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 1000000, 1000000)] * 2) as batch:
        counts2, pinfo2 = np.full(4, 7, dtype=np.uint64), np.full(2, -7, dtype=nb.PAIR_GRID_INFO_DTYPE)
        binfo2 = np.full(2, -7, dtype=nb.BINARY_GRID_INFO_DTYPE)
        assert nb.lib.nbody_batch_get_pair_counts_grid(batch._b, grid.ctypes.data, None, 0, e2.ctypes.data, 2, counts2.ctypes.data,
                                                      pinfo2.ctypes.data) == STATE_ERR
        assert nb.lib.nbody_batch_get_binaries_grid(batch._b, grid.ctypes.data, h * h, None, 0, binfo2.ctypes.data) == STATE_ERR
        assert (counts2 == 7).all() and (pinfo2["pairs"] == -7).all() and (binfo2["pairs"] == -7).all()
        batch.upload([bodies_of(nb, *S, 0), nb.BodiesData(0)])
        got = batch.pair_counts(e2, squared=True, grid=grid)      # and the handle goes on
        pg.pair_assert_same(got[0], gp, "batch after its errors")
        pg.binary_assert_same(batch.binaries(h, grid=grid)[0], gb, "batch after its errors")
