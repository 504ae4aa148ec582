"""The model of the pair counts and the bound pairs on the cell list against plain double loops, the window rule's property -
every counted or near pair lies inside its row's window - on every constructed case of the GPU tests, and the argument checks
of the four entry points, which need no device.  No GPU."""
import numpy as np
import pytest

import binary_cases as bc
import cell_cases as cc
import pair_cases as pc
import pairs_grid_cases as pg
import within_cases as wc

INVALID = -1
INF = float("inf")
TAGS = tuple(pg.DTYPES)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the window rule, before any kernel runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", pg.BODY_COUNTS)
def test_window_holds_on_the_edge_cases(n, tag):
    P = pg.standard(n, tag)[0]
    for ask in pg.standard_grids(n):
        grid = cc.grid_of(*ask)
        pg.window_holds(P, grid, pg.EDGES2[-1], strict=True)     # the pair counts: d2 < top
        pg.window_holds(P, grid, pg.SEP2)                        # the binaries: d2 <= sep2
    full = cc.grid_of(*pg.standard_grids(n)[0])
    assert pg.inside_of(P, full).all()                           # the bounding square holds every body


@pytest.mark.parametrize("tag", TAGS)
def test_window_holds_on_the_special_cases(tag):
    P, V, M, R, f = pg.shapes_state(tag)
    for nx, ny in pg.GRID_SHAPES:
        grid = cc.grid_of(nx, ny, (0, f, 0, f))
        assert pg.inside_of(P, grid).all()
        assert pg.window_holds(P, grid, (0.1 * f) ** 2) > 300    # the self pairs and more
    L = pg.lattice_state()[0]
    for ask in pg.lattice_grids():
        grid = cc.grid_of(*ask)
        for h2 in (1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, INF)):
            ties = pg.window_holds(L, grid, h2) - 289            # both ends of every pair, less the self pairs
            assert ties == (2 * pg.LATTICE_TIES if h2 >= 1.0 else 0), (ask, h2, ties)
    Q = pg.one_cell_state(tag)[0]
    grid = cc.grid_of(8, 8, (0, 8, 0, 8))
    assert len(set(cc.cell_index(Q, grid))) == 1
    for h2 in (0.0, 0.01, INF):
        pg.window_holds(Q, grid, h2)
    pts = wc.awkward_points(P, f)
    for ask in ((16, 16, (0, f, 0, f)), (8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f))):
        for h2 in ((1.5 * f / 16) ** 2, INF):
            pg.window_holds(P, cc.grid_of(*ask), h2, rows_xy=pts)
    for P4, V4, M4, R4 in pg.batch_states():
        for ask in pg.batch_grids():
            pg.window_holds(P4, cc.grid_of(*ask), pg.SEP2)
            for bins in (1, 2, 255, 256):
                pg.window_holds(P4, cc.grid_of(*ask), pg.bins_edges(bins)[-1], strict=True)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", (1, 2, 63, 65))
def test_subset_model_equals_a_plain_double_loop(n, tag):
    P, V, M, R = pg.standard(n, tag)
    pts = wc.awkward_points(P, 2.0 * pg.half_of(n))[:20] - pg.half_of(n)
    for ask in pg.standard_grids(n):
        grid = cc.grid_of(*ask)
        pg.pair_assert_same(pg.model_pair_counts_grid(P, grid, pg.EDGES2), pg.loop_pair_counts_grid(P, grid, pg.EDGES2), str(ask))
        pg.pair_assert_same(pg.model_pair_counts_grid(P, grid, pg.EDGES2, pts), pg.loop_pair_counts_grid(P, grid, pg.EDGES2, pts),
                            "points %r" % (ask,))
        for sep2 in (pg.SEP2, INF):
            pg.binary_assert_same(pg.model_binaries_grid(P, V, M, R, grid, sep2), pg.loop_binaries_grid(P, V, M, R, grid, sep2),
                                  "%r sep2 %g" % (ask, sep2))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", pg.BODY_COUNTS)
def test_edge_cases_are_what_the_gpu_tests_take_them_for(n, tag):
    P, V, M, R = pg.standard(n, tag)
    full, one, part = (cc.grid_of(*a) for a in pg.standard_grids(n))
    pf, pp = pg.model_pair_counts_grid(P, full, pg.EDGES2), pg.model_pair_counts_grid(P, part, pg.EDGES2)
    bf, bp = pg.model_binaries_grid(P, V, M, R, full, pg.SEP2), pg.model_binaries_grid(P, V, M, R, part, pg.SEP2)
    pg.pair_assert_same(pf, pg.model_pair_counts_grid(P, one, pg.EDGES2))
    pc.assert_same(pf, pc.model_pair_counts(P, pg.EDGES2))       # nothing outside: the plain model
    bc.assert_same(bf, bc.model_binaries(P, V, M, R, pg.SEP2))
    assert pf["outside"] == 0 and bf[1]["near"] + bf[1]["coincident"] == int(pf["counts"].sum())
    if n >= 63:
        assert 33 <= bf[1]["pairs"] <= 280 and 90 <= bf[1]["near"] <= 633 and (pf["counts"][1:] > 0).all()   # [0, 4) is empty at n = 63
        assert 24 <= pp["inside"] <= 136 and 0 < bp[1]["pairs"] < bf[1]["pairs"] and 0 < bp[1]["near"] < bf[1]["near"]
        assert 0 < int(pp["counts"].sum()) < int(pf["counts"].sum())


def test_special_cases_are_what_the_gpu_tests_take_them_for():
    for tag in TAGS:
        P, V, M, R, f = pg.shapes_state(tag)
        assert (P[7] == P[200]).all()
        grid = cc.grid_of(3, 3, (0, f, 0, f))
        zero = pg.model_pair_counts_grid(P, grid, [0.0, 1.0, 4.0])
        off = pg.model_pair_counts_grid(P, grid, [0.25, 1.0, 4.0])
        assert zero["below"] == 0 and off["below"] >= 1 and int(zero["counts"][0]) == int(off["counts"][0]) + off["below"]
        lst, info = pg.model_binaries_grid(P, V, M, R, grid, (0.1 * f) ** 2)
        assert info["coincident"] == 1 and info["pairs"] > 0 and not ((lst["i"] == 7) & (lst["j"] == 200)).any()
    L, LV, LM, LR = pg.lattice_state()
    for ask in pg.lattice_grids():
        grid = cc.grid_of(*ask)
        at = pg.model_pair_counts_grid(L, grid, [0.0, 1.0])
        above = pg.model_pair_counts_grid(L, grid, [0.0, np.nextafter(1.0, INF)])
        pairs = 289 * 288 // 2
        assert (int(at["counts"][0]), at["rest"]) == (0, pairs) and (int(above["counts"][0]), above["rest"]) == (pg.LATTICE_TIES, pairs - pg.LATTICE_TIES)
        assert pg.model_binaries_grid(L, LV, LM, LR, grid, 1.0)[1]["near"] == pg.LATTICE_TIES == 544
        assert pg.model_binaries_grid(L, LV, LM, LR, grid, np.nextafter(1.0, 0.0))[1]["near"] == 0
    for bins in (1, 2, 255, 256):
        e = pg.bins_edges(bins)
        assert len(e) == bins + 1 and (np.diff(e) > 0).all() and e[0] == 0.0 and e[-1] == pg.SEP2
        assert np.isinf(pg.bins_edges(bins, INF)[-1]) and (np.diff(pg.bins_edges(bins, INF)) > 0).all()
    states = pg.batch_states()
    assert [len(s[3]) for s in states] == list(pg.BATCH_COUNTS)
    holds, leaves = (cc.grid_of(*a) for a in pg.batch_grids())
    assert all(pg.inside_of(s[0], holds).all() for s in states)
    assert all(0 < pg.inside_of(s[0], leaves).sum() < len(s[3]) for s in states[2:])


def test_within_consequence_in_the_model():
    """Nothing outside, own rows: 2 * counts[0] at {0, nextafter(h2, +inf)} is the sum of within()'s count at h2."""
    P, V, M, R = pg.standard(300, "f32")
    grid = cc.grid_of(*pg.standard_grids(300)[0])
    got = pg.model_pair_counts_grid(P, grid, [0.0, np.nextafter(pg.SEP2, INF)])
    assert 2 * int(got["counts"][0]) == int(wc.model_within(P, R, grid, pg.SEP2)["rows"]["count"].sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host side of the product: argument checks before any device call
# ---------------------------------------------------------------------------------------------------------------------
def _bad_grids(nb):
    return (None, nb.make_grid(0, 4, (0, 1, 0, 1)), nb.make_grid(2048, 1024, (0, 1, 0, 1)), nb.make_grid(4, 4, (0, 0, 0, 1)),
            nb.make_grid(4, 4, (np.nan, 1, 0, 1)), nb.make_grid(4, 4, (1, 0, 0, 1)))


def test_pair_counts_invalid_arguments_need_no_handle():
    import ppa_nbody_collisions_amd as nb
    grid = nb.make_grid(4, 4, (0, 1, 0, 1))
    edges = np.array([0.0, 1.0, 4.0])
    counts, info = np.zeros(8, dtype=np.uint64), np.zeros(1, dtype=nb.PAIR_GRID_INFO_DTYPE)
    pts = np.zeros((4, 2))
    data = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    for fn in (nb.lib.nbody_get_pair_counts_grid, nb.lib.nbody_batch_get_pair_counts_grid):
        def call(g=grid, p=None, m=0, e=edges, bins=2, c=counts, inf=info, handle=None):
            return fn(handle, data(g), data(p), m, data(e), bins, data(c), data(inf))
        assert call() == INVALID                                 # a NULL handle, everything else in order
        assert call(p=pts, m=4) == INVALID
        bad = [dict(g=g) for g in _bad_grids(nb)]
        bad += [dict(e=None), dict(c=None), dict(inf=None), dict(bins=0), dict(bins=-1), dict(bins=257), dict(p=pts, m=-1),
                dict(p=pts, m=(1 << 27) + 1),                    # 16 bytes a point: more than 2^31
                dict(e=np.array([np.nan, 1.0, 4.0])), dict(e=np.array([-1.0, 1.0, 4.0])), dict(e=np.array([0.0, 4.0, 1.0])),
                dict(e=np.array([0.0, 1.0, 1.0])), dict(e=np.array([0.0, 1.0, np.nan])), dict(e=np.array([0.0, INF, INF]))]
        for b in bad:
            assert call(**b) == INVALID, b
            assert not counts.any() and not info.view(np.uint8).any()
        assert b"nbody" in nb.lib.nbody_last_error_string()
    big = np.zeros(258)
    big[1:] = np.arange(1, 258)
    assert nb.lib.nbody_get_pair_counts_grid(None, data(grid), None, 0, data(big), 257, data(np.zeros(257, dtype=np.uint64)), data(info)) == INVALID
    assert nb.PAIR_GRID_INFO_DTYPE.itemsize == 56 and nb.PAIR_GRID_INFO_DTYPE.names == pg.PAIR_INFO_DTYPE.names
    assert nb.PAIR_GRID_INFO_DTYPE.names[:5] == nb.PAIR_INFO_DTYPE.names


def test_binaries_invalid_arguments_need_no_handle():
    import ppa_nbody_collisions_amd as nb
    grid = nb.make_grid(4, 4, (0, 1, 0, 1))
    out, info = np.zeros(8, dtype=nb.BINARY_RECORD_DTYPE), np.zeros(1, dtype=nb.BINARY_GRID_INFO_DTYPE)
    data = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    for fn in (nb.lib.nbody_get_binaries_grid, nb.lib.nbody_batch_get_binaries_grid):
        def call(g=grid, sep2=1.0, o=out, cap=8, inf=info, handle=None):
            return fn(handle, data(g), sep2, data(o), cap, data(inf))
        assert call() == INVALID                                 # a NULL handle, everything else in order
        bad = [dict(g=g) for g in _bad_grids(nb)]
        bad += [dict(sep2=np.nan), dict(sep2=-1.0), dict(sep2=-INF), dict(cap=-1), dict(o=None, cap=8), dict(inf=None),
                dict(cap=(1 << 31) // 48 + 1)]                   # 48 bytes a record: more than 2^31
        for b in bad:
            assert call(**b) == INVALID, b
            assert not out.view(np.uint8).any() and not info.view(np.uint8).any()
    assert nb.BINARY_GRID_INFO_DTYPE.itemsize == 72 and nb.BINARY_GRID_INFO_DTYPE.names == pg.BINARY_INFO_DTYPE.names
    assert nb.BINARY_GRID_INFO_DTYPE.names[:7] == nb.BINARY_INFO_DTYPE.names


def test_the_matched_grid_is_within_grid():
    import ppa_nbody_collisions_amd as nb
    g = nb.within_grid((100, 50), pg.SEP)
    assert (g["nx"][0], g["ny"][0]) == (13, 6) and 1.0 / g["sx"][0] >= pg.SEP and 1.0 / g["sy"][0] >= pg.SEP
