"""The model of the encounters on the cell list against a literal walk of every owner row's window, the window rule's property
- a swept pair has d2 <= H2 of its owner and the other end's cell in the owner's window - on every constructed case and every
grid of the GPU tests, that every constructed case takes the branch it was built for, and the argument checks of the two entry
points, which need no device.  No GPU."""
import collections

import numpy as np
import pytest

import cell_cases as cc
import encounter_cases as ec
import encounters_grid_cases as eg

INVALID = -1
INF = float("inf")
TAGS = tuple(eg.DTYPES)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reach and the owner
# ---------------------------------------------------------------------------------------------------------------------
def test_reach_is_what_a_scalar_loop_gives():
    for tag in TAGS:
        P, V, R = eg.standard(65, tag)
        for h in (0.0, 1e-300, eg.H, 1e300, INF):
            a, b = eg.reach(P, V, R, h, eg.DTYPES[tag]), eg.reach_loop(P, V, R, h, eg.DTYPES[tag])
            assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b)), (tag, h)
    for name, c in eg.cases().items():
        a, b = eg.reach(*c.state, c.h, c.dtype), eg.reach_loop(*c.state, c.h, c.dtype)
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b)), name
    # h = 0: rho = |R|; a NaN velocity, 0 * inf and the fp64 guard: +inf; fp32 has no guard
    P, V, R = np.array([[1.0, 1.0]] * 4), np.array([[3.0, -4.0], [np.nan, 0.0], [0.0, 0.0], [1e-40, 0.0]]), np.array([-2.0, 1.0, 1.0, 1.0])
    assert eg.reach(P, V, R, 0.0, np.float32)[0].tolist() == [2.0, INF, 1.0, 1.0]
    assert eg.reach(P, V, R, 0.5, np.float32)[0].tolist() == [5.5, INF, 1.0, 1.0]
    assert eg.reach(P, V, R, INF, np.float32)[0].tolist() == [INF, INF, INF, INF]
    assert eg.reach(P, V, R, 0.5, np.float64)[0].tolist() == [5.5, INF, 1.0, INF]
    rho, Hh, H2 = eg.reach(P, V, R, 0.5, np.float32)
    assert Hh[0] == 11.0 * (1.0 + 2.0 ** -40) and H2[0] == Hh[0] * Hh[0] and Hh[1] == INF == H2[1]


def test_every_pair_has_exactly_one_owner():
    rho = np.array([1.0, 1.0, 2.0, INF, INF, 0.0])
    k = np.arange(len(rho))
    i, j = np.meshgrid(k, k, indexing="ij")
    own = eg.owner(rho, i, j)
    off = i != j
    assert (own ^ own.T)[off].all() and not own[~off].any()
    assert own[1, 0] and own[2, 1] and own[4, 3] and own[3, 2] and own[0, 5]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the window rule and the walk, before any kernel runs: every state and grid of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", eg.BODY_COUNTS)
def test_edge_cases_hold_and_are_what_the_gpu_tests_take_them_for(n, tag):
    P, V, R = eg.standard(n, tag)
    full, one, part = (cc.grid_of(*a) for a in eg.standard_grids(n))
    for grid in (full, one, part):
        eg.window_holds(P, V, R, grid, eg.H, eg.DTYPES[tag])
    mf, mo, mp = (eg.model_encounters_grid(P, V, R, g, eg.H) for g in (full, one, part))
    eg.assert_same(mf, mo)
    ec.assert_same(mf, ec.model_encounters(P, V, R, eg.H))      # nothing outside: the plain model
    assert mf[1]["outside"] == 0 and mf[1]["inside"] == n
    if n <= 65:
        for grid, m in ((full, mf), (one, mo), (part, mp)):
            eg.assert_same(eg.loop_encounters_grid(P, V, R, grid, eg.H, eg.DTYPES[tag]), m, "walk")
    if n >= 63:
        assert mf[1]["pairs"] >= 33 and 0 < mp[1]["inside"] < n and 0 < mp[1]["pairs"] < mf[1]["pairs"] and mf[1]["missed"] > 0


@pytest.mark.parametrize("name", eg.case_names())
def test_constructed_cases(name):
    c = eg.cases()[name]
    for k, ask in enumerate(c.asks):
        grid = cc.grid_of(*ask)
        model = eg.model_encounters_grid(*c.state, grid, c.h)
        eg.assert_same(eg.loop_encounters_grid(*c.state, grid, c.h, c.dtype), model, "%s %r" % (name, ask))   # nothing lost, nothing twice
        assert eg.window_holds(*c.state, grid, c.h, c.dtype) == model[1]["pairs"]
        for f, v in c.expect.items():
            assert model[1][f] == v, (name, ask, f, model[1][f], v)
        if c.rule is not None:
            assert eg.owner_rules(*c.state, grid, c.h, c.dtype)[c.rule] >= 1, (name, c.rule)
    if c.expect.get("outside", 0) == 0:
        ec.assert_same(eg.model_encounters_grid(*c.state, cc.grid_of(*c.asks[0]), c.h), ec.model_encounters(*c.state, c.h), name)


def test_constructed_cases_take_their_branches():
    C = eg.cases()
    for tag in TAGS:
        dt = eg.DTYPES[tag]
        def terms(name):
            c = C["%s-%s" % (name, tag)]
            t = eg.pair_terms(*c.state, c.h, 1, 0)
            rho, Hh, H2 = eg.reach(*c.state, c.h, dt)
            return c, t, rho, H2
        c, t, rho, _ = terms("fast-small")
        assert abs(c.R[1]) < abs(c.R[0]) and rho[1] > rho[0] and t["end"] and not t["now"]
        c, t, rho, _ = terms("slow-large")
        assert abs(c.R[0]) > abs(c.R[1]) and rho[0] > rho[1] and t["end"] and not t["now"]
        c, t, rho, _ = terms("head-on")
        assert rho[0] == rho[1] and eg.owner(rho, 1, 0) and not eg.owner(rho, 0, 1)
        c, t, rho, _ = terms("bullet")
        assert t["mid"] and not t["now"] and not t["end"]
        assert c.h * c.V[0, 0] == 10.0                          # ten cells of the 64 x 64 grid over the field
        cells = eg.window_cells(*c.state, cc.grid_of(64, 64, (0.0, eg.FIELD, 0.0, eg.FIELD)), c.h, dt)
        assert cells[0] >= 31 * 41 and cells[1] <= 9       # 20.5 cells to either side, cut at x = 0
        c, t, rho, _ = terms("end-exact")
        assert t["e2"] == t["s2"] == 25.0 and t["end"] and not t["mid"] and not t["now"]
        c, t, rho, _ = terms("grazing")
        assert t["disc"] == 0.0 and t["mid"] and not t["end"] and not t["now"]
        c, t, rho, H2 = terms("at-reach")
        two = rho[1] + rho[1]
        assert t["d2"] == two * two and t["d2"] <= H2[1] and t["d2"] > H2[1] * (1.0 - 2.0 ** -38) and t["swept"]
        c, t, rho, _ = terms("bulk")
        assert not t["swept"] and rho[0] == rho[1] == 501.0
        assert (eg.window_cells(*c.state, cc.grid_of(64, 64, (0.0, eg.FIELD, 0.0, eg.FIELD)), c.h, dt) == 64 * 64).all()
        c, t, rho, _ = terms("negative-radius")
        assert c.R[0] < 0 and rho[0] == 1.0 and t["now"]
        c, t, rho, _ = terms("nan-velocity")
        assert np.isnan(c.V[0, 0]) and rho[0] == INF and t["now"] and not t["end"] and not t["mid"]
        lst, info = eg.model_encounters_grid(*c.state, cc.grid_of(*c.asks[0]), c.h)
        assert (lst["t"][0], lst["i"][0], lst["j"][0], lst["flags"][0]) == (0.0, 0, 1, ec.NOW) and not np.signbit(lst["t"][0])
        c, t, rho, _ = terms("nan-coordinate")
        assert np.isnan(c.P[0, 0]) and not eg.inside_of(c.P, cc.grid_of(*c.asks[0]))[0]
        c, t, rho, _ = terms("infinite-radius")
        assert rho[0] == INF and t["s2"] == INF and t["now"] and t["end"]
        c, t, rho, _ = terms("outside")
        assert t["now"] and eg.inside_of(c.P, cc.grid_of(*c.asks[0])).tolist()[:2] == [True, False]
        c, t, rho, _ = terms("h-zero")
        assert np.array_equal(rho, np.abs(c.R)) and t["now"] and t["end"] and not t["mid"]
        lst, info = eg.model_encounters_grid(*c.state, cc.grid_of(*c.asks[0]), 0.0)
        assert info["pairs"] == info["now"] == info["end"] and info["missed"] == 0
        c, t, rho, _ = terms("h-tiny")
        assert c.h == 1e-300 and np.array_equal(rho, np.abs(c.R)) and t["now"]
        c, t, rho, _ = terms("h-inf")
        assert (rho == INF).all() and t["mid"] and not t["end"] and not t["now"]
    c = C["guard-f64"]
    rho = eg.reach(*c.state, c.h, np.float64)[0]
    assert rho[0] == INF and np.isfinite(rho[1:]).all() and np.isfinite(eg.reach(*c.state, c.h, np.float32)[0]).all()
    assert eg.window_cells(*c.state, cc.grid_of(64, 64, (0.0, eg.FIELD, 0.0, eg.FIELD)), c.h, np.float64)[0] == 64 * 64
    c = C["guard-hit-f64"]
    assert eg.reach(*c.state, c.h, np.float64)[0][0] == INF


def test_the_set_has_a_pair_owned_by_each_rule():
    total = collections.Counter()
    for c in eg.cases().values():
        total += eg.owner_rules(*c.state, cc.grid_of(*c.asks[0]), c.h, c.dtype)
    for tag in TAGS:
        total += eg.owner_rules(*eg.standard(300, tag), cc.grid_of(*eg.standard_grids(300)[0]), eg.H, eg.DTYPES[tag])
    assert total["radius"] >= 1 and total["speed"] >= 1 and total["index"] >= 1, total


@pytest.mark.parametrize("tag", TAGS)
def test_horizons_on_the_300_body_state(tag):
    P, V, R = eg.horizon_state(tag)
    full, _, part = (cc.grid_of(*a) for a in eg.standard_grids(300))
    seen = []
    for h in eg.HORIZONS + (1e-300,):
        for grid in (full, part):
            eg.window_holds(P, V, R, grid, h, eg.DTYPES[tag])
        lst, info = eg.model_encounters_grid(P, V, R, full, h)
        seen.append(info)
        if h == 0.0:
            assert info["pairs"] == info["now"] == info["end"] > 0 and info["missed"] == 0
            assert np.array_equal(eg.reach(P, V, R, h, eg.DTYPES[tag])[0], np.abs(R))
    assert seen[0]["pairs"] < seen[1]["pairs"] < seen[2]["pairs"] < seen[3]["pairs"] and seen[2]["missed"] > 0
    assert seen[4]["pairs"] == seen[0]["pairs"]                  # a tiny horizon sweeps what overlaps now


def test_batch_states_hold():
    states = eg.batch_states()
    assert [len(s[2]) for s in states] == list(eg.BATCH_COUNTS)
    holds, leaves = (cc.grid_of(*a) for a in eg.batch_grids())
    for S in states:
        for grid in (holds, leaves):
            eg.window_holds(*S, grid, eg.H, np.float32)
    assert all(eg.inside_of(s[0], holds).all() for s in states)
    assert all(0 < eg.inside_of(s[0], leaves).sum() < len(s[2]) for s in states[2:])
    assert eg.model_encounters_grid(*states[3], leaves, eg.H)[1]["pairs"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host side of the product: argument checks before any device call
# ---------------------------------------------------------------------------------------------------------------------
def _bad_grids(nb):
    return (None, nb.make_grid(0, 4, (0, 1, 0, 1)), nb.make_grid(2048, 1024, (0, 1, 0, 1)), nb.make_grid(4, 4, (0, 0, 0, 1)),
            nb.make_grid(4, 4, (np.nan, 1, 0, 1)), nb.make_grid(4, 4, (1, 0, 0, 1)))


def test_invalid_arguments_need_no_handle():
    import ppa_nbody_collisions_amd as nb
    grid = nb.make_grid(4, 4, (0, 1, 0, 1))
    out, info = np.zeros(8, dtype=nb.ENCOUNTER_RECORD_DTYPE), np.zeros(1, dtype=nb.ENCOUNTER_GRID_INFO_DTYPE)
    data = lambda a: None if a is None else a.ctypes.data        # noqa: E731
    for fn in (nb.lib.nbody_get_encounters_grid, nb.lib.nbody_batch_get_encounters_grid):
        def call(g=grid, h=1.0, o=out, cap=8, inf=info, handle=None):
            return fn(handle, data(g), h, data(o), cap, data(inf))
        assert call() == INVALID                                 # a NULL handle, everything else in order
        bad = [dict(g=g) for g in _bad_grids(nb)]
        bad += [dict(h=np.nan), dict(h=-1.0), dict(h=-INF), dict(cap=-1), dict(o=None, cap=8), dict(inf=None),
                dict(cap=(1 << 31) // 24 + 1)]                   # 24 bytes a record: more than 2^31
        for b in bad:
            assert call(**b) == INVALID, b
            assert not out.view(np.uint8).any() and not info.view(np.uint8).any()
        assert b"nbody" in nb.lib.nbody_last_error_string()
        assert call(g=None, h=np.nan) == INVALID and b"grid" in nb.lib.nbody_last_error_string()      # the grid first
    assert nb.ENCOUNTER_GRID_INFO_DTYPE.itemsize == 64 and nb.ENCOUNTER_GRID_INFO_DTYPE.names == eg.INFO_DTYPE.names
    assert nb.ENCOUNTER_GRID_INFO_DTYPE.names[:6] == nb.ENCOUNTER_INFO_DTYPE.names


def test_the_matched_grid_is_within_grid():
    import ppa_nbody_collisions_amd as nb
    g = nb.encounters_grid((100, 50), 0.5, 2.0, 6.0)             # 2 * (2 + 0.5 * 6) = 10
    w = nb.within_grid((100, 50), 10.0)
    assert g.tobytes() == w.tobytes() and (g["nx"][0], g["ny"][0]) == (20, 10)
    assert nb.encounters_grid((100, 50), 0.0, 0.0, 1.0, most=64)["nx"][0] == 64
    assert nb.encounters_grid((100, 50), INF, 1.0, 1.0)["nx"][0] == 1
