"""The model of the groups on the cell list against the brute-force groups, the window rule's property - every link is seen
from its larger end - on every constructed case of the GPU tests, and the argument checks of the two entry points, which
need no device.  No GPU."""
import numpy as np
import pytest

import cell_cases as cc
import group_cases as gc
import groups_grid_cases as gg
import within_cases as wc

INVALID = -1


# ---------------------------------------------------------------------------------------------------------------------
# 1. the window rule, before any kernel runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gg.case_names())
def test_window_holds_on_every_case(name):
    case = gg.cases()[name]
    for ask in case.asks:
        links = gg.window_holds(case.P, case.R, case.grid(ask), ask[3], ask[4])
        assert links == gg.adjacency_grid(case.P, case.R, case.grid(ask), ask[3], ask[4]).sum() // 2


def test_window_is_asymmetric():
    """What the design rests on: a small body under the big one does NOT have the big body's cell in its own window - only
    the big body's row finds that link - and the absolute value matters for a negative radius."""
    case = gg.cases()["asymmetric-first-negative-f64"]
    P, R, grid = case.P, case.R, case.grid(case.asks[0])
    x0, y0, sx, sy, nx, ny = grid
    A = gg.adjacency_grid(P, R, grid, 0.0, 1.0)
    under = np.flatnonzero(A[0])
    assert len(under) > 50 and (R[under] == R[1]).all()          # small bodies only
    S = 2.0 * np.abs(R)
    c0, c1 = wc._span((P[:, 0] - x0) * sx, S * sx, nx)
    r0, r1 = wc._span((P[:, 1] - y0) * sy, S * sy, ny)
    far = (np.abs(P[under, 0] - P[0, 0]) > 4.0) | (np.abs(P[under, 1] - P[0, 1]) > 4.0)
    assert far.any()                                             # bodies four and five cells away
    big_cell = (int((P[0, 0] - x0) * sx), int((P[0, 1] - y0) * sy))
    sees_big = (c0[under] <= big_cell[0]) & (big_cell[0] <= c1[under]) & (r0[under] <= big_cell[1]) & (big_cell[1] <= r1[under])
    assert not sees_big[far].any()
    neg = len(R) - 1
    assert R[neg] < 0 and A[neg].sum() > 20                      # s < 0, s*s large: linked all the same
    assert (c0[neg], c1[neg]) == (0, 16) and (2.0 * R[neg]) * (2.0 * R[neg]) == S[neg] * S[neg]   # x = 4.5, S = 12
    with pytest.raises(AssertionError):                          # the signed radius would give that row an empty reach
        _signed_window(P, R, grid)


def _signed_window(P, R, grid):
    """window_holds with S taken from the signed radius: fails on a negative one."""
    x0, y0, sx, sy, nx, ny = grid
    S = np.maximum(2.0 * R, 0.0)
    c0, c1 = wc._span((P[:, 0] - x0) * sx, S * sx, nx)
    cell = cc.cell_index(P, grid)
    ix = cell % nx
    A = gg.adjacency_grid(P, R, grid, 0.0, 1.0)
    need = A & (np.abs(R)[None, :] <= np.abs(R)[:, None])
    seen = (c0[:, None] <= ix[None, :]) & (ix[None, :] <= c1[:, None])
    assert not (need & ~seen).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bodies-65-f32", "bodies-300-f64", "shapes-f32", "chain-f64", "lattice-f32", "one-cell-f64",
                                  "asymmetric-last-f32", "asymmetric-first-negative-f64", "asymmetric-last-nan-f32"])
def test_model_equals_the_plain_groups_where_nothing_is_outside(name):
    case = gg.cases()[name]
    for ask in case.asks:
        model = gg.model_groups_grid(case.P, case.R, case.grid(ask), ask[3], ask[4])
        if model["outside"] == 0:
            gc.assert_same(model, gc.model_groups(case.P, case.R, ask[3], ask[4]), "%s %r" % (name, ask))
        else:
            inside = gg.inside_of(case.P, case.grid(ask))
            assert np.array_equal(model["label"][~inside], np.flatnonzero(~inside))      # outside: its own group
            assert model["n_groups"] >= model["outside"]
    assert any(gg.model_groups_grid(case.P, case.R, case.grid(a), a[3], a[4])["outside"] == 0 for a in case.asks)


@pytest.mark.parametrize("name", gg.case_names("bodies-"))
def test_edge_cases_are_what_the_gpu_tests_take_them_for(name):
    case = gg.cases()[name]
    n = len(case.R)
    full, one, part = (gg.model_groups_grid(case.P, case.R, case.grid(a), a[3], a[4]) for a in case.asks)
    gg.assert_same(full, one, name)
    if n >= 63:
        assert 1 < full["n_groups"] < n and full["largest"] > 2                       # groups of mixed size
        assert 0 < part["outside"] < n and not np.array_equal(part["label"], full["label"])


def test_special_cases_are_what_the_gpu_tests_take_them_for():
    for tag in wc.DTYPES:
        chain = gg.cases()["chain-" + tag]
        for ask in chain.asks:
            m = gg.model_groups_grid(chain.P, chain.R, chain.grid(ask), ask[3], ask[4])
            assert (m["n_groups"], m["largest"]) == ((1, 300) if ask[3] == 0.5 else (300, 1)) and m["outside"] == 0
        lat = gg.cases()["lattice-" + tag]
        for ask in lat.asks:
            m = gg.model_groups_grid(lat.P, lat.R, lat.grid(ask), ask[3], ask[4])
            assert (m["n_groups"], m["largest"]) == ((1, 289) if ask[3] == 1.0 else (289, 1)) and m["outside"] == 0
        for where in ("first", "last"):
            plain = gg.cases()["asymmetric-%s-%s" % (where, tag)]
            withnan = gg.cases()["asymmetric-%s-nan-%s" % (where, tag)]
            a = gg.model_groups_grid(plain.P, plain.R, plain.grid(plain.asks[0]), 0.0, 1.0)
            b = gg.model_groups_grid(withnan.P, withnan.R, withnan.grid(withnan.asks[0]), 0.0, 1.0)
            n = len(plain.R)
            assert np.array_equal(b["label"][:n], a["label"]) and b["label"][n] == n and b["inside"] == n + 1
            big = 0 if where == "first" else n - 1
            assert (a["label"] == a["label"][big]).sum() == a["largest"] > 50
            pair = (n - 2, n - 1) if where == "first" else (n - 3, n - 2)
            assert a["label"][pair[1]] == a["label"][pair[0]] != a["label"][big]      # the two equal bodies, across cells
            assert abs(int(plain.P[pair[0], 0]) - int(plain.P[pair[1], 0])) == 3 and plain.R[pair[0]] == plain.R[pair[1]]
    apart = gg.chain_links(np.float64)[1]
    assert apart == 0.5 - 2.0 ** -53                             # the next double below rounds s back up to 1


def test_overlap_consequence_in_the_model():
    """(0, 1), nothing outside: a body is alone in its group exactly where it overlaps nothing."""
    P, R, f = wc.state(300, np.float32)
    grid = cc.grid_of(8, 8, (0, f, 0, f))
    m = gg.model_groups_grid(P, R, grid, 0.0, 1.0)
    alone = np.bincount(m["label"], minlength=300)[m["label"]] == 1
    overlaps = wc.model_within(P, R, grid, np.inf)["rows"]["overlaps"]
    assert np.array_equal(alone, overlaps == 0) and 0 < alone.sum() < 300


# ---------------------------------------------------------------------------------------------------------------------
# 3. the host side of the product: argument checks before any device call, the helper grid
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_need_no_handle():
    import ppa_nbody_collisions_amd as nb
    grid = nb.make_grid(4, 4, (0, 1, 0, 1))
    label, info = np.zeros(8, dtype=np.int32), np.zeros(1, dtype=nb.GROUPS_GRID_INFO_DTYPE)
    data = lambda a: None if a is None else a.ctypes.data        # noqa: E731

    def one(handle, g, link, scale, lab, cap, inf):
        return nb.lib.nbody_get_groups_grid(handle, data(g), link, scale, data(lab), cap, data(inf))

    def batch(handle, g, link, scale, lab, cap, inf):
        return nb.lib.nbody_batch_get_groups_grid(handle, data(g), link, scale, data(lab), data(inf))
    for fn in (one, batch):
        def call(g=grid, link=1.0, scale=1.0, lab=label, cap=8, inf=info, handle=None):
            return fn(handle, g, link, scale, lab, cap, inf)
        assert call() == INVALID                                 # a NULL handle, everything else in order
        for bad in (dict(g=None), dict(link=np.nan), dict(link=-1.0), dict(link=-np.inf), dict(scale=np.nan), dict(scale=-1.0),
                    dict(scale=np.inf), dict(lab=None), dict(inf=None), dict(g=nb.make_grid(0, 4, (0, 1, 0, 1))),
                    dict(g=nb.make_grid(2048, 1024, (0, 1, 0, 1))), dict(g=nb.make_grid(4, 4, (0, 0, 0, 1))),
                    dict(g=nb.make_grid(4, 4, (np.nan, 1, 0, 1))), dict(g=nb.make_grid(4, 4, (1, 0, 0, 1)))):
            assert call(**bad) == INVALID, bad
            assert not label.any() and not info.view(np.uint8).any()
    assert one(None, grid, 1.0, 1.0, label, -1, info) == INVALID
    assert nb.GROUPS_GRID_INFO_DTYPE.itemsize == 24 and nb.GROUPS_GRID_INFO_DTYPE.names == gg.INFO_DTYPE.names


def test_groups_grid_helper():
    import ppa_nbody_collisions_amd as nb
    g = nb.groups_grid((100, 50), 3.0, 1.0, 2.0)                 # reach 1 * 2 * 2 + 3 = 7
    assert tuple(g[0]) == tuple(nb.within_grid((100, 50), 7.0)[0]) and (g["nx"][0], g["ny"][0]) == (28, 14)
    assert nb.groups_grid((100, 50), 0.0, 0.0, 5.0)["nx"][0] == 1024 and nb.groups_grid((100, 50), 3.0, 1.0, 2.0, most=8)["nx"][0] == 8
    assert nb.groups_grid((100, 50), np.inf, 1.0, 2.0)["nx"][0] == 1
