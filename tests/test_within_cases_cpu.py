"""The model of the radius queries against the definition as a scalar loop, the window rule's superset property on every case
of the GPU tests, what follows from the definition - held in the model - the argument checks that need no device and
within_grid.  No GPU."""
import numpy as np
import pytest

import cell_cases as cc
import neighbor_cases as nc
import pair_cases as pc
import within_cases as wc

INVALID = -1


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the scalar loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bodies-65-f32", "radii-f64", "lattice-f32", "points-f32", "points-f64", "one-cell-f32"])
def test_model_equals_the_scalar_loop(name):
    case = wc.cases()[name]
    for ask in case.asks:
        model = wc.model_within(case.P, case.R, case.grid(ask), ask[3], case.points)
        loop = wc.loop_within(case.P, case.R, case.grid(ask), ask[3], case.points)
        wc.assert_same(model, loop, "%s %r" % (name, ask))
        assert wc.lists_consistent(model)


def test_model_on_awkward_values():
    """A NaN d2 is never near, a +inf d2 is counted at h2 = +inf and never the nearest, a body outside is a row and no source."""
    P = np.array([[1.0, 1.0], [np.nan, 1.0], [1e200, 1.0], [1.5, 1.0], [9.0, 9.0], [1.5, 1.0]])
    R = np.full(len(P), 0.3)
    grid = cc.grid_of(8, 8, (0, 8, 0, 8))
    for h2 in (0.0, 0.25, np.inf):
        model, loop = wc.model_within(P, R, grid, h2), wc.loop_within(P, R, grid, h2)
        wc.assert_same(model, loop, "h2 %r" % h2)
        assert model["info"]["inside"] == 3 and model["info"]["outside"] == 3
    assert model["rows"]["count"].tolist() == [2, 0, 3, 2, 3, 2]                   # h2 = +inf: the NaN row sees nothing
    assert model["rows"]["index"].tolist() == [3, -1, -1, 5, 3, 3] and model["rows"]["cell"].tolist() == [9, -1, -1, 9, -1, 9]
    assert np.isinf(model["rows"]["d2"][2]) and model["list"][model["start"][2]:model["start"][3]].tolist() == [0, 3, 5]
    zero = wc.model_within(P, R, grid, 0.0)
    assert zero["rows"]["count"].tolist() == [0, 0, 0, 1, 0, 1] and zero["rows"]["overlaps"].tolist() == [0, 0, 0, 1, 0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the window rule: what the device looks at includes every near source
# ---------------------------------------------------------------------------------------------------------------------
def near_mask(case, grid, h2):
    P, xy = case.P, case.rows_xy()
    with np.errstate(over="ignore", invalid="ignore"):
        dx = P[None, :, 0] - xy[:, None, 0]
        dy = P[None, :, 1] - xy[:, None, 1]
        near = (cc.cell_index(P, grid) >= 0)[None, :] & ((dx * dx) + (dy * dy) <= h2)
    return near


@pytest.mark.parametrize("name", wc.case_names())
def test_window_holds_every_near_source(name):
    case = wc.cases()[name]
    for ask in case.asks:
        grid, h2 = case.grid(ask), ask[3]
        near = near_mask(case, grid, h2)
        cand = wc.window_model(case.P, grid, h2, case.rows_xy())
        missed = np.argwhere(near & ~cand)
        assert len(missed) == 0, (name, ask, "%d near pairs outside the window, first %s" % (len(missed), missed[0]))
        if np.isinf(h2):
            finite = np.isfinite(case.rows_xy()).all(axis=1)
            assert cand[finite].sum() == finite.sum() * int((cc.cell_index(case.P, grid) >= 0).sum())


def test_window_is_a_window():
    """The rule does cut: on the matched grid a row looks at a few cells, not at all of them; a far row at none."""
    case = wc.cases()["radii-f32"]
    ask = case.asks[1]                                           # h = 0.3 cell on 16 x 16
    cand = wc.window_model(case.P, case.grid(ask), ask[3], case.P)
    assert 0 < cand.sum() < 0.05 * cand.size
    pts = wc.cases()["points-f64"]
    ask = pts.asks[0]
    cand = wc.window_model(pts.P, pts.grid(ask), ask[3], pts.points)
    assert not cand[-1].any() and not cand[-2].any()             # the 1e200 points: proved empty by a compare
    f = cc.tenth_field(300)                                      # the (NaN, f/2) point: every column of its rows of cells
    along = np.stack([(np.arange(16) + 0.5) * f / 16, np.full(16, 0.5 * f)], axis=1)
    band = wc.window_model(pts.P, pts.grid(ask), ask[3], along).any(axis=0)
    assert np.array_equal(cand[-3], band) and 16 < band.sum() < len(pts.P)
    assert not cand[-6].any()                                    # 1e6 fields away


def test_window_on_the_lattice_and_at_awkward_rows():
    """Cell side = spacing = h at offsets 0 and 0.1: the d2 == h2 pairs sit in the neighbouring cells; rows a long way off,
    with h reaching them or not; a grid too fine for the margin's proof falls back to every cell."""
    case = wc.cases()["lattice-f64"]
    for ask in case.asks:
        grid = case.grid(ask)
        assert grid[2] == 1.0 and grid[3] == 1.0
        near = near_mask(case, grid, ask[3])
        assert near.sum() > 4 * len(case.P)                      # itself and up to four at d2 == h2
        assert not (near & ~wc.window_model(case.P, grid, ask[3], case.P)).any()
    P, _, f = wc.state(300, np.float64)
    far = np.array([[1e6 * f, 0.5 * f], [1e200, 0.0], [np.nan, np.nan], [-1e6 * f, 1e6 * f], [0.5 * f, 1e300]])
    for h2 in (0.0, 1.0, (1e6 * f) ** 2, 1e300, np.inf):
        grid = cc.grid_of(16, 16, (0, f, 0, f))
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy = P[None, :, 0] - far[:, None, 0], P[None, :, 1] - far[:, None, 1]
            near = (dx * dx) + (dy * dy) <= h2
        assert not (near & ~wc.window_model(P, grid, h2, far)).any(), h2
    tiny = np.array([[0.0, 0.0], [2.0 ** -1001, 0.0]])          # dx*dx underflows to 0: near at h2 = 0, 2^19 cells apart
    fine = (0.0, 0.0, 2.0 ** 1020, 1.0, 1 << 20, 1)
    assert wc.model_within(tiny, np.zeros(2), fine, 0.0)["rows"]["count"].tolist() == [1, 1]
    assert wc.window_model(tiny, fine, 0.0, tiny).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2b. the cases of the row scan: their shapes, their references inside the budget, the window rule on them
# ---------------------------------------------------------------------------------------------------------------------
def test_scan_cases_cross_the_blocks_and_the_trip():
    """What the cases are for, held here: rows either side of one and two blocks, a batch whose second system has an empty
    block 1, and points that need a second trip of the block scan, of one full and one partial block."""
    B, T = wc.SCAN_BLOCK_ROWS, wc.SCAN_TRIP_BLOCKS
    assert sorted(n for _, n in wc.SCAN_BODIES) == [B - 1, B, B + 1, B + 1, 2 * B + 1]
    assert wc.SCAN_BATCH == (B + 1, 3) and [len(wc.scan_cases()[k].P) for k in wc.scan_case_names("scan-batch-")] == [B + 1, 3]
    m = len(wc.scan_cases()["scan-points-f32"].points)
    blocks = -(-m // B)
    assert m == T * B + 1025 and blocks == T + 2 and m - (T + 1) * B == 1 and len(wc.scan_cases()["scan-points-f32"].P) == 65
    sample = wc.scan_sample(m)
    assert len(sample) == 64 == len(set(sample.tolist())) and sample[0] == 0 and sample[-1] == m - 1
    for edge in (B, 2 * B, (T - 1) * B, T * B, (T + 1) * B):
        assert edge - 1 in sample and edge in sample, edge


def test_scan_references_within_budget():
    """A condition, not a measurement: no reference of the row-scan cases may take more than the suite's 10 s."""
    import large_cases as lg
    for name in wc.scan_case_names():
        ref = wc.scan_reference(name)
        assert wc.scan_reference(name) is ref                      # computed once
        assert ref["info"]["total"] == ref["start"][-1] == len(ref["list"]) > 0
    print("seconds: " + "   ".join("%s %.1f" % (name, wc.SCAN_TIMES[name]) for name in wc.scan_case_names()))
    for name in wc.scan_case_names():
        assert wc.SCAN_TIMES[name] <= lg.BUDGET_S, (name, wc.SCAN_TIMES[name])
    with pytest.raises(ValueError):
        wc.scan_reference("scan-points-f32")["start"][0] = 1       # read-only


@pytest.mark.parametrize("name", wc.scan_case_names())
def test_window_holds_every_near_source_of_the_scan_cases(name):
    case = wc.scan_cases()[name]
    grid, h2 = case.grid(case.asks[0]), case.asks[0][3]
    xy = case.rows_xy()
    for a in range(0, len(xy), 1 << 16):                         # the points in slices: (rows, sources) masks
        rows = xy[a:a + (1 << 16)]
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy = case.P[None, :, 0] - rows[:, None, 0], case.P[None, :, 1] - rows[:, None, 1]
            near = (cc.cell_index(case.P, grid) >= 0)[None, :] & ((dx * dx) + (dy * dy) <= h2)
        missed = np.argwhere(near & ~wc.window_model(case.P, grid, h2, rows))
        assert len(missed) == 0, (name, "%d near pairs outside the window, first %s" % (len(missed), missed[0]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. what follows from the definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_consequences_in_the_model(dtype):
    P, R, f = wc.state(300, dtype, coincident=True)
    pts = wc.awkward_points(P, f)[:-3]                           # finite points
    everything = cc.grid_of(5, 3, (-1, 2 * f, -1, 2 * f))
    other = cc.grid_of(16, 16, (0, f, 0, f))
    h2 = (0.1 * f) ** 2
    for points in (None, pts):
        a, b = wc.model_within(P, R, everything, h2, points), wc.model_within(P, R, other, h2, points)
        assert a["info"]["outside"] == 0 == b["info"]["outside"]
        wc.assert_same(a, b, "two grids that hold every body", cell=False)
        assert not np.array_equal(a["rows"]["cell"], b["rows"]["cell"])
        # h2 = +inf: the bits of the neighbour queries
        inf = wc.model_within(P, R, other, np.inf, points)
        want = nc.model_neighbors(P, R, points=points)
        for fld in ("index", "overlaps"):
            assert np.array_equal(inf["rows"][fld], want[fld]), fld
        assert np.array_equal(cc.bits(inf["rows"]["d2"]), cc.bits(want["d2"]))
        assert (inf["rows"]["count"] == len(P) - (points is None)).all()
        # the pair counts with edges2 = {0, nextafter(h2, +inf)}: d2 < nextafter(h2) is d2 <= h2
        pairs = pc.model_pair_counts(P, [0.0, np.nextafter(h2, np.inf)], points)
        assert a["info"]["total"] == (2 if points is None else 1) * int(pairs["counts"][0]) > 0
    part = wc.model_within(P, R, cc.grid_of(8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f)), h2)
    own = wc.model_within(P, R, other, h2)
    assert 0 < part["info"]["outside"] < 300 and 0 < part["info"]["total"] < own["info"]["total"]
    assert part["rows"]["count"][part["info"]["largest_row"]] == part["info"]["largest"] == part["rows"]["count"].max()


def test_lattice_ties_go_to_the_lowest_index():
    case = wc.cases()["lattice-f64"]
    model = wc.model_within(case.P, case.R, case.grid(case.asks[0]), 1.0)
    assert np.array_equal(model["rows"]["index"], nc.lattice_expected(wc.LATTICE_SIDE))
    assert (model["rows"]["d2"] == 1.0).all() and model["rows"]["count"].max() == 4 and model["rows"]["count"].min() == 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. the host side of the product: argument checks before any device call, within_grid
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_need_no_handle():
    import ppa_nbody_collisions_amd as nb
    grid = nb.make_grid(4, 4, (0, 1, 0, 1))
    out, info = np.zeros(4, dtype=nb.WITHIN_DTYPE), np.zeros(1, dtype=nb.WITHIN_INFO_DTYPE)
    start, lst = np.zeros(5, dtype=np.int64), np.zeros(8, dtype=np.int32)
    pts = np.zeros((4, 2))
    for fn in (nb.lib.nbody_get_within, nb.lib.nbody_batch_get_within):
        def call(g=grid, h2=1.0, p=pts, m=4, o=out, s=start, l=lst, cap=8, i=info, handle=None):   # noqa: E741
            data = lambda a: None if a is None else a.ctypes.data                            # noqa: E731
            return fn(handle, data(g), h2, data(p), m, data(o), data(s), data(l), cap, data(i))
        assert call() == INVALID                                 # a NULL handle, everything else in order
        for bad in (dict(g=None), dict(h2=np.nan), dict(h2=-1.0), dict(h2=-np.inf), dict(s=None), dict(cap=-1), dict(m=-1),
                    dict(o=None), dict(i=None), dict(g=nb.make_grid(0, 4, (0, 1, 0, 1))), dict(g=nb.make_grid(2048, 1024, (0, 1, 0, 1))),
                    dict(g=nb.make_grid(4, 4, (0, 0, 0, 1))), dict(g=nb.make_grid(4, 4, (np.nan, 1, 0, 1)))):
            assert call(**bad) == INVALID, bad
            assert not out.view(np.uint8).any() and not info.view(np.uint8).any()


def test_within_grid():
    import ppa_nbody_collisions_amd as nb
    g = nb.within_grid((100, 50), 7.0)
    assert (g["nx"][0], g["ny"][0]) == (28, 14) and (g["x0"][0], g["y0"][0]) == (-100.0, -50.0)
    assert 1.0 / g["sx"][0] >= 7.0 and 1.0 / g["sy"][0] >= 7.0   # cells no smaller than the radius
    assert tuple(nb.within_grid((100, 50), 49.0, squared=True)[0]) == tuple(g[0])
    assert nb.within_grid((100, 50), 0.0)["nx"][0] == 1024 == nb.within_grid((100, 50), 1e-9)["ny"][0]
    assert nb.within_grid((100, 50), np.inf)["nx"][0] == 1 == nb.within_grid((100, 50), 1e9)["ny"][0]
    assert nb.within_grid((100, 50), 7.0, most=8)["nx"][0] == 8
    assert nb.WITHIN_DTYPE.itemsize == 24 and nb.WITHIN_INFO_DTYPE.itemsize == 32
