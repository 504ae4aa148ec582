"""Radius queries on the cell list (nbody_get_within, nbody_batch_get_within; Stepper.within, StepperGroup.within,
StepperBatch.within) on the MI355X: the sources within h of every body or point, the nearest of them, the overlapping ones
and the neighbour lists.

Every output is an integer, a minimum under a total order or a sorted list, and the definition has no fma and rounds every
operation on its own, so the numpy model of within_cases.py - brute force over all sources - restates it bit for bit: zero
tolerance throughout, against the model and product against product (neighbors, pair_counts, another grid, another rank, a
batch against a Stepper holding the same state).  test_within_cases_cpu.py holds, for every case used here, that the cells
the device looks at include every near source."""
import numpy as np
import pytest

import neighbor_cases as nc
import sharded_cases as sc
import within_cases as wc
from test_gpu_batch import params_of
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISION_OF = {np.float32: 0, np.float64: 1}


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, R, precision):
    n = len(P)
    return nb.BodiesData.from_arrays(P, np.zeros((n, 2)), np.ones(n), R, precision) if n else nb.BodiesData(0, precision)


def run_case(nb, case, check=None):
    """Every ask of the case, with lists, against the model; -> the results."""
    precision = PRECISION_OF[case.dtype]
    got_all = []
    with small_stepper(nb, precision, len(case.P)) as st:
        st.upload(bodies_of(nb, case.P, case.R, precision))
        for ask in case.asks:
            nx, ny, bounds, h2 = ask
            got = st.within(h2, case.points, grid=nb.make_grid(nx, ny, bounds), squared=True, lists=True)
            want = wc.model_within(case.P, case.R, got["grid"], h2, case.points)
            wc.assert_same(got, want, "%s %r" % (case.name, ask))
            assert wc.lists_consistent(got)
            plain = st.within(h2, case.points, grid=nb.make_grid(nx, ny, bounds), squared=True)
            assert "list" not in plain and plain["rows"].tobytes() == got["rows"].tobytes() and plain["info"] == got["info"]
            got_all.append(got)
    return got_all


# ---------------------------------------------------------------------------------------------------------------------
# 1. workgroup and wave edges: 8 x 8, 1 x 1 and a grid that leaves bodies - rows - outside
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.case_names("bodies-"))
def test_body_edges(nb, name):
    case = wc.cases()[name]
    n = len(case.P)
    full, one, part = run_case(nb, case)
    assert full["info"]["inside"] == n == one["info"]["inside"] and full["info"]["rows"] == n == part["info"]["rows"]
    assert (one["rows"]["cell"] == 0).all()
    wc.assert_same(full, one, name + ": 8 x 8 against 1 x 1", cell=False)
    if n >= 63:
        assert 0 < part["info"]["outside"] < n and (part["rows"]["cell"] == -1).sum() == part["info"]["outside"]
        assert part["rows"]["count"][part["rows"]["cell"] == -1].any()       # rows outside the grid that have sources near
        assert full["info"]["total"] > part["info"]["total"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. grid shapes, radii, the lattice, one cell, points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.case_names("shapes-"))
def test_grid_shapes(nb, name):
    results = run_case(nb, wc.cases()[name])
    for got in results[1:]:                                      # every grid holds every body: the same bytes but for `cell`
        wc.assert_same(got, results[0], name, cell=False)
    assert results[0]["info"]["outside"] == 0 and results[0]["info"]["total"] > 0


@pytest.mark.parametrize("name", wc.case_names("radii-"))
def test_radii(nb, name):
    case = wc.cases()[name]
    n = len(case.P)
    zero, small, wide, beyond, inf = run_case(nb, case)
    assert zero["info"]["total"] == 2 and zero["rows"]["count"][7] == 1 and zero["rows"]["index"][7] == n - 100   # the coincident pair
    assert zero["rows"]["d2"][n - 100] == 0.0 and zero["rows"]["index"][n - 100] == 7
    assert 2 < small["info"]["total"] < wide["info"]["total"] < beyond["info"]["total"] == n * (n - 1) == inf["info"]["total"]
    assert beyond["rows"].tobytes() == inf["rows"].tobytes() and np.array_equal(beyond["list"], inf["list"])


@pytest.mark.parametrize("name", wc.case_names("lattice-"))
def test_lattice_ties_and_boundaries(nb, name):
    """Spacing = cell side = h: the four nearest of an interior body are at d2 == h2 exactly, in four other cells, and the
    lowest index wins although the cell below is not the first the walk visits."""
    on, off = run_case(nb, wc.cases()[name])
    side = wc.LATTICE_SIDE
    for got in (on, off):
        assert np.array_equal(got["rows"]["index"], nc.lattice_expected(side)) and (got["rows"]["d2"] == 1.0).all()
        assert got["info"]["largest"] == 4 and got["info"]["largest_row"] == side + 1 and got["info"]["inside"] == side * side
    assert np.array_equal(on["rows"]["cell"], np.arange(side * side))               # on the boundaries: the cell above and right


@pytest.mark.parametrize("name", wc.case_names("one-cell-"))
def test_every_body_in_one_cell(nb, name):
    near, inf = run_case(nb, wc.cases()[name])
    assert (near["rows"]["cell"] == 18).all() and inf["info"]["total"] == 385 * 384
    assert 0 < near["info"]["total"] < inf["info"]["total"]


@pytest.mark.parametrize("name", wc.case_names("points-"))
def test_probe_points(nb, name):
    case = wc.cases()[name]
    matched, part, inf = run_case(nb, case)
    m = len(case.points)
    assert matched["info"]["rows"] == m == len(matched["rows"]) and matched["info"]["n"] == len(case.P)
    for got in (matched, part, inf):                             # the NaN point and the two 1e200 points see nothing near
        assert not got["rows"]["count"][-3:].any() or got is inf
        assert (got["rows"]["cell"][-3:] == -1).all()
    assert inf["rows"]["count"][-3] == 0 and (inf["rows"]["count"][-2:] == len(case.P)).all()
    assert (inf["rows"]["index"][-2:] == -1).all() and np.isinf(inf["rows"]["d2"][-2:]).all()     # +inf is counted, never nearest
    assert (matched["rows"]["d2"][:m // 4] == 0.0).any()         # points ON bodies


# ---------------------------------------------------------------------------------------------------------------------
# 3. product against product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_against_neighbors_and_pair_counts(nb, dtype):
    P, R, f = wc.state(300, dtype, coincident=True)
    pts = wc.awkward_points(P, f)[:-3]
    precision = PRECISION_OF[dtype]
    h = 0.1 * f
    edges2 = np.array([0.0, np.nextafter(h * h, np.inf)])
    with small_stepper(nb, precision, 300) as st:
        st.upload(bodies_of(nb, P, R, precision))
        for points in (None, pts):
            a = st.within(h * h, points, grid=nb.make_grid(16, 16, (0, f, 0, f)), squared=True, lists=True)
            b = st.within(h * h, points, grid=nb.make_grid(5, 3, (-1, 2 * f, -1, 2 * f)), squared=True, lists=True)
            assert a["info"]["outside"] == 0 == b["info"]["outside"]
            wc.assert_same(a, b, "two grids", cell=False)
            for fld in ("d2", "index", "count", "overlaps"):
                assert np.ascontiguousarray(a["rows"][fld]).tobytes() == np.ascontiguousarray(b["rows"][fld]).tobytes(), fld
            assert a["start"].tobytes() == b["start"].tobytes() and a["list"].tobytes() == b["list"].tobytes()
            pairs = st.pair_counts(edges2, points, squared=True)
            assert a["info"]["total"] == (2 if points is None else 1) * int(pairs["counts"][0]) > 0
            inf = st.within(np.inf, points, grid=nb.make_grid(16, 16, (0, f, 0, f)))
            nbr = st.neighbors(points)
            for fld in ("d2", "index", "overlaps"):
                assert np.ascontiguousarray(inf["rows"][fld]).tobytes() == np.ascontiguousarray(nbr[fld]).tobytes(), fld
        by_radius = st.within(h, grid=nb.make_grid(16, 16, (0, f, 0, f)))           # radius, squared by the wrapper
        assert by_radius["info"]["total"] == st.within(h * h, grid=nb.make_grid(16, 16, (0, f, 0, f)), squared=True)["info"]["total"]


def test_default_grid_after_steps_and_state_preservation(nb):
    """n = 1024 in a dense field: bodies merge, the count comes from the device; the default grid is within_grid over the
    field.  A step after the queries gives the bits of a run without them."""
    n = 1024
    cfg, b = dense_bodies(nb, n, seed=7003)
    w = float(dense_field(n))
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as ref:
        st.upload(b)
        ref.upload(b)
        st.step(2)
        ref.step(2)
        d = st.download()
        P, R = nc.widen(d)
        assert len(P) < n
        h = 0.0625 * w                                            # exact: 32 cells of side h over the field's 2 w
        got = st.within(h, lists=True)
        assert tuple(got["grid"]) == tuple(nb.within_grid((w, w), h)[0]) and got["grid"]["nx"] == 32 == got["grid"]["ny"]
        wc.assert_same(got, wc.model_within(P, R, got["grid"], h * h), "after 2 steps")
        assert got["info"]["n"] == len(P) and got["info"]["total"] > 0
        st.within(0.3 * w, points=P[:50] + 1.0)
        st.step(2)
        ref.step(2)
        assert st.download().block.tobytes() == ref.download().block.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the lists' capacity
# ---------------------------------------------------------------------------------------------------------------------
def test_list_capacity(nb):
    P, R, f = wc.state(300, np.float32)
    grid = nb.make_grid(8, 8, (0, f, 0, f))
    h2 = (f / 8) ** 2
    want = wc.model_within(P, R, grid[0], h2)
    total = want["info"]["total"]
    assert total > 300
    out, info = np.zeros(300, dtype=nb.WITHIN_DTYPE), np.zeros(1, dtype=nb.WITHIN_INFO_DTYPE)
    start, lst = np.full(301, -5, dtype=np.int64), np.full(total + 3, -5, dtype=np.int32)
    with small_stepper(nb, 0, 300) as st:
        call = lambda m, s, l, cap: nb.lib.nbody_get_within(st._ctx, grid.ctypes.data, h2, None, m, out.ctypes.data, s, l, cap,  # noqa: E731,E741
                                                            info.ctypes.data)
        assert call(300, None, None, 0) == STATE_ERR             # before an upload
        st.upload(bodies_of(nb, P, R, 0))
        assert call(299, None, None, 0) == CAPACITY_ERR and not out.view(np.uint8).any()      # no room for the rows
        assert call(300, start.ctypes.data, lst.ctypes.data, total - 1) == CAPACITY_ERR
        assert (lst == -5).all()                                 # the list untouched; out, start and info complete
        assert {k: int(info[k][0]) for k in wc.INFO_FIELDS} == want["info"] and start[300] == total
        assert np.array_equal(start, want["start"]) and out.tobytes() == want["rows"].tobytes()
        assert call(300, start.ctypes.data, lst.ctypes.data, total) == 0                      # the retry
        assert np.array_equal(lst[:total], want["list"]) and (lst[total:] == -5).all()
        assert call(300, start.ctypes.data, None, 0) == 0 and start[300] == total             # start alone
        got = st.within(h2, grid=grid, squared=True, lists=True)                              # the wrapper fits its guess
        wc.assert_same(got, want, "through the wrapper")
        wide = st.within(np.inf, grid=grid, lists=True)          # 89700 entries, more than the wrapper's first guess
        assert wide["info"]["total"] == 300 * 299 == len(wide["list"]) > 16 * 300
        assert np.array_equal(wide["list"].reshape(300, 299)[5], np.delete(np.arange(300), 5))


# ---------------------------------------------------------------------------------------------------------------------
# 5. batches and groups
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [0, 1, 64, 257, 300]


def test_batch_equals_steppers_and_model(nb):
    cap = 300
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        cfg, bd = dense_bodies(nb, max(n, 1), seed=60 + s)
        cfgs.append(cfg)
        bodies.append(bd if n else nb.BodiesData(0))
    w = float(dense_field(cap))
    grid = nb.make_grid(12, 9, (-w, w, -w / 2, w))              # leaves bodies outside
    pts = np.random.default_rng(5).uniform(-w, w, size=(70, 2))
    with nb.StepperBatch(len(BATCH_SIZES), cap, params=[params_of(c) for c in cfgs]) as batch:
        batch.upload(bodies)
        assert batch.counts().tolist() == BATCH_SIZES
        for points in (None, pts):
            got = batch.within(0.2 * w, points, grid=grid, lists=True)
            assert len(got) == len(BATCH_SIZES)
            for s, n in enumerate(BATCH_SIZES):
                state = batch.download(s)
                with nb.Stepper(cfgs[s], capacity=cap) as one:    # a Stepper holding the same state
                    one.upload(state)
                    want = one.within(0.2 * w, points, grid=grid, lists=True)
                wc.assert_same(got[s], want, "system %d" % s)
                P, R = nc.widen(state)
                wc.assert_same(got[s], wc.model_within(P.reshape(-1, 2), R, grid[0], (0.2 * w) * (0.2 * w), points), "system %d, the model" % s)
                assert got[s]["info"]["n"] == n and got[s]["info"]["rows"] == (n if points is None else len(pts))
            assert got[-1]["info"]["total"] > 0 and got[-1]["info"]["outside"] > 0
        dflt = batch.within(0.2 * w, lists=True)                  # the default grid: over the field of system 0
        for s in range(len(BATCH_SIZES)):
            P, R = nc.widen(batch.download(s))
            wc.assert_same(dflt[s], wc.model_within(P.reshape(-1, 2), R, dflt[s]["grid"], (0.2 * w) * (0.2 * w)), "default grid, system %d" % s)


def test_every_rank_of_a_group(nb):
    world, n = 2, 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    w = float(dense_field(n))
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    try:
        grp.upload(b)
        grp.step(sc.LAG + 2)                                      # past the exchange lag
        P, R = nc.widen(grp.download())
        assert len(P) < n
        want = wc.model_within(P, R, nb.within_grid((w, w), 0.1 * w)[0], (0.1 * w) * (0.1 * w))
        assert want["info"]["total"] > 0
        rank0 = grp.within(0.1 * w, lists=True, rank=0)
        rank1 = grp.within(0.1 * w, lists=True, rank=1)           # each on its own: not collective
        wc.assert_same(rank0, want, "rank 0")
        wc.assert_same(rank1, rank0, "rank 1 against rank 0")
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5b. the row scan past one block of 1024 rows and past one trip of 256 blocks (within_cases.scan_cases)
# ---------------------------------------------------------------------------------------------------------------------
def scan_ask(nb, case):
    nx, ny, bounds, h2 = case.asks[0]
    return nb.make_grid(nx, ny, bounds), h2


@pytest.mark.parametrize("name", wc.scan_case_names("scan-bodies-"))
def test_row_scan_across_blocks(nb, name):
    """Rows either side of one and two blocks: start[row] = the block's offset + the prefix inside the block."""
    case, want = wc.scan_cases()[name], wc.scan_reference(name)
    precision = PRECISION_OF[case.dtype]
    grid, h2 = scan_ask(nb, case)
    with small_stepper(nb, precision, len(case.P)) as st:
        st.upload(bodies_of(nb, case.P, case.R, precision))
        got = st.within(h2, grid=grid, squared=True, lists=True)
    wc.assert_same(got, want, name, lists=True)
    assert got["start"][len(case.P)] == want["info"]["total"] > len(case.P)


def test_row_scan_batch_with_an_empty_block(nb):
    """Two systems `stride` = 1025 apart holding 1025 and 3 bodies: two blocks each, the second system's block 1 has no row."""
    names = wc.scan_case_names("scan-batch-")
    cases = [wc.scan_cases()[k] for k in names]
    assert tuple(len(c.P) for c in cases) == wc.SCAN_BATCH
    grid, h2 = scan_ask(nb, cases[0])
    with nb.StepperBatch(len(cases), wc.SCAN_BATCH[0], params=[(0.2, 0.1, 100, 100)] * len(cases)) as batch:
        batch.upload([bodies_of(nb, c.P, c.R, 0) for c in cases])
        got = batch.within(h2, grid=grid, squared=True, lists=True)
    for s, name in enumerate(names):
        wc.assert_same(got[s], wc.scan_reference(name), name, lists=True)
    assert got[0]["info"]["total"] > wc.SCAN_BLOCK_ROWS and got[1]["info"]["rows"] == 3


def test_row_scan_second_trip_of_the_block_scan(nb):
    """m = 256 * 1024 + 1025 points: 258 blocks, so the block scan makes a second trip, of one full and one partial block."""
    name = "scan-points-f32"
    case, want = wc.scan_cases()[name], wc.scan_reference(name)
    m = len(case.points)
    assert m == wc.SCAN_POINTS and -(-m // wc.SCAN_BLOCK_ROWS) == wc.SCAN_TRIP_BLOCKS + 2
    grid, h2 = scan_ask(nb, case)
    with small_stepper(nb, 0, len(case.P)) as st:
        st.upload(bodies_of(nb, case.P, case.R, 0))
        got = st.within(h2, case.points, grid=grid, squared=True, lists=True)
    assert got["start"][m] == want["start"][m] == want["info"]["total"] == got["info"]["total"] > m
    assert got["info"]["largest_row"] == want["info"]["largest_row"]
    for row in wc.scan_sample(m):
        a, b = (r["list"][r["start"][row]:r["start"][row + 1]] for r in (got, want))
        assert np.array_equal(a, b), (row, a, b)
    wc.assert_same(got, want, name, lists=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. invalid arguments, each found before the handle is looked at
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(nb):
    P, R, f = wc.state(64, np.float32)
    grid = nb.make_grid(4, 4, (0, f, 0, f))
    out, info = np.zeros(64, dtype=nb.WITHIN_DTYPE), np.zeros(1, dtype=nb.WITHIN_INFO_DTYPE)
    start, lst = np.zeros(65, dtype=np.int64), np.zeros(64, dtype=np.int32)
    pts = np.zeros((4, 2))
    data = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    with small_stepper(nb, 0, 64) as st:                          # never uploaded: a valid call would be NBODY_ERR_STATE
        def call(g=grid, h2=1.0, p=None, m=64, o=out, s=start, l=lst, cap=64, i=info, handle=st._ctx):   # noqa: E741
            return nb.lib.nbody_get_within(handle, data(g), h2, data(p), m, data(o), data(s), data(l), cap, data(i))
        assert call() == STATE_ERR
        bad_grids = [nb.make_grid(0, 4, (0, 1, 0, 1)), nb.make_grid(4, -1, (0, 1, 0, 1)), nb.make_grid(2048, 1024, (0, 1, 0, 1)),
                     nb.make_grid(4, 4, (0, 0, 0, 1)), nb.make_grid(4, 4, (np.nan, 1, 0, 1)), nb.make_grid(4, 4, (1, 0, 0, 1))]
        for bad in ([dict(g=None), dict(h2=np.nan), dict(h2=-1.0), dict(h2=-np.inf), dict(s=None), dict(cap=-1), dict(m=-1),
                     dict(p=pts, m=-1), dict(o=None), dict(i=None), dict(handle=None)] + [dict(g=g) for g in bad_grids]):
            assert call(**bad) == INVALID, bad
        assert not out.view(np.uint8).any() and not info.view(np.uint8).any()
        with pytest.raises(nb.NbodyError) as e:
            st.within(-1.0, grid=grid, squared=True)
        assert e.value.status == INVALID
        st.upload(bodies_of(nb, P, R, 0))                         # and the handle goes on
        assert st.within(0.25 * f, grid=grid)["info"]["n"] == 64
