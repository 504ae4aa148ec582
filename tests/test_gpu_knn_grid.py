"""The k nearest neighbours on the cell list (nbody_get_knn_grid, nbody_batch_get_knn_grid; Stepper.knn(grid=...),
StepperGroup.knn, StepperBatch.knn) on the MI355X.

The result is the first k of a set under a total order and the definition has no fma and rounds every operation on its own,
so the numpy model of knn_grid_cases.py restates it bit for bit, the rounds of the widening rule included: zero tolerance
throughout, against the model (d2, index and every field of info) and product against product - knn() without a grid,
within(lists=True), another grid, another rank, a batch against a Stepper holding the same state.  test_knn_grid_cases_cpu.py
holds, for every case used here, that the rule ends with the brute-force result."""
import numpy as np
import pytest

import knn_cases as kc
import knn_grid_cases as kg
import neighbor_cases as nc
import sharded_cases as sc
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


def cut_of(h2_max):
    return None if np.isinf(h2_max) else h2_max


def run_case(nb, name):
    """Every ask of the case against the model of the rule - d2, index and info - and against knn() without a grid,
    within(lists=True) and a second grid wherever the definition says they agree; -> the results."""
    case = kg.cases()[name]
    precision = PRECISION_OF[case.dtype]
    got_all = []
    lo, hi = float(np.nanmin(case.P)) - 1.0, float(np.nanmax(case.P)) + 1.0
    with small_stepper(nb, precision, len(case.P)) as st:
        st.upload(bodies_of(nb, case.P, case.R, precision))
        for a, ask in enumerate(case.asks):
            nx, ny, bounds, k, h0, h2_max = ask
            what = "%s %r" % (name, ask)
            grid = nb.make_grid(nx, ny, bounds)
            got = st.knn(k, case.points, grid=grid, h0=h0, max_radius=cut_of(h2_max), squared=True)
            ref = kg.reference(name, a)
            assert sorted(got) == ["d2", "grid", "index", "info"] and tuple(got["grid"]) == tuple(grid[0])
            kg.assert_same(got, ref, what)
            # entry 0 and the number of entries against the radius query on the same grid with h2 = h2_max
            w = st.within(h2_max, case.points, grid=grid, squared=True, lists=True)
            assert np.array_equal(kg.bits(got["d2"][:, 0]), kg.bits(w["rows"]["d2"])) and np.array_equal(got["index"][:, 0], w["rows"]["index"]), what
            if case.points is None or np.isfinite(h2_max):       # within counts a source at d2 = +inf where h2 is +inf
                assert np.array_equal((got["index"] >= 0).sum(axis=1), np.minimum(k, w["rows"]["count"])), what
                for r in range(0, len(w["rows"]), 37):           # the first k of the row's list, re-sorted by (d2, j)
                    lst = w["list"][w["start"][r]:w["start"][r + 1]]
                    order = lst[np.lexsort((lst, ref["pairs"][r, lst]))][:k]
                    assert got["index"][r, :len(order)].tolist() == order.tolist(), (what, r)
            if got["info"]["outside"] == 0:
                other = st.knn(k, case.points, grid=nb.make_grid(5, 3, (lo, hi, lo, hi)), max_radius=cut_of(h2_max), squared=True)
                assert other["info"]["outside"] == 0
                kg.assert_same(other, got, what + ": a second grid", info=False)
                if np.isinf(h2_max):                             # the bytes of the brute-force query
                    plain = st.knn(k, case.points)
                    assert plain["d2"].tobytes() == got["d2"].tobytes() and plain["index"].tobytes() == got["index"].tobytes(), what
            got_all.append(got)
    return got_all


# ---------------------------------------------------------------------------------------------------------------------
# 1. wave and workgroup edges: 8 x 8, 1 x 1 and a grid that leaves bodies - rows, not sources - outside
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kg.case_names("bodies-"))
def test_body_edges(nb, name):
    n = len(kg.cases()[name].P)
    full, one, part = run_case(nb, name)
    assert full["info"]["inside"] == n == one["info"]["inside"] and full["info"]["rows"] == n == part["info"]["rows"]
    assert one["info"]["rounds"] == 1 and one["info"]["widened"] == 0                   # 1 x 1: the whole grid at once
    if n >= 63:
        assert 0 < part["info"]["outside"] < n and len(part["d2"]) == n
        outside = kg.cc.cell_index(kg.cases()[name].P, part["grid"]) < 0
        assert (part["index"][outside, 0] >= 0).all()            # rows outside the grid have their k nearest
        assert not np.isin(part["index"], np.flatnonzero(outside)).any()                # and are nobody's source


# ---------------------------------------------------------------------------------------------------------------------
# 2. tiers, padding, ties, coincident bodies, many rounds, awkward points, the first radius, the cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kg.case_names("tiers-") + kg.case_names("padding-"))
def test_tiers_and_padding(nb, name):
    results = run_case(nb, name)
    case = kg.cases()[name]
    for got, ask in zip(results, case.asks):
        assert got["d2"].shape == (len(case.P), ask[3])
        kc.check_invariants(got, np.arange(len(case.P)))
    if name.startswith("tiers-"):
        for got in results[:-1]:                                 # the lists of k and k' < k agree on the first k' entries
            kk = got["d2"].shape[1]
            assert got["index"].tobytes() == np.ascontiguousarray(results[-1]["index"][:, :kk]).tobytes()
    else:
        for got in results:
            assert ((got["index"] >= 0).sum(axis=1) == len(case.P) - 1).all() and got["info"]["rounds"] >= 1


@pytest.mark.parametrize("name", kg.case_names("lattice-"))
def test_lattice_ties(nb, name):
    """Spacing = cell side = h0: every 4-neighbour at d2 == H2_0 exactly, in four cells the walk does not visit in index order."""
    side = kg.LATTICE_SIDE
    interior = np.array([i for i in range(side * side) if 0 < i % side < side - 1 and 0 < i // side < side - 1])
    for got, ask in zip(run_case(nb, name), kg.cases()[name].asks):
        assert np.array_equal(got["index"][interior, :4], np.stack([interior - side, interior - 1, interior + 1, interior + side], axis=1))
        if ask[3] == 4:                                          # k = 4 stops in round 1 for interior rows: <=
            assert got["info"]["widened"] == side * side - len(interior)
        else:                                                    # k = 5 must widen
            assert got["info"]["widened"] == side * side and got["info"]["rounds"] >= 2 and (got["d2"][interior, 4] == 2.0).all()


@pytest.mark.parametrize("name", kg.case_names("stack-") + kg.case_names("clump-") + kg.case_names("first-radius-") + kg.case_names("cut-"))
def test_ties_rounds_radii_and_cuts(nb, name):
    results = run_case(nb, name)
    if name.startswith("stack-"):
        assert (results[0]["d2"][:kg.STACK] == 0.0).all() and (results[1]["d2"][:kg.STACK] == 0.0).all()       # 39 others at d2 = 0
        assert results[1]["index"][0].tolist() == list(range(1, 33)) and results[0]["index"][5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8]
    elif name.startswith("clump-"):
        assert results[0]["info"]["rounds"] >= 5
        for got in results[1:]:                                  # 1 x 7 and 7 x 1: the same entries
            kg.assert_same(got, results[0], name, info=False)
    elif name.startswith("first-radius-"):
        matched, tiny, huge = results
        assert tiny["info"]["rounds"] == kg.ROUNDS_MAX + 1 and huge["info"]["widened"] == 0 and huge["info"]["rounds"] == 1
        for got in (tiny, huge):
            assert got["d2"].tobytes() == matched["d2"].tobytes() and got["index"].tobytes() == matched["index"].tobytes()
    else:
        zero, short, exact, none = results
        assert (zero["index"] >= 0).sum() == 2 and (short["index"] >= 0).sum(axis=1).min() < 8
        assert exact["index"][0].tolist() == none["index"][0, :3].tolist() + [-1] * 5


@pytest.mark.parametrize("name", kg.case_names("points-"))
def test_awkward_points(nb, name):
    case = kg.cases()[name]
    matched, part, coarse = run_case(nb, name)
    m = len(case.points)
    for got in (matched, part, coarse):
        assert got["info"]["rows"] == m == len(got["d2"]) and got["info"]["n"] == len(case.P)
        assert (got["index"][-3:] == -1).all() and np.isinf(got["d2"][-3:]).all()       # NaN and 1e200: every d2 NaN or +inf
        assert got["info"]["rounds"] == kg.ROUNDS_MAX + 1        # the 1e200 rows stop only where the radius is +inf
        assert (got["index"][-6] >= 0).all()                     # 1e6 fields away: the k nearest all the same
    assert (matched["d2"][:m // 4, 0] == 0.0).any()              # points ON bodies


# ---------------------------------------------------------------------------------------------------------------------
# 3. argument errors, each found before the handle is looked at; the wrapper
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(nb):
    P, R, f = kg.wc.state(64, np.float32)
    grid = nb.make_grid(4, 4, (0, f, 0, f))
    d2, index = np.zeros((64, 8)), np.zeros((64, 8), dtype=np.int32)
    info = np.zeros(1, dtype=nb.KNN_GRID_INFO_DTYPE)
    data = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    with small_stepper(nb, 0, 64) as st:                          # never uploaded: a valid call would be NBODY_ERR_STATE
        def call(g=grid, p=None, m=64, k=8, h0=0.25 * f, h2=np.inf, d=d2, x=index, i=info, handle=st._ctx):
            return nb.lib.nbody_get_knn_grid(handle, data(g), data(p), m, k, h0, h2, data(d), data(x), data(i))
        assert call() == STATE_ERR
        for bad in (dict(k=0), dict(k=33), dict(h0=0.0), dict(h0=np.nan), dict(h2=-1.0), dict(h0=np.inf), dict(h0=2.0 ** -501),
                    dict(h2=np.nan), dict(g=None), dict(m=-1), dict(d=None), dict(x=None), dict(i=None), dict(handle=None),
                    dict(g=nb.make_grid(0, 4, (0, 1, 0, 1))), dict(g=nb.make_grid(2048, 1024, (0, 1, 0, 1)))):
            assert call(**bad) == INVALID, bad
        assert not d2.view(np.uint8).any() and not index.view(np.uint8).any() and not info.view(np.uint8).any()   # nothing written
        with pytest.raises(nb.NbodyError) as e:
            st.knn(33, grid=grid)
        assert e.value.status == INVALID
        with pytest.raises(ValueError):
            st.knn(8, max_radius=1.0)                            # the brute-force call has no cut
        st.upload(bodies_of(nb, P, R, 0))                         # and the handle goes on
        assert call(m=63) == CAPACITY_ERR and not d2.view(np.uint8).any()
        assert call(h0=2.0 ** -500) == 0 and info["rows"][0] == 64 and info["rounds"][0] == kg.ROUNDS_MAX + 1
        assert st.knn(8, grid=grid)["info"]["n"] == 64


def test_wrapper_without_a_grid_is_unchanged(nb):
    """Stepper.knn(k) with grid=None: the keys and the bytes of nbody_get_knn, as before."""
    P, R, f = kg.wc.state(300, np.float32, coincident=True)
    pts = nc.probe_points(P, 40, 3, f)
    with small_stepper(nb, 0, 300) as st:
        st.upload(bodies_of(nb, P, R, 0))
        for points in (None, pts):
            got = st.knn(8, points)
            assert sorted(got) == ["d2", "index"]
            kc.assert_same(got, kc.model_knn(P, 8, points=points), "grid=None")
            assert st.knn(8, points, grid=None)["d2"].tobytes() == got["d2"].tobytes()
            by_radius = st.knn(8, points, grid=nb.make_grid(8, 8, (0, f, 0, f)), max_radius=0.1 * f)   # squared by the wrapper
            kg.assert_same(by_radius, kg.model_knn_grid(P, by_radius["grid"], 8, (0.1 * f) * (0.1 * f), points), "max_radius", info=False)
        g = nb.knn_grid((0.5 * f, 0.5 * f), 8, 300)
        assert int(g["nx"][0]) == int(g["ny"][0]) == 6


# ---------------------------------------------------------------------------------------------------------------------
# 4. batches and groups
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [0, 1, 64, 257, 300]


def test_batch_equals_steppers_and_model(nb):
    cap = 300
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        cfg, bd = dense_bodies(nb, max(n, 1), seed=80 + s)
        cfgs.append(cfg)
        bodies.append(bd if n else nb.BodiesData(0))
    w = float(dense_field(cap))
    grid = nb.make_grid(12, 9, (-w, w, -w / 2, w))              # leaves bodies outside
    pts = np.random.default_rng(5).uniform(-w, w, size=(70, 2))
    with nb.StepperBatch(len(BATCH_SIZES), cap, params=[params_of(c) for c in cfgs]) as batch:
        batch.upload(bodies)
        assert batch.counts().tolist() == BATCH_SIZES
        for points in (None, pts):
            for k, cut in ((8, None), (17, 0.4 * w)):
                got = batch.knn(k, points, grid=grid, max_radius=cut)
                assert len(got) == len(BATCH_SIZES)
                for s, n in enumerate(BATCH_SIZES):
                    state = batch.download(s)
                    with nb.Stepper(cfgs[s], capacity=cap) as one:    # a Stepper holding the same state
                        one.upload(state)
                        want = one.knn(k, points, grid=grid, max_radius=cut)
                    kg.assert_same(got[s], want, "system %d" % s)
                    P, _ = nc.widen(state)
                    h2 = np.inf if cut is None else cut * cut
                    kg.assert_same(got[s], kg.rule_model(P.reshape(-1, 2), grid[0], k, kg.default_h0(grid[0]), h2, points), "system %d, the model" % s)
                    assert got[s]["info"]["n"] == n and got[s]["info"]["rows"] == (n if points is None else len(pts))
                assert got[-1]["info"]["outside"] > 0 and (got[-1]["index"] >= 0).any()
                assert (got[0]["index"] == -1).all()             # the empty system: no row, or every point's entries empty


def test_every_rank_of_a_group(nb):
    world, n = 2, 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    w = float(dense_field(n))
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    try:
        grp.upload(b)
        grp.step(sc.LAG + 2)                                      # past the exchange lag
        P, _ = nc.widen(grp.download())
        assert len(P) < n
        grid = nb.knn_grid((w, w), 8, len(P))
        want = kg.rule_model(P, grid[0], 8, kg.default_h0(grid[0]))
        rank0 = grp.knn(8, grid=grid, rank=0)
        rank1 = grp.knn(8, grid=grid, rank=1)                     # each on its own: not collective
        kg.assert_same(rank0, want, "rank 0")
        kg.assert_same(rank1, rank0, "rank 1 against rank 0")
        if want["info"]["outside"] == 0:                          # every body a source: the brute-force query's bytes
            plain = grp.knn(8, rank=1)
            assert plain["d2"].tobytes() == rank0["d2"].tobytes() and plain["index"].tobytes() == rank0["index"].tobytes()
    finally:
        grp.close()


def test_state_preservation_after_steps(nb):
    """n = 1024 in a dense field: bodies merge, the count comes from the device.  A step after the queries gives the bits of
    a run without them."""
    n = 1024
    cfg, b = dense_bodies(nb, n, seed=7013)
    w = float(dense_field(n))
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as ref:
        st.upload(b)
        ref.upload(b)
        st.step(2)
        ref.step(2)
        P, _ = nc.widen(st.download())
        assert len(P) < n
        grid = nb.knn_grid((w, w), 16, len(P))
        got = st.knn(16, grid=grid)
        kg.assert_same(got, kg.rule_model(P, grid[0], 16, kg.default_h0(grid[0])), "after 2 steps")
        assert got["info"]["n"] == len(P) == len(got["d2"])
        st.knn(5, points=P[:50] + 1.0, grid=grid, max_radius=0.2 * w)
        st.step(2)
        ref.step(2)
        assert st.download().block.tobytes() == ref.download().block.tobytes()
