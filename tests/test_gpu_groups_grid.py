"""Groups on the cell list (nbody_get_groups_grid, nbody_batch_get_groups_grid; Stepper.groups(grid=...), StepperGroup.groups,
StepperBatch.groups) on the MI355X: the friends-of-friends labels of the bodies inside a grid, found through the cell list.

A label is the lowest index of its connected component, an integer function of the set of links, and the links are the
brute-force predicate bit for bit: zero tolerance throughout - every label and count against the numpy model of
groups_grid_cases.py and product against product (Stepper.groups without a grid, another grid, another rank, a batch against
a Stepper holding the same state).  test_groups_grid_cases_cpu.py holds, for every constructed case used here, that every
link is seen from its larger end; the two tests on stepped states hold it on the downloaded state before they ask."""
import numpy as np
import pytest

import group_cases as gc
import groups_grid_cases as gg
import neighbor_cases as nc
import sharded_cases as sc
import within_cases as wc
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISION_OF = {np.float32: 0, np.float64: 1}


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, R, precision):
    n = len(R)
    return nb.BodiesData.from_arrays(P, np.zeros((n, 2)), np.ones(n), R, precision) if n else nb.BodiesData(0, precision)


def ask_one(nb, st, P, R, ask, what):
    """One ask on the resident state against the model of (P, R); -> the result."""
    nx, ny, bounds, link, scale = ask
    got = st.groups(link, scale, grid=nb.make_grid(nx, ny, bounds))
    want = gg.model_groups_grid(P, R, got["grid"], link, scale)
    print("%s %r: n %d -> %d groups, largest %d, outside %d, %d sweeps" % (what, ask, len(R), got["n_groups"], got["largest"],
                                                                          got["outside"], got["sweeps"]))
    gg.assert_same(got, want, "%s %r" % (what, ask))
    assert got["label"].dtype == np.int32 and 1 <= got["sweeps"] <= len(R) + 1, what
    return got


def run_case(nb, case):
    """Every ask of the case against the model -> (the results, Stepper.groups without a grid for every ask)."""
    precision = PRECISION_OF[case.dtype]
    with small_stepper(nb, precision, len(case.R)) as st:
        st.upload(bodies_of(nb, case.P, case.R, precision))
        got = [ask_one(nb, st, case.P, case.R, ask, case.name) for ask in case.asks]
        plain = [st.groups(ask[3], ask[4]) for ask in case.asks]
    return got, plain


def same_bytes(a, b):
    return a["label"].tobytes() == b["label"].tobytes() and (a["n_groups"], a["largest"]) == (b["n_groups"], b["largest"])


# ---------------------------------------------------------------------------------------------------------------------
# 1. workgroup and wave edges: 8 x 8, 1 x 1 and a grid that leaves bodies outside
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gg.case_names("bodies-"))
def test_body_edges(nb, name):
    case = gg.cases()[name]
    n = len(case.R)
    (full, one, part), plain = run_case(nb, case)
    assert full["inside"] == n == one["inside"] and full["outside"] == 0
    assert same_bytes(full, one) and same_bytes(full, plain[0]), name
    inside = gg.inside_of(case.P, part["grid"])
    assert part["outside"] == int((~inside).sum()) and np.array_equal(part["label"][~inside], np.flatnonzero(~inside))
    if n >= 63:
        assert 0 < part["outside"] < n and not np.array_equal(part["label"], full["label"])
        assert 1 < full["n_groups"] < n and full["largest"] > 2


# ---------------------------------------------------------------------------------------------------------------------
# 2. grid shapes, the long path, ties on cell boundaries, the asymmetric window, one cell
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gg.case_names("shapes-"))
def test_grid_shapes(nb, name):
    got, plain = run_case(nb, gg.cases()[name])
    for g in got:                                                # every grid holds every body: the same bytes
        assert g["outside"] == 0 and same_bytes(g, got[0]) and same_bytes(g, plain[0]), (name, g["grid"])
    assert 1 < got[0]["n_groups"] < 300


@pytest.mark.parametrize("name", gg.case_names("chain-"))
def test_the_long_path(nb, name):
    """The shuffled chain on 64 x 1 and on 300 x 1 cells (cell side = spacing): linked at link = spacing - 2 * radius, where
    d2 == s*s, the one label 0 travels up to 299 links; apart at the largest link below."""
    case = gg.cases()[name]
    got, plain = run_case(nb, case)
    for g, p, ask in zip(got, plain, case.asks):
        assert same_bytes(g, p), ask
        if ask[3] == 0.5:
            assert (g["label"] == 0).all() and (g["n_groups"], g["largest"]) == (1, 300) and g["sweeps"] <= 301, ask
        else:
            assert np.array_equal(g["label"], np.arange(300)) and (g["n_groups"], g["largest"]) == (300, 1), ask


@pytest.mark.parametrize("name", gg.case_names("lattice-"))
def test_ties_on_cell_boundaries(nb, name):
    """Spacing = cell side = link, centres only, at offsets 0 and 0.1: every link is at d2 == s*s and crosses a boundary."""
    case = gg.cases()[name]
    got, plain = run_case(nb, case)
    for g, p, ask in zip(got, plain, case.asks):
        assert same_bytes(g, p), ask
        assert (g["n_groups"], g["largest"]) == ((1, 289) if ask[3] == 1.0 else (289, 1)), ask
        assert g["inside"] == 289


@pytest.mark.parametrize("name", gg.case_names("asymmetric-"))
def test_the_asymmetric_window(nb, name):
    """One body of r = 6 over small ones whose own windows are 3 x 3 cells: only its row finds those links, whether it has
    the lowest or the highest index; two equal bodies touching across cells; a negative radius; a NaN radius."""
    case = gg.cases()[name]
    (got,), (plain,) = run_case(nb, case)
    assert same_bytes(got, plain) and got["outside"] == 0, name
    n = len(case.R)
    extra = ("negative" in name) + ("nan" in name)
    big = 0 if "first" in name else n - 1 - extra
    under = np.flatnonzero(gc.adjacency(case.P, case.R, 0.0, 1.0)[big])
    assert len(under) > 50 and (got["label"][under] == got["label"][big]).all()
    assert np.abs(case.P[under] - case.P[big]).max() > 5.0       # five cells away
    if "nan" in name:
        assert got["label"][n - 1] == n - 1 and (got["label"] == n - 1).sum() == 1
        twin = gg.cases()[name.replace("-nan", "")]
        assert np.array_equal(got["label"][:n - 1], gg.model_groups_grid(twin.P, twin.R, got["grid"], 0.0, 1.0)["label"])
    if "negative" in name:
        assert (got["label"] == got["label"][n - 1]).sum() > 20


@pytest.mark.parametrize("name", gg.case_names("one-cell-"))
def test_every_body_in_one_cell_and_an_infinite_link(nb, name):
    (near, inf), plain = run_case(nb, gg.cases()[name])
    assert same_bytes(near, plain[0]) and same_bytes(inf, plain[1])
    assert 1 < near["n_groups"] < 385 and (inf["n_groups"], inf["largest"]) == (1, 385) and (inf["label"] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_alone_exactly_where_nothing_overlaps(nb, dtype):
    """(0, 1), nothing outside: label[i] == i with no other body carrying i exactly where within()'s overlaps is 0."""
    P, R, f = wc.state(300, dtype)
    grid = nb.make_grid(8, 8, (0, f, 0, f))
    with small_stepper(nb, PRECISION_OF[dtype], 300) as st:
        st.upload(bodies_of(nb, P, R, PRECISION_OF[dtype]))
        got = st.groups(0.0, 1.0, grid=grid)
        overlaps = st.within(np.inf, grid=grid)["rows"]["overlaps"]
    alone = np.bincount(got["label"], minlength=300)[got["label"]] == 1
    assert got["outside"] == 0 and np.array_equal(alone, overlaps == 0) and 0 < alone.sum() < 300


# ---------------------------------------------------------------------------------------------------------------------
# 3. a resident state after collisions, and no effect on stepping
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
        P, R = nc.widen(st.download())
        assert len(R) < n                                        # compaction has run
        typical = float(np.median(R))
        mixed = 0
        for link, scale in ((0.0, 1.0), (0.5 * typical, 1.0), (4.0 * typical, 0.0)):
            matched = nb.groups_grid((w, w), link, scale, typical)
            lo, hi = P.min(axis=0) - 1.0, P.max(axis=0) + 1.0
            holds_all = nb.make_grid(int(matched["nx"][0]), int(matched["ny"][0]), (lo[0], hi[0], lo[1], hi[1]))
            for grid in (matched, holds_all):
                gg.window_holds(P, R, grid[0], link, scale)
                got = st.groups(link, scale, grid=grid)
                gg.assert_same(got, gg.model_groups_grid(P, R, grid[0], link, scale), "link %g scale %g" % (link, scale))
            plain = st.groups(link, scale)
            assert got["outside"] == 0 and same_bytes(got, plain), (link, scale)
            mixed += 1 < got["n_groups"] < len(R)
        assert mixed                                             # some link gives neither one clump nor all singletons
        st.step(2)
        twin.step(2)
        assert st.download().block.tobytes() == twin.download().block.tobytes()
        assert int(st.stats().pairs) == int(twin.stats().pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. batch
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_equals_steppers_and_model(nb):
    """Four systems - none, one body, the shuffled chain, a random state - under one link: the chain's label travels for
    many sweeps, the random state converges after a few and leaves at the prologue from then on."""
    cap, S = gg.BATCH_CAP, len(gg.BATCH_COUNTS)
    states = gg.batch_states()
    bodies = [bodies_of(nb, P, R, 0) for P, R in states]
    link = gg.BATCH_LINK
    with nb.StepperBatch(S, cap, params=[(0.2, 0.1, 100, 100)] * S) as batch, small_stepper(nb, 0, cap) as one:
        batch.upload(bodies)
        assert batch.counts().tolist() == list(gg.BATCH_COUNTS)
        for ask in gg.BATCH_GRIDS:
            grid = nb.make_grid(*ask)
            got = batch.groups(link, 1.0, grid=grid)
            assert len(got) == S
            raw = np.full((S, cap), -77, dtype=np.int32)          # the C call into a prefilled buffer: the tails stay
            infos = np.zeros(S, dtype=nb.GROUPS_GRID_INFO_DTYPE)
            assert nb.lib.nbody_batch_get_groups_grid(batch._b, grid.ctypes.data, link, 1.0, raw.ctypes.data, infos.ctypes.data) == 0
            alone = []
            for s, (P, R) in enumerate(states):
                n = gg.BATCH_COUNTS[s]
                what = "system %d (n %d) grid %r" % (s, n, ask)
                assert np.array_equal(raw[s, :n], got[s]["label"]) and (raw[s, n:] == -77).all(), what
                assert tuple(infos[s]) == (n, got[s]["n_groups"], got[s]["largest"], got[s]["sweeps"], got[s]["inside"],
                                           got[s]["outside"]), what
                gg.assert_same(got[s], gg.model_groups_grid(P, R, grid[0], link, 1.0), what + ": model")
                assert got[s]["sweeps"] == got[0]["sweeps"], what   # the one number of the whole call
                if n == 0:
                    assert got[s]["label"].shape == (0,) and (got[s]["n_groups"], got[s]["inside"], got[s]["outside"]) == (0, 0, 0)
                    continue
                one.upload(bodies[s])                             # a Stepper holding the same state
                want = one.groups(link, 1.0, grid=grid)
                gg.assert_same(got[s], want, what + ": Stepper")
                assert got[s]["label"].tobytes() == want["label"].tobytes()
                alone.append(want["sweeps"])
            print("grid %r: sweeps of each system on its own %r, of the batch %d" % (ask, alone, got[0]["sweeps"]))
            assert got[0]["sweeps"] >= 2 and min(alone) < max(alone)                # a system converged sweeps before another
        assert got[2]["outside"] > 0 and got[3]["outside"] > 0   # the second grid leaves bodies outside


# ---------------------------------------------------------------------------------------------------------------------
# 5. not collective
# ---------------------------------------------------------------------------------------------------------------------
def test_either_rank_of_a_sharded_group(nb):
    world, n = 2, 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    w = float(dense_field(n))
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    try:
        grp.upload(b)
        grp.step(sc.LAG + 2)                                      # past the exchange lag
        state = grp.download()
        P, R = nc.widen(state)
        assert len(R) < n
        link = float(np.median(R))
        grid = nb.groups_grid((w, w), link, 1.0, link)
        assert gg.window_holds(P, R, grid[0], link, 1.0) > 0
        want = gg.model_groups_grid(P, R, grid[0], link, 1.0)
        assert want["n_groups"] < len(R)
        rank1 = grp.groups(link, grid=grid, rank=1)               # each on its own: not collective
        rank0 = grp.groups(link, grid=grid, rank=0)
        gg.assert_same(rank0, want, "rank 0")
        gg.assert_same(rank1, rank0, "rank 1 against rank 0")
        assert rank1["label"].tobytes() == rank0["label"].tobytes()
        with nb.Stepper(cfg) as single:                           # a single-rank context holding the group's state
            single.upload(state)
            gg.assert_same(single.groups(link, grid=grid), rank0, "a single-rank context")
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors on a live handle, and the buffers shared with within() and cells()
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_shared_buffers(nb):
    P, R, f = wc.state(300, np.float32)
    grid = nb.make_grid(8, 8, (0, f, 0, f))
    other = nb.make_grid(5, 3, (0.25 * f, f, 0, f))
    call = nb.lib.nbody_get_groups_grid
    label = np.full(300, -7, dtype=np.int32)
    info = np.full(1, -7, dtype=nb.GROUPS_GRID_INFO_DTYPE)
    untouched = (label.tobytes(), info.tobytes())
    want = gg.model_groups_grid(P, R, grid[0], gg.EDGE_LINK, 1.0)
    with small_stepper(nb, 0, 300) as st, small_stepper(nb, 0, 300) as fresh:
        assert call(st._ctx, grid.ctypes.data, 1.0, 1.0, label.ctypes.data, 300, info.ctypes.data) == STATE_ERR   # before an upload
        assert b"before" in nb.lib.nbody_last_error_string()
        st.upload(bodies_of(nb, P, R, 0))
        fresh.upload(bodies_of(nb, P, R, 0))
        assert call(st._ctx, grid.ctypes.data, 1.0, 1.0, label.ctypes.data, 299, info.ctypes.data) == CAPACITY_ERR
        assert (label.tobytes(), info.tobytes()) == untouched
        gg.assert_same(st.groups(gg.EDGE_LINK, grid=grid), want, "after NBODY_ERR_CAPACITY")   # the handle still answers
        for bad in ((None, 1.0, 1.0, label.ctypes.data, 300, info.ctypes.data), (grid.ctypes.data, -1.0, 1.0, label.ctypes.data, 300, info.ctypes.data),
                    (grid.ctypes.data, 1.0, np.inf, label.ctypes.data, 300, info.ctypes.data), (grid.ctypes.data, 1.0, 1.0, None, 300, info.ctypes.data),
                    (grid.ctypes.data, 1.0, 1.0, label.ctypes.data, -1, info.ctypes.data), (grid.ctypes.data, 1.0, 1.0, label.ctypes.data, 300, None)):
            assert call(st._ctx, *bad) == INVALID, bad
        assert (label.tobytes(), info.tobytes()) == untouched
        assert call(st._ctx, grid.ctypes.data, gg.EDGE_LINK, 1.0, label.ctypes.data, 300, info.ctypes.data) == 0
        assert np.array_equal(label, want["label"])
        assert tuple(info[0])[:3] == (300, want["n_groups"], want["largest"]) and tuple(info[0])[4:] == (300, 0)
        # the sorted records and the cell list are shared: within() and cells() after the new query, on another grid, give a
        # fresh handle's bytes - and the new query after them gives its own again
        h = 0.1 * f
        a, b = st.within(h, grid=other, lists=True), fresh.within(h, grid=other, lists=True)
        wc.assert_same(a, b, "within() after groups(grid=...)")
        assert a["rows"].tobytes() == b["rows"].tobytes() and a["list"].tobytes() == b["list"].tobytes()
        ca, cb = st.cells(other, lists=True), fresh.cells(other, lists=True)
        assert ca["cells"].tobytes() == cb["cells"].tobytes() and ca["order"].tobytes() == cb["order"].tobytes() and ca["info"] == cb["info"]
        gg.assert_same(st.groups(gg.EDGE_LINK, grid=grid), want, "after within() and cells()")
        st.upload(nb.BodiesData(0))                               # no bodies: nothing launched
        assert call(st._ctx, grid.ctypes.data, 4.0, 1.0, label.ctypes.data, 0, info.ctypes.data) == 0
        assert tuple(info[0]) == (0, 0, 0, 0, 0, 0) and np.array_equal(label, want["label"])
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 100, 100)] * 2) as batch:
        labels = np.full((2, 300), -7, dtype=np.int32)
        infos = np.full(2, -7, dtype=nb.GROUPS_GRID_INFO_DTYPE)
        bcall = nb.lib.nbody_batch_get_groups_grid
        assert bcall(batch._b, grid.ctypes.data, 1.0, 1.0, labels.ctypes.data, infos.ctypes.data) == STATE_ERR
        batch.upload([bodies_of(nb, P, R, 0), nb.BodiesData(0)])
        assert bcall(batch._b, grid.ctypes.data, 1.0, -2.0, labels.ctypes.data, infos.ctypes.data) == INVALID
        assert bcall(batch._b, grid.ctypes.data, 1.0, 1.0, None, infos.ctypes.data) == INVALID
        assert (labels == -7).all() and (infos["sweeps"] == -7).all()
        got = batch.groups(gg.EDGE_LINK, grid=grid)               # and the handle goes on
        gg.assert_same(got[0], want, "batch after its errors")
