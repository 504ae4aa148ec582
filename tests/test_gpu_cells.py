"""Cell sums (nbody_get_cells, nbody_batch_get_cells; Stepper.cells, StepperGroup.cells, StepperBatch.cells) on the MI355X: the
count, mass, momentum and twice the kinetic energy of the bodies in every cell of a uniform grid, and the cell list.

The definition has no fma, rounds every operation on its own and fixes the order of every sum, so the numpy model of
cell_cases.py restates it bit for bit: zero tolerance throughout - integers exactly, doubles by their bits - against the
model, and product against product (nbody_get_shells, another rank, a batch against a Stepper holding the same state) the
same way.  The masses span 1e4 .. 1e17: test_cell_cases_cpu.py asserts that the sums of these states change with the order,
so a kernel that adds in another order, or re-associates, fails the comparisons here."""
import numpy as np
import pytest

import cell_cases as cc
import sharded_cases as sc
from test_gpu_batch import params_of
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
DTYPE_OF = {0: np.float32, 1: np.float64}


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, V, M, precision):
    n = len(P)
    return nb.BodiesData.from_arrays(P, V, M, np.full(n, 0.25), precision) if n else nb.BodiesData(0, precision)


def widen_state(b):
    """A BodiesData (or a download) -> (P, V, M) float64, exact."""
    return (np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Velocities, dtype=np.float64),
            np.asarray(b.Masses, dtype=np.float64))


def check(st, P, V, M, nx, ny, bounds, what, moments=True):
    """cells() with lists on the resident state against the model of (P, V, M); -> the result."""
    got = st.cells(nx, ny, bounds, moments=moments, lists=True)
    want = cc.model_cells(P, V, M, got["grid"], moments)
    assert got["cells"].shape == (ny, nx), what
    cc.assert_same(got, want, what)
    assert got["info"]["inside"] + got["info"]["outside"] == got["info"]["n"] == len(P), what
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. workgroup and wave edges of the per-body kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 385])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_body_edges(nb, precision, n):
    P, V, M = cc.moving_state(n, DTYPE_OF[precision])
    f = cc.tenth_field(n)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, 8, 8, (0, f, 0, f), "n %d, 8 x 8" % n)
        assert got["info"]["inside"] == n and (n < 63 or got["info"]["occupied"] > 8)
        got = check(st, P, V, M, 1, 1, (0, f, 0, f), "n %d, 1 x 1" % n)      # one segment: every body's rank is its index
        assert got["info"]["largest"] == n and got["order"].tolist() == list(range(n))
        got = check(st, P, V, M, 8, 8, (0.25 * f, 0.75 * f, 0.25 * f, f), "n %d, bodies outside" % n)
        assert n < 63 or 0 < got["info"]["outside"] < n


# ---------------------------------------------------------------------------------------------------------------------
# 2. grid shapes
# ---------------------------------------------------------------------------------------------------------------------
# cells_scan takes 4 consecutive cells per lane, 256 per wave, 4096 per trip.  515 x 511 = 263165 = 64 * 4096 + 1021 cells:
# 64 full trips, then a trip that ends after 3 full waves (768 cells) and 63 full lanes (252 cells) on the first cell of a
# lane - every boundary of the scan is crossed with cells on both sides, and the carry runs through 64 trips
BIG_GRID = (515, 511)


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (3, 3), (64, 64), (257, 3), BIG_GRID], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_grid_shapes(nb, precision, shape):
    n = 300
    nx, ny = shape
    assert BIG_GRID[0] * BIG_GRID[1] >= 1 << 18 and BIG_GRID[0] * BIG_GRID[1] % 4096 == 1021 and 1021 % 256 == 253 and 253 % 4 == 1
    P, V, M = cc.moving_state(n, DTYPE_OF[precision])
    f = cc.tenth_field(n)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, nx, ny, (0, f, 0, f), "%d x %d" % shape)
        assert got["info"]["inside"] == n
        if nx * ny >= 4096:
            assert got["info"]["occupied"] > n // 2 and (got["cells"]["count"] == 0).sum() > nx * ny - n     # mostly empty
            assert got["cell_of"].max() > nx * ny - nx * ny // 8                                              # up to the last trip
        got = check(st, P, V, M, nx, ny, (0.1 * f, 0.9 * f, 0.2 * f, 0.8 * f), "%d x %d, bodies outside" % shape)
        assert got["info"]["outside"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. segment sizes: both paths of cells_sum, segments that span waves and workgroups in cells_place and cells_rank
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_segment_sizes(nb, precision):
    """Cells of exactly 1, 63, 64, 65, 129 and 1000 members on an 8 x 8 grid (the rest empty), the bodies in a random order: 63
    is the largest cell one lane sums, 64 the smallest a wave does, 65 and 129 leave a ragged last gather, 1000 is a segment
    of four workgroups' slots.  1322 bodies: six workgroups."""
    sizes = [1, 63, 64, 65, 129, 1000]
    P, V, M, bounds = cc.sized_state(sizes, DTYPE_OF[precision])
    with small_stepper(nb, precision, len(P)) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, 8, 8, bounds, "sized cells")
        assert got["cells"]["count"].reshape(-1)[:7].tolist() == sizes + [0]
        assert got["info"]["largest"] == 1000 and got["info"]["largest_cell"] == 5 and got["info"]["occupied"] == 6
        check(st, P, V, M, 8, 8, bounds, "sized cells, no moments", moments=False)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_body_in_one_cell(nb, precision):
    n = 1000
    P, V, M = cc.moving_state(n, DTYPE_OF[precision], field=1.0)
    P = (P * 0.5 + 2.25).astype(DTYPE_OF[precision]).astype(np.float64)     # inside cell (2, 2) of [0, 8)^2
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, 8, 8, (0, 8, 0, 8), "one cell of 64")
        assert got["info"] == {"n": n, "inside": n, "outside": 0, "occupied": 1, "largest": n, "largest_cell": 18}
        assert got["order"].tolist() == list(range(n))


# ---------------------------------------------------------------------------------------------------------------------
# 4. edges and awkward values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_on_the_cell_boundaries(nb, precision):
    """lattice(8) with x0 = 0 and sx = 1: every body sits on a corner of four cells and belongs to the one above and to the
    right of it - cell (x, y) holds body y * 8 + x alone."""
    P, _ = cc.lattice(8)
    V, M = cc.velocities(64, DTYPE_OF[precision]), np.arange(1.0, 65.0)
    with small_stepper(nb, precision, 64) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, 8, 8, (0, 8, 0, 8), "lattice")
        assert got["grid"]["sx"] == 1.0 and got["grid"]["sy"] == 1.0
        assert got["cell_of"].tolist() == list(range(64)) and (got["cells"]["count"] == 1).all()
        assert np.array_equal(got["cells"]["mass"].reshape(-1), M)
        got = check(st, P, V, M, 7, 7, (0, 7, 0, 7), "lattice, the last row and column outside")
        assert got["info"]["outside"] == 15


@pytest.mark.parametrize("precision", PRECISIONS)
def test_awkward_values(nb, precision):
    dtype = DTYPE_OF[precision]
    top = dtype(8.0)
    below = np.nextafter(top, dtype(0.0))                        # one ulp of the state's precision below the upper bound
    P = np.array([[0.0, 0.0], [-0.0, 1.0], [top, 1.0], [below, below], [1e30, 1.0], [-1e30, 1.0], [1.0, 1e30], [1.0, -1e30],
                  [3.0, 3.0], [3.0, 3.0], [1.0, top]], dtype=dtype).astype(np.float64)
    n = len(P)
    V, M = cc.velocities(n, dtype), np.arange(1.0, n + 1.0)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, 8, 8, (0, 8, 0, 8), "awkward")
        # the upper bound is outside, one ulp below it is the last cell, -0.0 at x0 = 0 is column 0, 1e30 either way is outside
        assert got["cell_of"].tolist() == [0, 8, -1, 63, -1, -1, -1, -1, 27, 27, -1]
        assert got["info"] == {"n": n, "inside": 5, "outside": 6, "occupied": 4, "largest": 2, "largest_cell": 27}


# ---------------------------------------------------------------------------------------------------------------------
# 5. product against product
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_shells_and_itself(nb, precision):
    n = 300
    P, V, M = cc.moving_state(n, DTYPE_OF[precision])
    f = cc.tenth_field(n)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        # one cell for everything: the ascending sum over all j, which is shells' one bin [0, inf) at a far point
        one = st.cells(1, 1, (-f, 2 * f, -f, 2 * f))
        far = st.shells(np.array([0.0, np.inf]), points=np.array([[-50.0 * f, 70.0 * f]]), squared=True)
        assert one["info"]["inside"] == n == far["count"][0, 0]
        assert cc.bits(one["cells"]["mass"])[0, 0] == cc.bits(far["mass"])[0, 0]
        # moments=False: the same mass and count, px, py and k2 +0.0
        grid = nb.make_grid(4, 4, (0, f, 0, f))
        first = st.cells(grid, lists=True)
        plain = st.cells(grid, moments=False, lists=True)
        for fld in ("mass", "count", "first"):
            assert first["cells"][fld].tobytes() == plain["cells"][fld].tobytes()
        for fld in ("px", "py", "k2"):
            assert not cc.bits(plain["cells"][fld]).any() and cc.bits(first["cells"][fld]).any()
        # two calls in a row: the same bits, whatever order the waves arrived in
        second = st.cells(grid, lists=True)
        assert first["cells"].tobytes() == second["cells"].tobytes() and first["info"] == second["info"]
        for fld in ("cell_of", "start", "order"):
            assert np.array_equal(first[fld], second[fld]) and np.array_equal(first[fld], plain[fld])
        assert cc.lists_consistent(first)


# ---------------------------------------------------------------------------------------------------------------------
# 6. after real steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps(nb, semantics):
    """n = 1024 at stock radii in a dense field: bodies merge, the count comes from the device's Meta, the velocities are
    those of the steps.  The default bounds are the field."""
    n = 1024
    cfg, b = dense_bodies(nb, n, seed=7003)
    w = float(dense_field(n))
    with nb.Stepper(cfg, semantics=semantics) as st:
        st.upload(b)
        st.step(3)
        P, V, M = widen_state(st.download())
        assert len(P) < n                                         # merged
        got = st.cells(16, lists=True)
        assert cc.grid_tuple(got["grid"]) == cc.grid_of(16, 16, (-w, w, -w, w))
        cc.assert_same(got, cc.model_cells(P, V, M, got["grid"]), "after 3 steps, the field")
        assert got["info"]["n"] == len(P) and got["info"]["inside"] > 0
        check(st, P, V, M, 32, 8, (0, w, 0, w), "after 3 steps, a quadrant")


# ---------------------------------------------------------------------------------------------------------------------
# 7. an empty system
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_empty_system(nb, precision):
    with small_stepper(nb, precision, 16) as st:
        st.upload(nb.BodiesData(0, precision))
        got = st.cells(5, 3, (0, 5, 0, 3), lists=True)
        cc.assert_same(got, cc.model_cells(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), got["grid"]), "empty")
        cells = got["cells"]
        assert (cells["count"] == 0).all() and (cells["first"] == -1).all() and not got["start"].any()
        for fld in cc.CELL_FIELDS:
            assert not cc.bits(cells[fld]).any()                # +0.0
        assert got["info"] == {"n": 0, "inside": 0, "outside": 0, "occupied": 0, "largest": 0, "largest_cell": 0}
        assert len(got["cell_of"]) == 0 and len(got["order"]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors that need a handle
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_and_state_errors(nb):
    n = 100
    P, V, M = cc.moving_state(n, np.float32)
    grid = nb.make_grid(4, 4, (0, 50, 0, 50))
    cells, info = np.zeros(16, dtype=nb.CELL_DTYPE), np.zeros(1, dtype=nb.CELLS_INFO_DTYPE)
    lists = [np.full(n, -5, dtype=np.int32), np.full(17, -5, dtype=np.int32), np.full(n, -5, dtype=np.int32)]
    co, stt, od = (a.ctypes.data for a in lists)
    with small_stepper(nb, 0, n) as st:
        call = lambda *a: nb.lib.nbody_get_cells(st._ctx, grid.ctypes.data, 1, cells.ctypes.data, *a, info.ctypes.data)  # noqa: E731
        assert call(None, None, None, 0) == STATE_ERR           # before an upload
        st.upload(bodies_of(nb, P, V, M, 0))
        assert call(co, None, None, n - 1) == CAPACITY_ERR and call(None, stt, od, n - 1) == CAPACITY_ERR
        assert all((a == -5).all() for a in lists) and not cells.view(np.uint8).any()       # nothing written
        assert call(None, stt, None, 0) == 0 and call(None, None, None, -1) == 0            # cap is the lists' room only
        assert call(co, stt, od, n) == 0 and lists[1][16] == info["inside"][0] == (lists[0] >= 0).sum()


# ---------------------------------------------------------------------------------------------------------------------
# 9. batches
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [0, 1, 64, 129, 1024]


def test_batch_equals_stepper_and_model(nb):
    cap = 1024
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        cfg, bd = dense_bodies(nb, max(n, 1), seed=40 + s)
        cfgs.append(cfg)
        bodies.append(bd if n else nb.BodiesData(0))
    S = len(BATCH_SIZES)
    w = float(dense_field(cap))
    bounds = (-w, w, -w / 2, w)
    with nb.StepperBatch(S, cap, params=[params_of(c) for c in cfgs]) as batch:
        batch.upload(bodies)
        for steps, (nx, ny) in ((0, (8, 8)), (3, (33, 5))):
            batch.step(steps)
            got, counts = batch.cells(nx, ny, bounds, lists=True), batch.counts()
            assert got["cells"].shape == (S, ny, nx) and got["start"].shape == (S, nx * ny + 1)
            assert got["cell_of"].shape == (S, cap) == got["order"].shape and got["info"]["n"].tolist() == counts.tolist()
            if steps == 0:
                assert counts.tolist() == BATCH_SIZES
            else:
                assert counts[-1] < cap                           # merged
            for s in range(S):
                n = int(counts[s])
                state = batch.download(s)
                with nb.Stepper(cfgs[s], capacity=cap) as one:    # a Stepper holding the same state
                    one.upload(state)
                    want = one.cells(nx, ny, bounds, lists=True)
                inside = want["info"]["inside"]
                mine = {"cells": got["cells"][s], "info": got["info"][s], "cell_of": got["cell_of"][s, :n], "start": got["start"][s],
                        "order": got["order"][s, :inside]}
                cc.assert_same(mine, want, "system %d after %d steps" % (s, steps))
                cc.assert_same(mine, cc.model_cells(*widen_state(state), want["grid"]), "system %d, the model" % s)
                assert (got["cell_of"][s, n:] == -1).all() and (got["order"][s, inside:] == -1).all()   # the tails stay
            assert got["info"]["inside"][-1] > 0


def test_batch_capacity_error(nb):
    cfg, bd = dense_bodies(nb, 4, seed=3)
    with nb.StepperBatch(5, 4, params=[params_of(cfg)] * 5) as batch:
        batch.upload([bd] * 5)
        with pytest.raises(nb.NbodyError) as e:                   # 5 x 2^20 cells > 2^22
            batch.cells(1024, 1024, (0, 1, 0, 1), moments=False)
        assert e.value.status == CAPACITY_ERR
        assert batch.cells(2, 2, (-1e4, 1e4, -1e4, 1e4))["info"]["inside"].tolist() == [4] * 5


# ---------------------------------------------------------------------------------------------------------------------
# 10. groups: any rank gives the bits of a single-rank context
# ---------------------------------------------------------------------------------------------------------------------
def test_every_rank_of_a_group(nb):
    world, n = 2, 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    w = float(dense_field(n))
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    grp.upload(b)
    grp.step(sc.LAG + 2)                                          # past the exchange lag
    d = grp.download()
    P, V, M = widen_state(d)
    assert len(P) < n                                             # the count has shrunk
    with nb.Stepper(cfg) as one:                                  # a single-rank context on the group's download
        one.upload(d)
        want = one.cells(16, 12, (-w, w, -w, w), moments=False, lists=True)
    cc.assert_same(want, cc.model_cells(P, V, M, want["grid"], moments=False), "single rank")
    assert want["info"]["inside"] > 0
    for rank in reversed(range(world)):                           # each on its own
        cc.assert_same(grp.cells(16, 12, (-w, w, -w, w), lists=True, rank=rank), want, "rank %d" % rank)
        with pytest.raises(nb.NbodyError) as e:
            grp.cells(16, 12, (-w, w, -w, w), moments=True, rank=rank)
        assert e.value.status == STATE_ERR
    grp.close()
