"""The model of the cell sums against the definition as a scalar loop, the lists against the sums, the states' sensitivity to
the order of the sums, the argument checks that need no device, make_grid and cell_maps.  No GPU."""
import numpy as np
import pytest

import cell_cases as cc

INVALID, CAPACITY_ERR = -1, -7
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def same_everything(a, b, what):
    cc.assert_same(a, b, what)
    cc.assert_same(b, a, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the scalar loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("moments", [True, False])
def test_model_equals_the_scalar_loop(dtype, moments):
    n = 300
    P, V, M = cc.moving_state(n, dtype)
    f = cc.tenth_field(n)
    for nx, ny, bounds in ((4, 4, (0, f, 0, f)), (7, 3, (0, f, 0, f)), (1, 1, (-1, 2 * f, -1, 2 * f)),
                           (5, 6, (0.25 * f, 0.75 * f, 0.1 * f, 0.5 * f))):     # the last: bodies outside on every side
        grid = cc.grid_of(nx, ny, bounds)
        model, loop = cc.model_cells(P, V, M, grid, moments), cc.loop_cells(P, V, M, grid, moments)
        same_everything(model, loop, "%d x %d" % (nx, ny))
        assert model["info"]["inside"] + model["info"]["outside"] == n
        if not moments:
            assert not model["cells"]["px"].any() and not model["cells"]["k2"].any()
    assert model["info"]["outside"] > 0


def test_model_equals_the_scalar_loop_on_awkward_values():
    P = np.array([[0.0, 0.0], [-0.0, 1.0], [8.0, 1.0], [np.nextafter(8.0, 0.0), 7.5], [1e30, 1.0], [-1e30, 1.0], [np.nan, 1.0],
                  [1.0, np.inf], [3.0, 3.0], [3.0, 3.0]])
    n = len(P)
    V, M = cc.velocities(n, np.float64), np.arange(1.0, n + 1.0)
    grid = cc.grid_of(8, 8, (0, 8, 0, 8))
    model = cc.model_cells(P, V, M, grid)
    same_everything(model, cc.loop_cells(P, V, M, grid), "awkward")
    assert model["cell_of"].tolist() == [0, 8, -1, 63, -1, -1, -1, -1, 27, 27]
    assert model["info"] == {"n": n, "inside": 5, "outside": 5, "occupied": 4, "largest": 2, "largest_cell": 27}


def test_empty_states_and_grids():
    grid = cc.grid_of(3, 2, (0, 3, 0, 2))
    for P in (np.zeros((0, 2)), np.full((4, 2), 9.0)):          # no body; no body inside
        m = cc.model_cells(P, np.zeros_like(P), np.ones(len(P)), grid)
        same_everything(m, cc.loop_cells(P, np.zeros_like(P), np.ones(len(P)), grid), "empty")
        assert (m["cells"]["count"] == 0).all() and (m["cells"]["first"] == -1).all() and not m["start"].any()
        assert (cc.bits(m["cells"]["mass"]) == 0).all() and m["info"]["largest"] == 0 and m["info"]["largest_cell"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the lists are consistent with the sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_are_consistent_with_the_sums(dtype):
    n = 300
    P, V, M = cc.moving_state(n, dtype)
    f = cc.tenth_field(n)
    for grid in (cc.grid_of(4, 4, (0, f, 0, f)), cc.grid_of(9, 2, (0.2 * f, f, 0, 0.9 * f))):
        assert cc.lists_consistent(cc.model_cells(P, V, M, grid))
    P, V, M, bounds = cc.sized_state([1, 63, 64, 65, 129], dtype)
    res = cc.model_cells(P, V, M, cc.grid_of(8, 8, bounds))
    assert cc.lists_consistent(res)
    assert res["cells"]["count"].reshape(-1)[:6].tolist() == [1, 63, 64, 65, 129, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the order matters: a kernel that adds in another order fails the GPU comparisons
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, mass_cells, px_cells", [pytest.param(np.float32, 7, 13, id="f32"),
                                                         pytest.param(np.float64, 8, 10, id="f64")])
def test_the_order_matters(dtype, mass_cells, px_cells):
    """order_sensitive_state(300, dtype) on a 4 x 4 grid over [0, tenth_field(300))^2: the masses of 7 (fp32) and 8 (fp64) of the
    16 cells differ by bits between the ascending and the descending sum - the positions and masses are shell_cases' own, so
    those numbers are fixed by the state.  px depends on the velocities as well, which are cell_cases.velocities': 13 and 10
    of the 16 cells differ.  A kernel that adds in another order fails the GPU comparisons on this state."""
    n = 300
    P, V, M = cc.moving_state(n, dtype)
    f = cc.tenth_field(n)
    assert cc.order_matters(P, V, M, cc.grid_of(4, 4, (0, f, 0, f))) == (mass_cells, px_cells)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_order_matters_in_the_sized_states(dtype):
    P, V, M, bounds = cc.sized_state([1, 63, 64, 65, 129, 1000], dtype)
    mass, px = cc.order_matters(P, V, M, cc.grid_of(8, 8, bounds))
    assert mass >= 4 and px == 5                                # of the five cells with more than one member


# ---------------------------------------------------------------------------------------------------------------------
# 4. every argument check that needs no device
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks_without_a_device(nb):
    assert nb.lib.nbody_abi_version() == 2
    good = nb.make_grid(4, 3, (0.0, 8.0, 0.0, 6.0))
    cells = np.zeros(16, dtype=nb.CELL_DTYPE)
    info = np.zeros(1, dtype=nb.CELLS_INFO_DTYPE)
    lists = [np.zeros(32, dtype=np.int32) for _ in range(3)]
    fake = 1                                                    # a handle is only looked at after every value

    def ctx(grid, flags=0, cell_of=None, start=None, order=None, cap=32, handle=fake, cells_p=cells, info_p=info):
        return nb.lib.nbody_get_cells(handle, None if grid is None else grid.ctypes.data, flags,
                                      None if cells_p is None else cells_p.ctypes.data, cell_of, start, order, cap,
                                      None if info_p is None else info_p.ctypes.data)

    def batch(grid, flags=0, cell_of=None, start=None, order=None):
        return nb.lib.nbody_batch_get_cells(None, None if grid is None else grid.ctypes.data, flags, cells.ctypes.data, cell_of,
                                            start, order, info.ctypes.data)

    def changed(**kw):
        g = good.copy()
        for k, v in kw.items():
            g[k] = v
        return g

    bad_grids = [changed(nx=0), changed(ny=0), changed(nx=-3), changed(nx=1 << 10, ny=(1 << 10) + 1), changed(nx=1 << 20, ny=2),
                 changed(nx=1 << 16, ny=1 << 16),               # nx * ny wraps in 32 bits
                 changed(x0=np.nan), changed(x0=np.inf), changed(y0=-np.inf), changed(y0=np.nan),
                 changed(sx=0.0), changed(sx=-1.0), changed(sx=np.inf), changed(sx=np.nan),
                 changed(sy=0.0), changed(sy=-0.5), changed(sy=np.inf), changed(sy=np.nan)]
    for g in [None] + bad_grids:
        assert ctx(g, handle=None) == INVALID and batch(g) == INVALID, g
        assert b"cells" in nb.lib.nbody_last_error_string()
    for flags in (2, 4, 0x80000000, 3):
        assert ctx(good, flags=flags, handle=None) == INVALID and batch(good, flags=flags) == INVALID
        assert b"flags" in nb.lib.nbody_last_error_string()
    co, st, od = (a.ctypes.data for a in lists)
    assert ctx(good, order=od, handle=None) == INVALID and batch(good, order=od) == INVALID       # order needs start
    assert b"order without start" in nb.lib.nbody_last_error_string()
    assert ctx(good, cell_of=co, cap=-1, handle=None) == INVALID
    assert ctx(good, start=st, order=od, cap=-1, handle=None) == INVALID
    # the values come before the handle: with good values the NULL handle and the NULL results are what is left
    assert ctx(good, handle=None) == INVALID and b"NULL argument" in nb.lib.nbody_last_error_string()
    assert ctx(good, cell_of=co, start=st, order=od, handle=None) == INVALID
    assert b"NULL argument" in nb.lib.nbody_last_error_string()
    assert ctx(good, cells_p=None) == INVALID and ctx(good, info_p=None) == INVALID
    assert batch(good) == INVALID and b"NULL argument" in nb.lib.nbody_last_error_string()
    assert batch(changed(nx=1 << 10, ny=1 << 10)) == INVALID    # the largest grid passes its own check: the NULL batch is left
    assert b"NULL argument" in nb.lib.nbody_last_error_string()
    assert not cells.view(np.uint8).any() and not info.view(np.uint8).any()                       # nothing was written


# ---------------------------------------------------------------------------------------------------------------------
# 5. make_grid and cell_maps
# ---------------------------------------------------------------------------------------------------------------------
def test_make_grid(nb):
    g = nb.make_grid(256, bounds=(-5000.0, 5000.0, -2500.0, 2500.0))
    assert g.dtype == nb.GRID_DTYPE and g.dtype.itemsize == 40 and g.shape == (1,)
    assert (int(g["nx"][0]), int(g["ny"][0])) == (256, 256)
    assert g["sx"][0] == np.float64(256) / np.float64(10000.0) and g["sy"][0] == np.float64(256) / np.float64(5000.0)
    g = nb.make_grid(3, 7, (0.0, 0.3, 1.0, 1.7))
    assert cc.grid_tuple(g[0]) == cc.grid_of(3, 7, (0.0, 0.3, 1.0, 1.7))       # the same doubles as the model's
    again = nb.make_grid(g[0])
    assert again.tobytes() == g.tobytes() and nb.make_grid(g).tobytes() == g.tobytes()
    with pytest.raises(ValueError):
        nb.make_grid(4)
    assert nb.CELL_DTYPE == cc.CELL_DTYPE and nb.CELL_DTYPE.itemsize == 40 and nb.CELLS_INFO_DTYPE.itemsize == 24
    assert nb.CELLS_INFO_DTYPE.names == cc.INFO_FIELDS and nb.CELLS_MAX == 1 << 20 and nb.CELLS_MOMENTS == 1


def test_cell_maps_on_a_hand_made_result(nb):
    cells = np.zeros((1, 3), dtype=nb.CELL_DTYPE)
    # cell 0: two bodies of mass 1 moving at (+1, 0) and (-1, 0): mean 0, dispersion 1; cell 1: one body of mass 4 at (3, 4)
    cells[0, 0] = (2.0, 0.0, 0.0, 2.0, 2, 0)
    cells[0, 1] = (4.0, 12.0, 16.0, 100.0, 1, 2)
    cells[0, 2] = (0.0, 0.0, 0.0, 0.0, 0, -1)
    res = {"cells": cells, "grid": nb.make_grid(3, 1, (0.0, 6.0, 0.0, 4.0))[0]}
    maps = nb.cell_maps(res)
    assert maps["area"] == 8.0
    assert maps["surface_density"].tolist() == [[0.25, 0.5, 0.0]]
    assert maps["mean_velocity"][0, 0].tolist() == [0.0, 0.0] and maps["mean_velocity"][0, 1].tolist() == [3.0, 4.0]
    assert np.isnan(maps["mean_velocity"][0, 2]).all()
    assert maps["dispersion"][0, 0] == 1.0 and maps["dispersion"][0, 1] == 0.0 and np.isnan(maps["dispersion"][0, 2])
    assert maps["cic_mean"] == 1.0 and maps["cic_variance"] == pytest.approx(2.0 / 3.0) and maps["cic_ratio"] == pytest.approx(2.0 / 3.0)
    with pytest.raises(ValueError):
        nb.cell_maps({"cells": np.zeros((2, 1, 3), dtype=nb.CELL_DTYPE), "grid": res["grid"]})
