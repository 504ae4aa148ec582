"""The numpy model of the neighbour queries (tests/neighbor_cases.py) against a plain scalar loop of the definition and against
exact rational arithmetic, the consequences the header states (ties, coincident bodies, NaN and huge coordinates, symmetry),
and what of nbody_get_neighbors / nbody_batch_get_neighbors and their wrappers can be checked without a device: the record
layout and the argument handling."""
import ctypes

import numpy as np
import pytest

import neighbor_cases as nc

INVALID = -1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 129, 300])
def test_model_equals_the_plain_loop(n, dtype):
    P, R = nc.random_state(n, dtype, seed=n, field=40.0)          # dense: overlaps are plentiful
    own = nc.model_neighbors(P, R)
    nc.assert_same(own, nc.loop_neighbors(P, R), "own form")
    assert n < 100 or own["overlaps"].sum() > n // 4
    pts = nc.probe_points(P, 37, seed=n + 1, field=40.0)
    exp = nc.model_neighbors(P, R, points=pts)
    nc.assert_same(exp, nc.loop_neighbors(P, R, points=pts), "explicit points")
    rows = np.array([0, n - 1, n // 2])
    nc.assert_same(nc.model_neighbors(P, R, rows=rows), own[rows], "a subset of the rows")
    nc.assert_same(nc.model_neighbors(P, R, chunk=7), own, "chunking")
    if n == 1:
        assert tuple(own[0]) == nc.EMPTY                          # no eligible source
    assert nc.same(exp[1:2], exp[-2:-1])                          # the same point at two places of `points`
    # a point on a body sees it at d2 = +0 and overlaps it whatever its radius
    assert exp["d2"][0] == 0 and exp["overlaps"][0] >= 1 and not np.signbit(exp["d2"][0])


def test_no_sources():
    got = nc.model_neighbors(np.zeros((0, 2)), np.zeros(0), points=[[1.0, 2.0], [3.0, 4.0]])
    assert [tuple(r) for r in got] == [nc.EMPTY, nc.EMPTY]
    assert len(nc.model_neighbors(np.zeros((0, 2)), np.zeros(0))) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_exact_check_on_random_states(dtype):
    P, R = nc.random_state(200, dtype, seed=5)
    own = nc.model_neighbors(P, R)
    nc.exact_check(P, R, own, sample=[0, 1, 63, 64, 127, 128, 199])
    pts = nc.probe_points(P, 24, seed=6, field=100.0)
    nc.exact_check(P, R, nc.model_neighbors(P, R, points=pts), points=pts)
    rows = np.array([5, 150])
    nc.exact_check(P, R, nc.model_neighbors(P, R, rows=rows), rows=rows)


def test_exact_check_rejects_a_wrong_answer():
    P, R = nc.random_state(50, np.float64, seed=8)
    own = nc.model_neighbors(P, R)
    bad = own.copy()
    bad["d2"][3] = np.nextafter(np.nextafter(np.nextafter(bad["d2"][3], np.inf), np.inf), np.inf)   # 3 ulps can be 6 u
    bad["d2"][3] *= 1 + 2.0 ** -49
    with pytest.raises(AssertionError):
        nc.exact_check(P, R, bad, sample=[3])
    far = own.copy()
    far["index"][4] = int(np.argmax(((P - P[4]) ** 2).sum(axis=1)))
    with pytest.raises(AssertionError):
        nc.exact_check(P, R, far, sample=[4])


def test_ties_go_to_the_lowest_index():
    P, R = nc.lattice(8)
    own = nc.model_neighbors(P, R)
    assert (own["d2"] == 1.0).all()
    assert np.array_equal(own["index"], nc.lattice_expected(8))
    interior = [i for i in range(64) if 0 < i // 8 < 7 and 0 < i % 8 < 7]
    assert all(own["index"][i] == i - 8 for i in interior)        # four candidates, the lowest wins
    assert (own["overlaps"] == 0).all()                           # radii 1/4: 1 <= 1/4 is false
    touching = nc.model_neighbors(P, np.full(64, 0.5))            # d2 = 1 <= (1/2 + 1/2)^2: equality counts
    assert touching["overlaps"][9] == 4 and touching["overlaps"][0] == 2 and touching["overlaps"][1] == 3
    nc.assert_same(own, nc.loop_neighbors(P, R))
    # the centre of a cell: four bodies at d2 = 1/2, the lowest of them wins
    cell = nc.model_neighbors(P, R, points=[[2.5, 3.5]])
    assert cell["d2"][0] == 0.5 and cell["index"][0] == 3 * 8 + 2


def test_coincident_bodies():
    P = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])
    zero = nc.model_neighbors(P, np.zeros(3))
    assert zero["d2"][0] == 0 and not np.signbit(zero["d2"][0]) and zero["index"][0] == 2 and zero["index"][2] == 0
    assert zero["overlaps"].tolist() == [1, 0, 1]                 # each other's overlap even at radii 0: 0 <= 0
    assert zero["index"][1] == 0 and zero["d2"][1] == 49.0 + 36.0  # a tie between 0 and 2: the lowest
    nc.assert_same(zero, nc.loop_neighbors(P, np.zeros(3)))


def test_nan_and_huge_coordinates():
    P, R = nc.random_state(40, np.float64, seed=2, field=10.0, radius=2.0)
    clean = nc.model_neighbors(P, R)
    Pn = P.copy()
    Pn[7, 0] = np.nan                                             # a NaN coordinate: every d2 with body 7 is NaN
    got = nc.model_neighbors(Pn, R)
    nc.assert_same(got, nc.loop_neighbors(Pn, R))
    assert tuple(got[7]) == nc.EMPTY                              # its own row has no eligible source
    assert (got["index"] != 7).all()                              # never the nearest ...
    others = np.arange(40) != 7
    keep = np.delete(np.arange(40), 7)
    sub = nc.model_neighbors(P[keep], R[keep])                    # ... and never an overlap: the rest is the state without it
    assert np.array_equal(got["overlaps"][others], sub["overlaps"])
    assert np.array_equal(got["d2"][others], sub["d2"]) and np.array_equal(keep[sub["index"]], got["index"][others])
    Ph = P.copy()
    Ph[7, 1] = 1e200                                              # squares to +inf: never the nearest
    got = nc.model_neighbors(Ph, R)
    nc.assert_same(got, nc.loop_neighbors(Ph, R))
    assert tuple(got[7]) == nc.EMPTY and (got["index"] != 7).all()
    assert np.array_equal(got["overlaps"][others], sub["overlaps"])   # +inf <= s*s is false for finite radii: no overlap
    Rh = R.copy()
    Rh[3] = 1e200                                                 # s*s = +inf: +inf <= +inf, the one case a +inf d2 counts
    got = nc.model_neighbors(Ph, Rh)
    nc.assert_same(got, nc.loop_neighbors(Ph, Rh))
    assert got["overlaps"][7] == 1 and got["overlaps"][3] == 39 and got["index"][7] == -1
    Rn = R.copy()
    Rn[5] = np.nan                                                # a NaN radius: s*s is NaN, body 5 overlaps nothing
    got = nc.model_neighbors(P, Rn)
    nc.assert_same(got, nc.loop_neighbors(P, Rn))
    assert got["overlaps"][5] == 0 and np.array_equal(got["d2"], clean["d2"]) and np.array_equal(got["index"], clean["index"])
    pts = np.array([[np.nan, 1.0], [1e200, 1.0], [np.inf, 0.0]])
    got = nc.model_neighbors(P, R, points=pts)
    assert [tuple(r) for r in got] == [nc.EMPTY] * 3


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_overlaps_are_symmetric(dtype):
    P, R = nc.random_state(300, dtype, seed=12, field=30.0)
    X, Y = P[:, 0], P[:, 1]
    dx, dy = X[None, :] - X[:, None], Y[None, :] - Y[:, None]
    d2 = dx * dx + dy * dy
    assert np.array_equal(d2.view(np.uint64), d2.T.view(np.uint64))   # d2_ij and d2_ji: the same bits
    s = R[:, None] + R[None, :]
    hit = (d2 <= s * s) & ~np.eye(300, dtype=bool)
    assert np.array_equal(hit, hit.T)
    own = nc.model_neighbors(P, R)
    assert np.array_equal(own["overlaps"], hit.sum(axis=1)) and own["overlaps"].sum() % 2 == 0 and own["overlaps"].sum() > 0


def test_record_layout(nb):
    assert ctypes.sizeof(nb.Neighbor) == 16
    assert (nb.Neighbor.d2.offset, nb.Neighbor.index.offset, nb.Neighbor.overlaps.offset) == (0, 8, 12)
    assert nb.NEIGHBOR_DTYPE.itemsize == 16 and nb.NEIGHBOR_DTYPE == nc.DTYPE
    assert [nb.NEIGHBOR_DTYPE.fields[k][1] for k in ("d2", "index", "overlaps")] == [0, 8, 12]
    assert nb.NEIGHBOR_DTYPE["d2"] == np.float64 and nb.NEIGHBOR_DTYPE["index"] == np.int32


def test_null_handles_are_invalid(nb):
    out = (nb.Neighbor * 4)()
    n = ctypes.c_int(7)
    assert nb.lib.nbody_get_neighbors(None, None, 4, out, ctypes.byref(n)) == INVALID
    assert b"nbody_get_neighbors" in nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_batch_get_neighbors(None, None, 4, out) == INVALID
    assert b"nbody_batch_get_neighbors" in nb.lib.nbody_last_error_string()
    assert n.value == 7 and out[0].index == 0


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("points", [[1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros((2, 2, 2)), 5.0, np.zeros((2, 0))])
def test_wrong_points_shape_raises_before_the_library(nb, points):
    with pytest.raises(ValueError):
        nb.Stepper.neighbors(_NoLibrary(), points)
    with pytest.raises(ValueError):
        nb.StepperBatch.neighbors(_NoLibrary(), points)
