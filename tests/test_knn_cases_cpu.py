"""The numpy model of the k-nearest-neighbour queries (tests/knn_cases.py) against a plain scalar loop of the definition, the
consequences the header states (entry 0 is nbody_get_neighbors', prefixes, ties, padding, NaN), and what of nbody_get_knn /
nbody_batch_get_knn and their wrappers can be checked without a device: the exported symbols, the declarations, the bindings
and the argument handling."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import knn_cases as kc
import neighbor_cases as nc

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbody_get_knn", "nbody_batch_get_knn")


@pytest.fixture
def bound(nb):
    """The package, once it binds both symbols: every test of this file is about them."""
    for name in SYMBOLS:
        assert name in nb.SYMBOLS and hasattr(nb.lib, name), name
    return nb


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 40, 129])
def test_model_equals_the_plain_loop(bound, n, dtype):
    P, _ = kc.random_state(n, dtype, seed=n, field=40.0)
    pts = kc.probe_points(P, 19, seed=n + 1, field=40.0)
    for k in (1, 2, 5, 32):
        own = kc.model_knn(P, k)
        assert own["d2"].shape == (n, k) and own["index"].shape == (n, k) and own["index"].dtype == np.int32
        kc.assert_same(own, kc.loop_knn(P, k), "own form, k %d" % k)
        kc.check_invariants(own, rows=np.arange(n))
        exp = kc.model_knn(P, k, points=pts)
        kc.assert_same(exp, kc.loop_knn(P, k, points=pts), "explicit points, k %d" % k)
        kc.check_invariants(exp)
        rows = np.array([0, n - 1, n // 2])
        kc.assert_same(kc.model_knn(P, k, rows=rows), kc.sliced(own, rows), "a subset of the rows")
        kc.assert_same(kc.model_knn(P, k, chunk=7), own, "chunking")
        assert exp["d2"][0, 0] == 0 and exp["index"][0, 0] == 0      # a point on body 0: listed at +0, no self exclusion
        assert kc.same(kc.sliced(exp, slice(1, 2)), kc.sliced(exp, slice(-2, -1)))   # one point at two places


def test_lattice_ties_and_coincident_bodies(bound):
    P, _ = kc.lattice(8)
    for k in (4, 5, 8, 12):
        own = kc.model_knn(P, k)
        kc.assert_same(own, kc.loop_knn(P, k), "lattice, k %d" % k)
    own = kc.model_knn(P, 8)
    i = 3 * 8 + 3                                                     # interior: 4 at d2 = 1, then 4 at d2 = 2, each by index
    assert own["d2"][i].tolist() == [1.0] * 4 + [2.0] * 4
    assert own["index"][i].tolist() == [i - 8, i - 1, i + 1, i + 8, i - 9, i - 7, i + 7, i + 9]
    assert own["index"][0].tolist()[:3] == [1, 8, 9]                  # a corner: right, above, diagonal
    cell = kc.model_knn(P, 5, points=[[2.5, 3.5]])                    # the centre of a cell: four bodies at d2 = 1/2
    assert cell["d2"][0, :4].tolist() == [0.5] * 4 and cell["index"][0, :4].tolist() == [26, 27, 34, 35]
    Q = np.concatenate([P, P[[20, 20]]])                              # bodies 64 and 65 on body 20
    own = kc.model_knn(Q, 4)
    kc.assert_same(own, kc.loop_knn(Q, 4), "coincident")
    assert own["index"][20, :2].tolist() == [64, 65] and own["d2"][20, :2].tolist() == [0.0, 0.0]
    assert own["index"][64, :2].tolist() == [20, 65] and own["index"][65, :2].tolist() == [20, 64]
    assert not np.signbit(own["d2"][20, 0])
    assert own["index"][12, :4].tolist() == [4, 11, 13, 20]           # below 20: 20 before its twins 64, 65 at d2 = 1 ...
    assert kc.model_knn(Q, 6)["index"][12].tolist() == [4, 11, 13, 20, 64, 65]   # ... which follow by index


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_entry_0_is_the_nearest_neighbour(bound, dtype):
    P, R = kc.random_state(300, dtype, seed=4, field=30.0)
    P[150] = P[20]
    P[77, 0] = np.nan
    pts = kc.probe_points(P, 40, seed=5, field=30.0)
    near, near_pts = nc.model_neighbors(P, R), nc.model_neighbors(P, R, points=pts)
    for k in (1, 3, 32):
        own, exp = kc.model_knn(P, k), kc.model_knn(P, k, points=pts)
        assert np.array_equal(kc.bits(own["d2"][:, 0]), kc.bits(near["d2"])) and np.array_equal(own["index"][:, 0], near["index"])
        assert np.array_equal(kc.bits(exp["d2"][:, 0]), kc.bits(near_pts["d2"])) and np.array_equal(exp["index"][:, 0], near_pts["index"])


def test_prefix_property(bound):
    P, _ = kc.random_state(200, np.float32, seed=6, field=20.0)
    P[[5, 6, 7]] = P[4]
    full = kc.model_knn(P, 32)
    for k in (1, 2, 4, 5, 8, 9, 16, 17, 31):
        kc.assert_same(kc.model_knn(P, k), kc.sliced(full, (slice(None), slice(0, k))), "k %d of 32" % k)


@pytest.mark.parametrize("n", [1, 2, 5, 32])
def test_k_at_or_above_n_pads(bound, n):
    P, _ = kc.random_state(n, np.float64, seed=n + 20)
    for k in (n - 1, n, n + 1, 32):
        if not 1 <= k <= 32:
            continue
        own = kc.model_knn(P, k)
        kc.assert_same(own, kc.loop_knn(P, k), "n %d k %d" % (n, k))
        live = min(k, n - 1)
        assert (own["index"][:, :live] >= 0).all() and (own["index"][:, live:] == -1).all()
        assert (own["d2"][:, live:] == np.inf).all() and (own["d2"][:, :live] < np.inf).all()
        exp = kc.model_knn(P, k, points=[[1.0, 2.0]])
        assert (exp["index"][0, :min(k, n)] >= 0).all() and (exp["index"][0, n:] == -1).all()


def test_nan_rows_and_empty_systems(bound):
    P, _ = kc.random_state(40, np.float64, seed=2, field=10.0)
    P[7, 0] = np.nan
    P[9, 1] = 1e200                                                   # squares to +inf: not eligible
    own = kc.model_knn(P, 5)
    kc.assert_same(own, kc.loop_knn(P, 5), "NaN and 1e200")
    for i in (7, 9):
        assert (own["index"][i] == -1).all() and (own["d2"][i] == np.inf).all()
    assert not np.isin(own["index"], [7, 9]).any()
    keep = np.delete(np.arange(40), [7, 9])                           # the rest is the state without the two
    sub = kc.model_knn(P[keep], 5)
    assert np.array_equal(kc.bits(own["d2"][keep]), kc.bits(sub["d2"])) and np.array_equal(own["index"][keep], keep[sub["index"]])
    exp = kc.model_knn(P, 3, points=[[np.nan, 1.0], [np.inf, 0.0], [1e200, 1.0]])
    assert (exp["index"] == -1).all() and (exp["d2"] == np.inf).all()
    none = kc.model_knn(np.zeros((0, 2)), 4, points=[[1.0, 2.0], [3.0, 4.0]])
    assert none["d2"].shape == (2, 4) and (none["index"] == -1).all() and (none["d2"] == np.inf).all()
    assert kc.model_knn(np.zeros((0, 2)), 4)["d2"].shape == (0, 4)


def test_assert_same_rejects_a_wrong_answer(bound):
    P, _ = kc.random_state(50, np.float64, seed=8)
    own = kc.model_knn(P, 4)
    kc.assert_same(own, {"d2": own["d2"].copy(), "index": own["index"].copy()})
    ulp = {"d2": own["d2"].copy(), "index": own["index"]}
    ulp["d2"][3, 2] = np.nextafter(ulp["d2"][3, 2], np.inf)           # one bit of one entry
    swapped = {"d2": own["d2"], "index": own["index"].copy()}
    swapped["index"][7, [0, 1]] = swapped["index"][7, [1, 0]]
    zero = {"d2": np.where(own["d2"] == 0, -0.0, own["d2"]), "index": own["index"]}
    zero["d2"][0, 0] = -0.0                                           # equal as a number, not by bits
    for wrong in (ulp, swapped, zero, kc.sliced(own, slice(0, 49)), kc.model_knn(P, 3)):
        assert not kc.same(wrong, own)
        with pytest.raises(AssertionError):
            kc.assert_same(wrong, own)
    with pytest.raises(AssertionError):
        kc.check_invariants(own, rows=own["index"][:, 0])             # a row that lists itself
    unsorted = {"d2": own["d2"][:, ::-1], "index": own["index"][:, ::-1]}
    with pytest.raises(AssertionError):
        kc.check_invariants(unsorted)


def test_library_header_and_bindings(bound):
    nb = bound
    exported = subprocess.check_output(["nm", "-D", "--defined-only", nb.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"^#define NBODY_KNN_MAX 32$", header, re.M) and nb.KNN_MAX == 32 == kc.KNN_MAX
    assert re.search(r"^#define NBODY_ABI_VERSION 2$", header, re.M)
    assert nb.lib.nbody_abi_version() == 2
    assert len(nb.SYMBOLS["nbody_get_knn"][1]) == 7 and len(nb.SYMBOLS["nbody_batch_get_knn"][1]) == 6
    for cls in (nb.Stepper, nb.StepperGroup, nb.StepperBatch):
        assert callable(getattr(cls, "knn"))


def test_null_handles_and_bad_k_are_invalid(bound):
    nb = bound
    d2 = np.full(8, 7.0)
    index = np.full(8, 7, dtype=np.int32)
    n = ctypes.c_int(7)
    assert nb.lib.nbody_get_knn(None, None, 4, 2, d2.ctypes.data, index.ctypes.data, ctypes.byref(n)) == INVALID
    assert b"nbody_get_knn" in nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_batch_get_knn(None, None, 4, 2, d2.ctypes.data, index.ctypes.data) == INVALID
    assert b"nbody_batch_get_knn" in nb.lib.nbody_last_error_string()
    for k in (0, 33, -1):
        assert nb.lib.nbody_get_knn(None, None, 4, k, d2.ctypes.data, index.ctypes.data, ctypes.byref(n)) == INVALID
        assert nb.lib.nbody_batch_get_knn(None, None, 4, k, d2.ctypes.data, index.ctypes.data) == INVALID
    assert n.value == 7 and (d2 == 7.0).all() and (index == 7).all()


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("points", [[1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros((2, 2, 2)), 5.0, np.zeros((2, 0))])
def test_wrong_points_shape_raises_before_the_library(bound, points):
    with pytest.raises(ValueError):
        bound.Stepper.knn(_NoLibrary(), 3, points)
    with pytest.raises(ValueError):
        bound.StepperBatch.knn(_NoLibrary(), 3, points)
