"""The numpy model of the shell sums (tests/shell_cases.py) against a plain scalar loop of the definition, the consequences
the header states (equality at the edges, unit masses, the row sums against the pair counts, independent bins, NaN and +inf
separations, coincident bodies, mass 0 and a NaN mass), the condition that lets the GPU tests tell a wrong order of the mass
sum from the right one, shell_profile, and what of nbody_get_shells / nbody_batch_get_shells and their wrappers can be checked
without a device: the exported symbols, the declarations, the bindings and the argument checks that come before any device
call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pair_cases as pc
import shell_cases as shc

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbody_get_shells", "nbody_batch_get_shells")
LATTICE_EDGES2 = np.array([0.0, 1.0, 2.0, 4.0, 5.0])
# lattice(8): unordered pairs at d2 = 1, 2, 4, 5: 2*8*7, 2*7*7, 2*8*6, 4*7*6 (test_pair_cases_cpu.py); a row sees each twice
LATTICE_AT = {1.0: 112, 2.0: 98, 4.0: 96, 5.0: 168}


@pytest.fixture
def bound(nb):
    """The package, once it binds both symbols: every test of this file is about them."""
    for name in SYMBOLS:
        assert name in nb.SYMBOLS and hasattr(nb.lib, name), name
    return nb


def edge_sets(field):
    """test_pair_cases_cpu.py's, the geometric one cut to 32 bins."""
    top = (0.3 * field) ** 2
    return [np.linspace(0.0, top, 9), np.array([0.0, np.inf]), np.array([4.0, 9.0]), np.geomspace(1e-3, 4 * field * field, 33)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 2, 50])
def test_model_equals_the_plain_loop(bound, n, dtype):
    P, M = shc.order_sensitive_state(n, dtype, seed=n + 1, field=20.0)
    pts = np.random.default_rng(n).uniform(-2, 22, size=(7, 2))
    if n:
        pts[3] = P[n // 2]                                       # a point on a body: d2 = +0, counted
    for e2 in edge_sets(20.0):
        B = len(e2) - 1
        got = shc.model_shells(P, M, e2)
        assert got["mass"].shape == (n, B) and got["count"].shape == (n, B) and got["count"].dtype == np.int32
        shc.assert_same(got, shc.loop_shells(P, M, e2), "own form, n %d, %d bins" % (n, B))
        for m in (0, 1, 7):
            got = shc.model_shells(P, M, e2, pts[:m])
            assert got["mass"].shape == (m, B)
            shc.assert_same(got, shc.loop_shells(P, M, e2, pts[:m]), "points form, n %d, m %d, %d bins" % (n, m, B))
    whole = shc.model_shells(P, M, [0.0, np.inf])
    assert (whole["count"] == max(n - 1, 0)).all()               # every other body, once
    on = shc.model_shells(P, M, [0.0, 1e-300], pts[3:4])
    assert on["count"].tolist() == [[1 if n else 0]] and on["mass"].tolist() == [[M[n // 2] if n else 0.0]]


def test_lattice_equality_at_the_edges(bound):
    P, _ = shc.lattice(8)
    M = np.ones(64)
    for d2, k in LATTICE_AT.items():                             # the closed forms, one value at a time: ordered pairs
        assert int(shc.model_shells(P, M, [d2, np.nextafter(d2, np.inf)])["count"].sum()) == 2 * k
    got = shc.model_shells(P, M, LATTICE_EDGES2)
    shc.assert_same(got, shc.loop_shells(P, M, LATTICE_EDGES2))
    assert got["count"].sum(axis=0).tolist() == [0, 224, 196, 192]       # e2[k] <= d2: the lower edge belongs to the bin
    assert got["count"][3 * 8 + 3].tolist() == [0, 4, 4, 4]              # an interior body; d2 == 5 is not below the top
    down = np.concatenate([[0.0], np.nextafter(LATTICE_EDGES2[1:], -np.inf)])    # one ulp down: every integer d2 stays
    assert shc.model_shells(P, M, down)["count"].sum(axis=0).tolist() == [0, 224, 196, 192]
    up = np.concatenate([[0.0], np.nextafter(LATTICE_EDGES2[1:], np.inf)])       # one ulp up: one bin down, d2 == 5 comes in
    got = shc.model_shells(P, M, up)
    shc.assert_same(got, shc.loop_shells(P, M, up))
    assert got["count"].sum(axis=0).tolist() == [224, 196, 192, 336]
    assert np.array_equal(got["mass"], got["count"].astype(np.float64))  # unit masses


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_unit_masses_row_sums_and_independent_bins(bound, dtype):
    n = 60
    P, M = shc.order_sensitive_state(n, dtype, seed=9, field=15.0)
    pts = shc.probe_points(P, 23, seed=4, field=15.0)
    for e2 in (np.linspace(0.0, 40.0, 6), np.array([0.0, np.inf]), np.array([4.0, 9.0]), np.geomspace(1e-3, 900.0, 33)):
        unit_own, unit_pts = shc.model_shells(P, np.ones(n), e2), shc.model_shells(P, np.ones(n), e2, pts)
        for unit in (unit_own, unit_pts):                        # where every mass is 1.0, mass == count exactly
            assert np.array_equal(shc.bits(unit["mass"]), shc.bits(unit["count"].astype(np.float64)))
        own, exp = shc.model_shells(P, M, e2), shc.model_shells(P, M, e2, pts)
        assert np.array_equal(own["count"], unit_own["count"]) and np.array_equal(exp["count"], unit_pts["count"])
        dd, dr = pc.model_pair_counts(P, e2), pc.model_pair_counts(P, e2, pts)
        assert own["count"].sum(axis=0, dtype=np.int64).tolist() == (2 * dd["counts"].astype(np.int64)).tolist()
        assert exp["count"].sum(axis=0, dtype=np.int64).tolist() == dr["counts"].astype(np.int64).tolist()
        for k in range(len(e2) - 1):                             # bin k alone: the same bits
            shc.assert_same(shc.model_shells(P, M, e2[k:k + 2]), {"mass": own["mass"][:, k:k + 1], "count": own["count"][:, k:k + 1]},
                            "bin %d alone" % k)
            shc.assert_same(shc.model_shells(P, M, e2[k:k + 2], pts), {"mass": exp["mass"][:, k:k + 1], "count": exp["count"][:, k:k + 1]},
                            "bin %d alone, points" % k)
    one = shc.model_shells(P, M, [0.0, 30.0], pts[5:6])          # the row's place in `points` plays no part
    assert shc.same(one, shc.sliced(shc.model_shells(P, M, [0.0, 30.0], pts), slice(5, 6)))


def test_awkward_values(bound):
    n = 40
    P, M = shc.order_sensitive_state(n, np.float64, seed=3, field=10.0)
    e2 = np.array([0.0, 1.0, 50.0, np.inf])
    clean = shc.model_shells(P, M, e2)
    assert (clean["count"].sum(axis=1) == n - 1).all()
    Pn = P.copy()
    Pn[5, 0] = np.nan                                            # counted nowhere, its own row empty, top edge +inf or not
    got = shc.model_shells(Pn, M, e2)
    shc.assert_same(got, shc.loop_shells(Pn, M, e2))
    assert (got["count"][5] == 0).all() and (got["mass"][5] == 0).all() and (np.delete(got["count"], 5, 0).sum(axis=1) == n - 2).all()
    Pi = P.copy()
    Pi[5] = [1e200, 0.0]                                         # d2 = +inf fails d2 < +inf
    got = shc.model_shells(Pi, M, e2)
    shc.assert_same(got, shc.loop_shells(Pi, M, e2))
    assert (got["count"][5] == 0).all() and (np.delete(got["count"], 5, 0).sum(axis=1) == n - 2).all()
    C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])         # two bodies at one place: d2 = +0
    Mc = np.array([5.0, 7.0, 11.0])
    got = shc.model_shells(C, Mc, [0.0, 1.0])
    assert got["count"].tolist() == [[1], [0], [1]] and got["mass"].tolist() == [[11.0], [0.0], [5.0]]
    got = shc.model_shells(C, Mc, [1e-300, 1.0])                 # below the first edge: counted nowhere
    assert got["count"].tolist() == [[0], [0], [0]] and not got["mass"].any()
    Mz = M.copy()
    Mz[7] = 0.0                                                  # a body of mass 0 counts and adds +0
    got = shc.model_shells(P, Mz, e2)
    shc.assert_same(got, shc.loop_shells(P, Mz, e2))
    assert np.array_equal(got["count"], clean["count"]) and not np.signbit(got["mass"]).any()
    Mn = M.copy()
    Mn[7] = np.nan                                               # a NaN mass: its bin's mass is NaN, and it still counts
    got = shc.model_shells(P, Mn, e2)
    shc.assert_same(got, shc.loop_shells(P, Mn, e2))
    assert np.array_equal(got["count"], clean["count"])
    d2_7 = ((P[:, 0] - P[7, 0]) ** 2) + ((P[:, 1] - P[7, 1]) ** 2)
    has7 = (e2[:-1][None, :] <= d2_7[:, None]) & (d2_7[:, None] < e2[1:][None, :])
    has7[7] = False
    assert np.array_equal(np.isnan(got["mass"]), has7)
    assert np.array_equal(shc.bits(got["mass"][~has7]), shc.bits(clean["mass"][~has7]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_shared_state_is_sensitive_to_the_order(bound, dtype):
    """What lets test_gpu_shells.py tell a device that adds in another order from one that keeps the contract: with
    ORDER_SEED, for the edges that test uses, the model's mass differs from the sum in descending j in many (row, bin)."""
    n = 300
    P, M = shc.order_sensitive_state(n, dtype)
    assert M.min() >= 1e4 and M.max() <= 1.0001e17 and M.max() / M.min() > 1e10
    e2 = shc.tenth_edges(shc.tenth_field(n))
    differ = shc.order_matters(P, M, e2)
    print("n %d, %s: %d of %d (row, bin) masses depend on the order" % (n, np.dtype(dtype).name, differ, n * 8))
    assert differ >= 1
    assert shc.order_matters(P, M, [0.0, np.inf]) >= 1 and shc.order_matters(P, M, e2, P[:37] + 0.25) >= 1
    got = shc.model_shells(P, M, e2)
    assert (got["count"].sum(axis=0) > 0).all() and (got["count"].sum(axis=1) < n - 1).any()    # bins in use, sources outside


def test_shell_profile(bound):
    nb = bound
    rec = {"mass": np.array([[1.0, 3.0, 4.0], [0.0, 0.0, 0.0], [0.0, 8.0, 0.0]]),
           "count": np.array([[1, 2, 1], [0, 0, 0], [0, 3, 0]], dtype=np.int32), "edges2": np.array([1.0, 4.0, 9.0, 25.0])}
    p = nb.shell_profile(rec)
    area = np.pi * np.array([3.0, 5.0, 16.0])
    assert np.array_equal(p["area"], area)
    assert np.array_equal(p["surface_density"], rec["mass"] / area) and np.array_equal(p["number_density"], rec["count"] / area)
    assert p["enclosed_mass"].tolist() == [[1.0, 4.0, 8.0], [0.0, 0.0, 0.0], [0.0, 8.0, 8.0]]
    assert p["enclosed_count"].tolist() == [[1, 3, 4], [0, 0, 0], [0, 3, 3]]
    half = p["half_mass_radius2"]                                # row 0: 4 of 8 is reached at the second bin's upper edge
    assert half[0] == 9.0 and np.isnan(half[1]) and half[2] == 9.0
    with pytest.raises(ValueError):
        nb.shell_profile({"mass": rec["mass"], "count": rec["count"], "edges2": rec["edges2"][:3]})


def test_library_header_and_bindings(bound):
    nb = bound
    exported = subprocess.check_output(["nm", "-D", "--defined-only", nb.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
    assert re.search(r"^#define NBODY_SHELLS_MAX 32$", header, re.M) and nb.SHELLS_MAX == 32 == shc.SHELLS_MAX
    assert nb.lib.nbody_abi_version() == 2
    assert len(nb.SYMBOLS["nbody_get_shells"][1]) == 8 and len(nb.SYMBOLS["nbody_batch_get_shells"][1]) == 7
    for cls in (nb.Stepper, nb.StepperGroup, nb.StepperBatch):
        assert callable(getattr(cls, "shells"))
    assert callable(nb.shell_profile)


def test_bad_arguments_are_invalid_before_any_device_call(bound):
    """From a NULL handle: the values are checked before the handle, so each refusal can be seen here, with its reason."""
    nb = bound
    mass = np.full(8, 7.0)
    count = np.full(8, 7, dtype=np.int32)
    n = ctypes.c_int(7)
    good = np.array([0.0, 1.0, 4.0])
    Mp, Cp, Np = mass.ctypes.data, count.ctypes.data, ctypes.byref(n)

    def one(m, e2, bins, mass=Mp, count=Cp, n_out=Np):
        return nb.lib.nbody_get_shells(None, None, m, None if e2 is None else e2.ctypes.data, bins, mass, count, n_out)

    def many(m, e2, bins, mass=Mp, count=Cp):
        return nb.lib.nbody_batch_get_shells(None, None, m, None if e2 is None else e2.ctypes.data, bins, mass, count)

    for call, name in ((one, b"nbody_get_shells"), (many, b"nbody_batch_get_shells")):
        def refused(reason, *a, **kw):
            assert call(*a, **kw) == INVALID
            msg = nb.lib.nbody_last_error_string()
            assert msg.startswith(name + b": ") and reason in msg, msg

        refused(b"NULL", 4, good, 2)                             # the handle
        refused(b"NULL", 4, None, 2)                             # edges2
        refused(b"NULL", 4, good, 2, mass=None)
        refused(b"NULL", 4, good, 2, count=None)
        for bins in (0, 33, -1):
            refused(b"bins = %d (1 .. 32)" % bins, 4, np.arange(34.0), bins)
        refused(b"m = -1", -1, good, 2)
        refused(b"edges2[0] = nan", 4, np.array([np.nan, 1.0, 4.0]), 2)
        refused(b"edges2[2]", 4, np.array([0.0, 1.0, np.nan]), 2)
        refused(b"edges2[0] = -1", 4, np.array([-1.0, 1.0, 4.0]), 2)
        refused(b"edges2[2] = 1 is not above edges2[1] = 1", 4, np.array([0.0, 1.0, 1.0]), 2)
        refused(b"edges2[1] = 0.5 is not above edges2[0] = 2", 4, np.array([2.0, 0.5, 4.0]), 2)
        refused(b"more than 2^31 bytes of results", (1 << 31) // (12 * 2) + 1, good, 2)     # m x bins x 12 bytes
        refused(b"more than 2^31 bytes of results", (1 << 31) // (12 * 32) + 1, np.arange(33.0), 32)
        refused(b"NULL", (1 << 31) // (12 * 2), good, 2)         # the largest m that passes: on to the handle
        refused(b"NULL", 4, np.array([0.0, 1.0, np.inf]), 2)     # a +inf top edge is legal
    assert one(4, good, 2, n_out=None) == INVALID and b"nbody_get_shells: NULL" in nb.lib.nbody_last_error_string()
    assert n.value == 7 and (mass == 7.0).all() and (count == 7).all()


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("edges", [[1.0], [[0.0, 1.0]], [], [0.0, -1.0, 2.0]])
def test_wrong_edges_raise_before_the_library(bound, edges):
    with pytest.raises(ValueError):
        bound.Stepper.shells(_NoLibrary(), edges)
    with pytest.raises(ValueError):
        bound.StepperBatch.shells(_NoLibrary(), edges)
