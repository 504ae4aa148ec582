"""The numpy model of the shell moments (tests/shell_moment_cases.py) against a plain scalar loop of the definition, the
consequences the header states (mass and count with the bits of the shell sums, independent bins, sources at rest, unit
masses, a NaN velocity), the condition that lets the GPU tests tell a wrong order of any of the nine sums from the right one,
shell_kinematics, and what of nbody_get_shell_moments / nbody_batch_get_shell_moments and their wrappers can be checked without
a device: the exported symbols, the declarations, the bindings and the argument checks that come before any device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import shell_cases as shc
import shell_moment_cases as smc

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("nbody_get_shell_moments", "nbody_batch_get_shell_moments")


@pytest.fixture
def bound(nb):
    """The package, once it binds both symbols: every test of this file is about them."""
    for name in SYMBOLS:
        assert name in nb.SYMBOLS and hasattr(nb.lib, name), name
    return nb


def edge_sets(field):
    top = (0.3 * field) ** 2
    return [np.linspace(0.0, top, 9), np.array([0.0, np.inf]), np.array([4.0, 9.0]), np.geomspace(1e-3, 4 * field * field, 6)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 65, 130])
def test_model_equals_the_plain_loop(bound, n, dtype):
    field = 20.0
    P, V, M = smc.moment_state(n, dtype, seed=n + 1, field=field)
    allpts = smc.probe_points(P, 37, seed=n, field=field)        # the first 9 ON bodies: d2 = +0, counted
    allvel = smc.point_velocities(37, seed=n)
    for e2 in edge_sets(field):
        B = len(e2) - 1
        got = smc.model_shell_moments(P, V, M, e2)
        assert got["moments"].shape == (n, B) and got["moments"].dtype == smc.DTYPE
        smc.assert_same(got, smc.loop_shell_moments(P, V, M, e2), "own form, n %d, %d bins" % (n, B))
        for m in (0, 1, 37):
            for vel in (None, allvel[:m]):
                got = smc.model_shell_moments(P, V, M, e2, allpts[:m], vel)
                assert got["moments"].shape == (m, B)
                smc.assert_same(got, smc.loop_shell_moments(P, V, M, e2, allpts[:m], vel),
                                "points form, n %d, m %d, %d bins, velocities %s" % (n, m, B, vel is not None))
    whole = smc.model_shell_moments(P, V, M, [0.0, np.inf])["moments"]
    assert (whole["count"] == n - 1).all()                       # every other body, once
    # a point at rest and a point with a velocity of zeros: the same bits
    at_rest = smc.model_shell_moments(P, V, M, [0.0, 900.0], allpts)
    smc.assert_same(at_rest, smc.model_shell_moments(P, V, M, [0.0, 900.0], allpts, np.zeros((37, 2))), "zeros against None")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mass_and_count_have_the_bits_of_the_shell_sums(bound, dtype):
    n = 130
    P, V, M = smc.moment_state(n, dtype, seed=9, field=15.0)
    pts = smc.probe_points(P, 23, seed=4, field=15.0)
    vel = smc.point_velocities(23, seed=4)
    for e2 in (np.linspace(0.0, 40.0, 6), np.array([0.0, np.inf]), np.array([4.0, 9.0]), np.geomspace(1e-3, 900.0, 9)):
        for points, pv in ((None, None), (pts, None), (pts, vel)):
            mom = smc.model_shell_moments(P, V, M, e2, points, pv)["moments"]
            sums = shc.model_shells(P, M, e2, points)
            assert np.array_equal(smc.bits(mom["mass"]), smc.bits(sums["mass"])) and np.array_equal(mom["count"], sums["count"])
            assert mom["count"].sum() > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_independent_bins_rows_and_unit_masses(bound, dtype):
    n = 65
    P, V, M = smc.moment_state(n, dtype, seed=5, field=15.0)
    pts = smc.probe_points(P, 23, seed=4, field=15.0)
    vel = smc.point_velocities(23, seed=8)
    e2 = np.geomspace(0.5, 900.0, 9)
    own = smc.model_shell_moments(P, V, M, e2)["moments"]
    exp = smc.model_shell_moments(P, V, M, e2, pts, vel)["moments"]
    assert (own["count"].sum(axis=0) > 0).sum() >= 6
    for k in range(len(e2) - 1):                                 # bin k alone: the same bits
        smc.assert_same(smc.model_shell_moments(P, V, M, e2[k:k + 2])["moments"], own[:, k:k + 1], "bin %d alone" % k)
        smc.assert_same(smc.model_shell_moments(P, V, M, e2[k:k + 2], pts, vel)["moments"], exp[:, k:k + 1], "bin %d alone, points" % k)
    one = smc.model_shell_moments(P, V, M, e2, pts[5:6], vel[5:6])["moments"]     # the row's place in `points` plays no part
    assert smc.same(one, exp[5:6])
    some = smc.model_shell_moments(P, V, M, e2, rows=[3, 64])["moments"]
    assert smc.same(some, own[[3, 64]])
    unit = smc.model_shell_moments(P, V, np.ones(n), e2)["moments"]               # where every mass is 1.0, mass == count
    assert np.array_equal(smc.bits(unit["mass"]), smc.bits(unit["count"].astype(np.float64)))


def test_sources_at_rest_and_awkward_values(bound):
    n = 40
    P, V, M = smc.moment_state(n, np.float64, seed=3, field=10.0)
    e2 = np.array([0.0, 1.0, 50.0, np.inf])
    clean = smc.model_shell_moments(P, V, M, e2)["moments"]
    assert (clean["count"].sum(axis=1) == n - 1).all()
    rest = smc.model_shell_moments(P, np.zeros((n, 2)), M, e2)["moments"]        # every velocity zero: +0.0, sign bit clear
    smc.assert_same(rest, smc.loop_shell_moments(P, np.zeros((n, 2)), M, e2))
    for f in smc.VELOCITY_FIELDS:
        assert not smc.bits(rest[f]).any(), f
    assert np.array_equal(smc.bits(rest["mass"]), smc.bits(clean["mass"])) and np.array_equal(smc.bits(rest["mr2"]), smc.bits(clean["mr2"]))
    minus = smc.model_shell_moments(P, np.full((n, 2), -0.0), M, e2, P[:5] + 0.25)["moments"]   # -0.0 velocities, points at rest
    for f in smc.VELOCITY_FIELDS:
        assert not np.signbit(minus[f]).any() and not minus[f].any(), f
    for f in smc.FIELDS:                                         # no -0.0 anywhere in a generic state either
        assert not (np.signbit(clean[f]) & (clean[f] == 0)).any(), f
    Vn = V.copy()
    Vn[7, 0] = np.nan                                            # a NaN velocity: the velocity sums of its bin NaN, still counted
    got = smc.model_shell_moments(P, Vn, M, e2)["moments"]
    smc.assert_same(got, smc.loop_shell_moments(P, Vn, M, e2))
    assert np.array_equal(got["count"], clean["count"])
    d2_7 = ((P[:, 0] - P[7, 0]) ** 2) + ((P[:, 1] - P[7, 1]) ** 2)
    has7 = (e2[:-1][None, :] <= d2_7[:, None]) & (d2_7[:, None] < e2[1:][None, :])
    has7[7] = False
    row7 = np.zeros_like(has7)
    row7[7] = got["count"][7] > 0                                # body 7's own row: its own NaN velocity is in every u
    for f in ("px", "ke", "rad", "ang", "rad2", "ang2"):
        assert np.array_equal(np.isnan(got[f]), has7 | row7), f
    for f in ("mass", "mr2"):
        assert np.array_equal(smc.bits(got[f]), smc.bits(clean[f])), f
    C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])         # two bodies at one place: d2 = +0
    Vc = np.array([[1.0, 2.0], [0.0, 0.0], [-1.0, 0.5]])
    Mc = np.array([5.0, 7.0, 11.0])
    got = smc.model_shell_moments(C, Vc, Mc, [0.0, 1.0])["moments"]
    assert got["count"].tolist() == [[1], [0], [1]] and got["px"].tolist() == [[-22.0], [0.0], [10.0]]
    assert got["ke"].tolist() == [[11.0 * 6.25], [0.0], [5.0 * 6.25]] and not got["mr2"].any() and not got["rad"].any()
    got = smc.model_shell_moments(C, Vc, Mc, [1e-300, 1.0])["moments"]           # below the first edge: counted nowhere
    assert not got["count"].any() and not got["ke"].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_shared_state_is_sensitive_to_the_order(bound, dtype):
    """What lets test_gpu_shell_moments.py tell a device that adds any of the nine sums in another order from one that keeps
    the contract: with ORDER_SEED, n = 300 and tenth_edges, every field of the model differs from the sum in descending j
    in some (row, bin).  Observed, of 2400 entries: fp32 62 / 368 / 376 / 400 / 414 / 477 / 456 / 425 / 410, fp64 431 / 445 /
    458 / 444 / 424 / 429 / 448 / 441 / 403 in the order of FIELDS."""
    n = 300
    P, V, M = smc.moment_state(n, dtype)
    assert np.abs(V).max() <= 10.0 and V.min() < -9.0 and V.max() > 9.0
    e2 = smc.tenth_edges(smc.tenth_field(n))
    up = smc.model_shell_moments(P, V, M, e2)["moments"]
    down = smc.model_shell_moments(P, V, M, e2, descending=True)["moments"]
    assert np.array_equal(up["count"], down["count"])
    differ = {f: smc.differing(up, down, f) for f in smc.FIELDS}
    print("n %d, %s: of %d (row, bin) entries depend on the order: %s" % (n, np.dtype(dtype).name, up.size, differ))
    for f in smc.FIELDS:
        assert differ[f] > 0, f
        assert not (np.signbit(up[f]) & (up[f] == 0)).any(), f  # no -0.0 anywhere
    assert (up["count"].sum(axis=0) > 0).all() and (up["count"].sum(axis=1) < n - 1).any()    # bins in use, sources outside


def test_shell_kinematics(bound):
    """Unit masses in the flow u = H d + Omega z x d about body 5: the least-squares rates come back."""
    nb = bound
    n, H, W = 300, -0.11, 0.37
    P, _, _ = smc.moment_state(n, np.float64)
    d = P - P[5]
    V = H * d + W * np.stack([-d[:, 1], d[:, 0]], axis=1)        # body 5 itself at rest
    e2 = np.array([0.0, 400.0])
    mom = smc.model_shell_moments(P, V, np.ones(n), e2, rows=[5])
    assert mom["moments"]["count"][0, 0] > 20
    kin = nb.shell_kinematics(mom)
    for name in ("mean_velocity", "sigma2", "mean_r2", "expansion_rate", "rotation_rate", "vr2", "vt2", "anisotropy"):
        assert kin[name].shape[:2] == (1, 1), name
    rel = abs(kin["expansion_rate"][0, 0] / H - 1.0), abs(kin["rotation_rate"][0, 0] / W - 1.0)
    print("relative error of the expansion and rotation rates: %.3g, %.3g" % rel)
    assert rel[0] <= 1e-12 and rel[1] <= 1e-12
    m = mom["moments"][0, 0]
    assert kin["mean_r2"][0, 0] == m["mr2"] / m["mass"] and kin["vr2"][0, 0] == m["rad2"] / m["mr2"]
    assert kin["sigma2"][0, 0] > 0 and np.array_equal(kin["mean_velocity"][0, 0], [m["px"] / m["mass"], m["py"] / m["mass"]])
    assert np.array_equal(nb.shell_kinematics(mom["moments"])["rotation_rate"], kin["rotation_rate"])   # the array itself
    # a pure rotation has no radial motion: d . u is rounding noise, the anisotropy's denominator is no signal - documented as
    # meaningless or NaN.  What can be held: the radial moments are nothing against the tangential ones.
    Vr = W * np.stack([-d[:, 1], d[:, 0]], axis=1)
    rot = nb.shell_kinematics(smc.model_shell_moments(P, Vr, np.ones(n), e2, rows=[5]))
    assert abs(rot["rotation_rate"][0, 0] / W - 1.0) <= 1e-12 and abs(rot["expansion_rate"][0, 0]) <= 1e-12 * W
    assert rot["vr2"][0, 0] <= 1e-24 * rot["vt2"][0, 0]
    # a bin at rest: 0 / 0, NaN; an empty bin: NaN in every entry
    rest = nb.shell_kinematics(smc.model_shell_moments(P, np.zeros((n, 2)), np.ones(n), np.array([0.0, 400.0, 401.0, 1e9]), rows=[5]))
    assert np.isnan(rest["anisotropy"][0, 0]) and rest["sigma2"][0, 0] == 0.0 and rest["expansion_rate"][0, 0] == 0.0
    empty = smc.model_shell_moments(P, V, np.ones(n), np.array([1e9, 2e9]), rows=[5])
    assert empty["moments"]["count"][0, 0] == 0
    for name, a in nb.shell_kinematics(empty).items():
        assert np.isnan(a).all(), name
    with pytest.raises(ValueError):
        nb.shell_kinematics(np.zeros((2, 2)))


def test_library_header_and_bindings(bound):
    nb = bound
    exported = subprocess.check_output(["nm", "-D", "--defined-only", nb.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "nbody.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
    assert re.search(r"^#define NBODY_SHELL_MOMENTS_MAX 8$", header, re.M) and nb.SHELL_MOMENTS_MAX == 8 == smc.SHELL_MOMENTS_MAX
    assert nb.lib.nbody_abi_version() == 2
    assert len(nb.SYMBOLS["nbody_get_shell_moments"][1]) == 8 and len(nb.SYMBOLS["nbody_batch_get_shell_moments"][1]) == 7
    assert nb.SHELL_MOMENT_DTYPE == smc.DTYPE and nb.SHELL_MOMENT_DTYPE.itemsize == 80
    assert nb.SHELL_MOMENT_DTYPE.fields["count"][1] == 72 and nb.SHELL_MOMENT_DTYPE.fields["pad"][1] == 76
    for cls in (nb.Stepper, nb.StepperBatch):
        assert callable(getattr(cls, "shell_moments"))
    assert not hasattr(nb.StepperGroup, "shell_moments")        # the velocities of other ranks' bodies are not on a rank
    assert callable(nb.shell_kinematics)


def test_bad_arguments_are_invalid_before_any_device_call(bound):
    """From a NULL handle: the values are checked before the handle, so each refusal can be seen here, with its reason."""
    nb = bound
    out = np.full(8, 7.0)                                        # stands for the records: never written
    n = ctypes.c_int(7)
    good = np.array([0.0, 1.0, 4.0])
    pts = np.zeros((4, 2))
    Op, Np, Pp = out.ctypes.data, ctypes.byref(n), pts.ctypes.data

    def one(m, e2, bins, out=Op, n_out=Np, points=None, point_vel=None):
        return nb.lib.nbody_get_shell_moments(None, points, point_vel, m, None if e2 is None else e2.ctypes.data, bins, out, n_out)

    def many(m, e2, bins, out=Op, points=None, point_vel=None):
        return nb.lib.nbody_batch_get_shell_moments(None, points, point_vel, m, None if e2 is None else e2.ctypes.data, bins, out)

    for call, name in ((one, b"nbody_get_shell_moments"), (many, b"nbody_batch_get_shell_moments")):
        def refused(reason, *a, **kw):
            assert call(*a, **kw) == INVALID
            msg = nb.lib.nbody_last_error_string()
            assert msg.startswith(name + b": ") and reason in msg, msg

        refused(b"NULL", 4, good, 2)                             # the handle
        refused(b"NULL", 4, None, 2)                             # edges2
        refused(b"NULL", 4, good, 2, out=None)
        for bins in (0, 9, 32, -1):
            refused(b"bins = %d (1 .. 8)" % bins, 4, np.arange(34.0), bins)
        refused(b"point_vel without points", 4, good, 2, point_vel=Pp)
        refused(b"NULL", 4, good, 2, points=Pp, point_vel=Pp)    # with points it is legal: on to the handle
        refused(b"m = -1", -1, good, 2)
        refused(b"edges2[0] = nan", 4, np.array([np.nan, 1.0, 4.0]), 2)
        refused(b"edges2[2]", 4, np.array([0.0, 1.0, np.nan]), 2)
        refused(b"edges2[0] = -1", 4, np.array([-1.0, 1.0, 4.0]), 2)
        refused(b"edges2[2] = 1 is not above edges2[1] = 1", 4, np.array([0.0, 1.0, 1.0]), 2)
        refused(b"edges2[1] = 0.5 is not above edges2[0] = 2", 4, np.array([2.0, 0.5, 4.0]), 2)
        refused(b"more than 2^31 bytes of results", (1 << 31) // (80 * 2) + 1, good, 2)     # m x bins x 80 bytes
        refused(b"more than 2^31 bytes of results", (1 << 31) // (80 * 8) + 1, np.arange(9.0), 8)
        refused(b"NULL", (1 << 31) // (80 * 2), good, 2)         # the largest m that passes: on to the handle
        refused(b"NULL", 4, np.array([0.0, 1.0, np.inf]), 2)     # a +inf top edge is legal
    assert one(4, good, 2, n_out=None) == INVALID and b"nbody_get_shell_moments: NULL" in nb.lib.nbody_last_error_string()
    assert n.value == 7 and (out == 7.0).all()


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("edges", [[1.0], [[0.0, 1.0]], [], [0.0, -1.0, 2.0], np.arange(34.0)])
def test_wrong_edges_raise_before_the_library(bound, edges):
    with pytest.raises(ValueError):
        bound.Stepper.shell_moments(_NoLibrary(), edges)
    with pytest.raises(ValueError):
        bound.StepperBatch.shell_moments(_NoLibrary(), edges)


def test_wrong_point_velocities_raise_before_the_library(bound):
    for cls in (bound.Stepper, bound.StepperBatch):
        with pytest.raises(ValueError):
            cls.shell_moments(_NoLibrary(), [0.0, 1.0], None, np.zeros((3, 2)))          # point_vel without points
        with pytest.raises(ValueError):
            cls.shell_moments(_NoLibrary(), [0.0, 1.0], np.zeros((3, 2)), np.zeros((4, 2)))
