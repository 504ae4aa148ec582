"""The oracle of tests/tide_cases.py against closed forms and against differences of the field oracle, the two numpy
helpers, and what of nbody_get_tides / nbody_batch_get_tides and their Python wrappers can be checked without a device:
argument handling and the record layout."""
import ctypes

import numpy as np
import pytest

import field_cases as fc
import tide_cases as tc
from tide_cases import G, LD, U

INVALID = -1
EPS = LD(2.0) ** -63


def setup_module(module):
    tc.require_long_double()


@pytest.mark.parametrize("e", [-40, -3, 0, 1, 7, 60])
def test_two_bodies_at_power_of_two_separations(e):
    """The body at the origin and its partner on the x-axis: txx = 2 G m / d^3, tyy = -G m / d^3, txy = 0; with dv = (v, 0)
    adot = (-2 G m v / d^3, 0), with dv = (0, v) adot = (0, G m v / d^3)."""
    d, m0, m1, v = 2.0 ** e, 3.0, 5.0, 0.75
    P = np.array([[0.0, 0.0], [d, 0.0]])
    M = np.array([m0, m1])
    q = LD(G) * LD(m1) / LD(d) / LD(d) / LD(d)
    for V, want_j in (([[0, 0], [v, 0]], (-2 * q * v, 0)), ([[0, 0], [0, v]], (0, q * v)),
                      ([[1.5, 0], [1.5 + v, 0]], (-2 * q * v, 0)), ([[0, -v], [0, 0]], (0, q * v))):
        tide, jerk, coin, bt, bj = tc.exact_tides(P, np.array(V, dtype=np.float64), M, rows=[0, 1])
        assert coin == 0
        for got, want in ((tide[0, 0], 2 * q), (tide[0, 2], -q), (jerk[0, 0], want_j[0]), (jerk[0, 1], want_j[1])):
            assert abs(got - want) <= 8 * EPS * abs(want), (e, got, want)
        assert tide[0, 1] == 0
        assert abs(bt[0, 0] - 4 * q) <= 8 * EPS * q and abs(bt[0, 2] - q) <= 8 * EPS * q and bt[0, 1] == 0
        # seen from the partner the tensor of the other mass, the jerk reversed
        q0 = LD(G) * LD(m0) / LD(d) / LD(d) / LD(d)
        assert abs(tide[1, 0] - 2 * q0) <= 8 * EPS * q0 and abs(tide[1, 2] + q0) <= 8 * EPS * q0
        assert abs(jerk[1, 0] + want_j[0] * m0 / m1) <= 8 * EPS * abs(want_j[0]) and \
            abs(jerk[1, 1] + want_j[1] * m0 / m1) <= 8 * EPS * abs(want_j[1])
    # an explicit point on the axis, at distance d from body 0 and 2 d from body 1, at rest among sources at rest
    tide, jerk, coin, bt, bj = tc.exact_tides(P, None, M, points=[[-d, 0.0]])
    want = LD(G) * (LD(m0) + LD(m1) / 8) / LD(d) / LD(d) / LD(d)
    assert coin == 0 and abs(tide[0, 0] - 2 * want) <= 8 * EPS * want and abs(tide[0, 2] + want) <= 8 * EPS * want
    assert (jerk == 0).all() and (bj == 0).all()


@pytest.mark.parametrize("n", [3, 4, 7, 128, 129])
def test_centre_of_a_regular_polygon(n):
    """Equal masses on a regular polygon: at the centre txx = tyy = G n m / (2 R^3) and txy = 0, within the bound once the
    rounding of the vertices to double counts."""
    R, m = 1024.0, 7.0
    k = np.arange(n)
    P = np.stack([R * np.cos(2 * np.pi * k / n), R * np.sin(2 * np.pi * k / n)], axis=1)
    tide, jerk, coin, bt, bj = tc.exact_tides(P, None, np.full(n, m), points=[[0.0, 0.0]])
    want = LD(G) * n * m / (2 * LD(R) ** 3)
    assert coin == 0
    # a vertex within 2 u R of its place moves each of its terms by at most 5 * 2 u of G m / R^3 (r^-5 d_a d_b: 5 + 2 powers)
    slack = 16 * U * LD(G) * n * m / LD(R) ** 3
    assert abs(tide[0, 0] - want) <= slack and abs(tide[0, 2] - want) <= slack and abs(tide[0, 1]) <= slack
    tc.check_tides(np.array([[float(want), 0.0, float(want)]]), None, tide, jerk, bt + slack / U, bj, n, "polygon %d" % n)
    assert abs(bt[0, 0] + bt[0, 2] - 5 * LD(G) * n * m / LD(R) ** 3) <= slack      # sum (3 u_x^2 + 1 + 3 u_y^2 + 1) = 5 n


def random_state(n, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-50, 50, size=(n, 2))
    V = rng.uniform(-3, 3, size=(n, 2))
    M = rng.uniform(1e9, 5e10, size=n)
    return P, V, M


def test_trace_identity():
    """txx + tyy = G sum m_j / r_j^3 > 0: the 3-D force law in a plane is not traceless."""
    P, V, M = random_state(60, 1)
    pts = np.random.default_rng(2).uniform(-60, 60, size=(20, 2))
    tide, _, coin, bt, _ = tc.exact_tides(P, V, M, points=pts)
    d = np.hypot(P[None, :, 0].astype(LD) - pts[:, None, 0].astype(LD), P[None, :, 1].astype(LD) - pts[:, None, 1].astype(LD))
    want = (LD(G) * M[None, :].astype(LD) / d / d / d).sum(axis=1)
    assert coin == 0 and (want > 0).all()
    assert (np.abs(tide[:, 0] + tide[:, 2] - want) <= 64 * 60 * EPS * want).all()
    assert (np.abs(bt[:, 0] + bt[:, 2] - 5 * want) <= 64 * 60 * EPS * want).all()


def test_jerk_is_T_v_for_sources_at_rest():
    """With every source at rest dv = -v and adot = T v."""
    P, _, M = random_state(40, 3)
    rng = np.random.default_rng(4)
    pts, pv = rng.uniform(-60, 60, size=(15, 2)), rng.uniform(-2, 2, size=(15, 2))
    tide, jerk, _, bt, bj = tc.exact_tides(P, None, M, points=pts, point_vel=pv)
    vx, vy = pv[:, 0].astype(LD), pv[:, 1].astype(LD)
    want = np.stack([tide[:, 0] * vx + tide[:, 1] * vy, tide[:, 1] * vx + tide[:, 2] * vy], axis=1)
    assert (np.abs(jerk - want) <= 64 * 40 * EPS * bj).all(), (jerk, want)
    # the same through own rows: one moving body among bodies at rest
    V = np.zeros((40, 2))
    V[7] = [1.25, -0.5]
    tide, jerk, _, _, bj = tc.exact_tides(P, V, M, rows=[7])
    want = np.array([tide[0, 0] * LD(1.25) - tide[0, 1] * LD(0.5), tide[0, 1] * LD(1.25) - tide[0, 2] * LD(0.5)])
    assert (np.abs(jerk[0] - want) <= 64 * 40 * EPS * bj[0]).all()


def test_against_central_differences_of_the_field():
    """T_ab = d a_a / d x_b in space, adot = d a / d t along straight paths, both by central differences of
    field_cases.exact_field in long double: step h, truncation O(h^2), rounding O(eps / h)."""
    P, V, M = random_state(30, 5)
    rng = np.random.default_rng(6)
    pts, pv = rng.uniform(-60, 60, size=(10, 2)), rng.uniform(-2, 2, size=(10, 2))
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
    assert coin == 0
    h = 2.0 ** -14                                              # exactly representable shifts of O(50) coordinates
    ap = [fc.exact_field(P, M, points=pts + s * np.array(e))[0] for e in ([h, 0], [0, h]) for s in (1, -1)]
    dadx, dady = (ap[0] - ap[1]) / (2 * LD(h)), (ap[2] - ap[3]) / (2 * LD(h))
    # nearest source of any point is more than 0.1 away here: h^2 / r^2 < 2^-20
    rmin = np.hypot(P[None, :, 0] - pts[:, None, 0], P[None, :, 1] - pts[:, None, 1]).min()
    assert rmin > 0.1
    tol = 1e-5 * bt
    assert (np.abs(dadx[:, 0] - tide[:, 0]) <= tol[:, 0]).all() and (np.abs(dady[:, 1] - tide[:, 2]) <= tol[:, 2]).all()
    assert (np.abs(dadx[:, 1] - tide[:, 1]) <= tol[:, 1] + 1e-5 * bt[:, 0]).all()
    assert (np.abs(dady[:, 0] - tide[:, 1]) <= tol[:, 1] + 1e-5 * bt[:, 0]).all()          # symmetric
    t = 2.0 ** -14
    af = fc.exact_field(P + t * V, M, points=pts + t * pv)[0]
    ab = fc.exact_field(P - t * V, M, points=pts - t * pv)[0]
    dadt = (af - ab) / (2 * LD(t))
    assert (np.abs(dadt - jerk) <= 1e-5 * bj).all(), (dadt, jerk)
    # own rows the same way
    tide, jerk, _, bt, bj = tc.exact_tides(P, V, M, rows=np.arange(30))
    af, ab = fc.exact_field(P + t * V, M, rows=np.arange(30))[0], fc.exact_field(P - t * V, M, rows=np.arange(30))[0]
    assert (np.abs((af - ab) / (2 * LD(t)) - jerk) <= 1e-5 * bj).all()


def test_probe_on_a_body_is_skipped_and_counted():
    P = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0], [-6.0, 8.0]])
    V = np.array([[1.0, 0.0], [0.0, 2.0], [5.0, 5.0], [-1.0, 0.5]])
    M = np.array([2.0, 5.0, 11.0, 13.0])
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=[[3.0, 4.0], [0.0, 0.0], [1.0, 1.0]])
    assert coin == 3                                            # two sources under the first point, one under the second
    rest = tc.exact_tides(P[[0, 3]], V[[0, 3]], M[[0, 3]], points=[[3.0, 4.0]])
    assert np.array_equal(tide[0], rest[0][0]) and np.array_equal(jerk[0], rest[1][0]) and rest[2] == 0
    # own positions: the self term is not counted, the coincident partner is
    tide, jerk, coin, _, _ = tc.exact_tides(P, V, M, rows=[0, 1, 2, 3])
    assert coin == 2 == fc.exact_field(P, M, rows=[0, 1, 2, 3])[3]
    rest = tc.exact_tides(P[[1, 0, 3]], V[[1, 0, 3]], M[[1, 0, 3]], rows=[0])
    assert np.array_equal(tide[1], rest[0][0]) and np.array_equal(jerk[1], rest[1][0])


def test_a_one_body_system_gives_zeros():
    one = tc.exact_tides(np.array([[10.0, 20.0]]), np.array([[1.0, 2.0]]), np.array([4.0]), rows=[0])
    assert one[2] == 0 and all((a == 0).all() for a in (one[0], one[1], one[3], one[4]))


@pytest.mark.parametrize("e,me,ve", tc.FAR_CASES)
def test_far_cases_have_normal_terms(e, me, ve):
    """The states of test_gpu_tides.py's far-range test: every magnitude sum, hence every exact term up to the factors
    within [1/8, 16], is a normal double with room to spare."""
    P, V, M, pts, pv = tc.far_state(e, me, ve)
    for kw in (dict(rows=[0, 1, 2]), dict(points=pts, point_vel=pv), dict(points=pts)):
        tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, **kw)
        assert coin == 0
        for b in (bt[:, 0], bt[:, 2], bj):
            assert float(b.min()) > 2.0 ** -1000 and float(b.max()) < 2.0 ** 1000, (e, kw.keys(), b)
        assert float(np.abs(tide[:, [0, 2]]).min()) > 2.0 ** -1000


def test_bound_constants():
    """The derived values of the module docstring's table."""
    assert (tc.TIDE_K, tc.TIDE_C, tc.JERK_K, tc.JERK_C) == (1, 26, 2, 28) and tc.U == 2.0 ** -53
    w = 3 + 3 + 1 + 3 + 1 + 1                                   # y, y2, y3, w
    ux, w3 = 1 + 3 + 1, w + 1
    term = (w3 + ux + 1) + ux
    assert w == 12 and term == 24 and tc.TIDE_C == max(term, w) + 2
    ru = (ux + 1 + 1) + 1
    second = (w3 + ru + 1) + ux
    assert second == 27 and w + 1 == 13 and tc.JERK_C == max(second, w + 1) + 1


def test_tide_eigen_and_tidal_radius_of_a_single_source(nb):
    """A mass M at distance R: lambda = (2 G M / R^3, -G M / R^3) whatever the direction, r_t = R (m / 2M)^(1/3)."""
    Ms, R, m = 4.0e12, 37.5, 2.5e3
    for ang in (0.0, 0.3, np.pi / 2, 2.0, -2.5):
        pt = [[R * np.cos(ang), R * np.sin(ang)]]
        tide = tc.exact_tides(np.zeros((1, 2)), None, np.array([Ms]), points=pt)[0].astype(np.float64)
        hi, lo = nb.tide_eigen(tide)
        assert hi.shape == (1,) and abs(hi[0] - 2 * G * Ms / R ** 3) <= 1e-14 * hi[0]
        assert abs(lo[0] + G * Ms / R ** 3) <= 1e-14 * hi[0]
        rt = nb.tidal_radius(tide, m, G)
        assert abs(rt[0] - R * (m / (2 * Ms)) ** (1 / 3)) <= 1e-14 * rt[0]
    # compressive along every axis: no tidal radius
    assert nb.tidal_radius([[-1.0, 0.0, -2.0], [0.0, 0.0, 0.0]], 1.0, G).tolist() == [np.inf, np.inf]
    hi, lo = nb.tide_eigen(np.zeros((2, 5, 3)))
    assert hi.shape == lo.shape == (2, 5)
    with pytest.raises(ValueError):
        nb.tide_eigen(np.zeros((4, 2)))


def test_tide_record_layout(nb):
    assert ctypes.sizeof(nb.Tide) == 24
    assert [f[0] for f in nb.Tide._fields_] == ["txx", "txy", "tyy"]
    assert nb.TIDE_DTYPE.itemsize == 24 and nb.TIDE_DTYPE.names == ("txx", "txy", "tyy")
    assert [nb.TIDE_DTYPE.fields[k][1] for k in nb.TIDE_DTYPE.names] == [0, 8, 16]


def last_error(nb):
    return nb.lib.nbody_last_error_string()


def test_null_handles_and_invalid_arguments(nb):
    """Every NBODY_ERR_INVALID case is found before any device call - and before the handle is looked at, so none of them
    needs a context here; each message names the entry point and what is wrong."""
    tide, jerk, pts = (nb.Tide * 4)(), np.zeros((4, 2)), np.zeros((4, 2))
    vel = np.zeros((4, 2))
    n, coin = ctypes.c_int(7), ctypes.c_int64(7)
    rn, rc = ctypes.byref(n), ctypes.byref(coin)
    one, many = nb.lib.nbody_get_tides, nb.lib.nbody_batch_get_tides
    handle = ctypes.create_string_buffer(8)                     # never read: every call below fails its checks first
    H = ctypes.addressof(handle)
    big = (1 << 31) // 24 + 1
    cases = [                                                   # (points, point_vel, m, tide, jerk), what the message says
        ((pts.ctypes.data, None, -1, tide, jerk.ctypes.data), b"m = -1"),
        ((None, vel.ctypes.data, 4, tide, jerk.ctypes.data), b"point_vel without points"),
        ((pts.ctypes.data, vel.ctypes.data, 4, tide, None), b"point_vel without jerk"),
        ((pts.ctypes.data, None, big, tide, None), b"2^31"),
        ((pts.ctypes.data, None, 4, None, None), b"NULL argument"),
    ]
    for args, text in cases:
        assert one(H, *args, rn, rc) == INVALID
        assert b"nbody_get_tides" in last_error(nb) and text in last_error(nb), (text, last_error(nb))
    assert one(None, pts.ctypes.data, None, 4, tide, None, rn, rc) == INVALID and b"nbody_get_tides: NULL" in last_error(nb)
    assert one(H, pts.ctypes.data, None, 4, tide, None, None, rc) == INVALID and b"NULL argument" in last_error(nb)
    assert one(H, pts.ctypes.data, None, 4, tide, None, rn, None) == INVALID and b"NULL argument" in last_error(nb)
    # a batch: the values are checked before the handle is read, the handle before anything is read through it
    for args, text in cases[:3]:
        assert many(None, *args, rc) == INVALID
        assert b"nbody_batch_get_tides" in last_error(nb) and text in last_error(nb), (text, last_error(nb))
    assert many(None, pts.ctypes.data, None, big, tide, None, rc) == INVALID and b"2^31" in last_error(nb)
    assert many(None, pts.ctypes.data, None, 4, tide, None, rc) == INVALID and b"nbody_batch_get_tides: NULL" in last_error(nb)
    assert n.value == 7 and coin.value == 7


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("points", [[1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros((2, 2, 2)), 5.0, np.zeros((2, 0))])
def test_wrong_points_shape_raises_before_the_library(nb, points):
    with pytest.raises(ValueError):
        nb.Stepper.tides(_NoLibrary(), points)
    with pytest.raises(ValueError):
        nb.StepperBatch.tides(_NoLibrary(), points, jerk=True)


@pytest.mark.parametrize("points,point_vel,jerk", [
    (np.zeros((3, 2)), np.zeros((2, 2)), True), (np.zeros((3, 2)), np.zeros(3), True), (np.zeros((3, 2)), np.zeros((3, 3)), True),
    (np.zeros((3, 2)), 1.0, True), (None, np.zeros((3, 2)), True), (np.zeros((3, 2)), np.zeros((3, 2)), False)])
def test_wrong_point_vel_raises_before_the_library(nb, points, point_vel, jerk):
    with pytest.raises(ValueError):
        nb.Stepper.tides(_NoLibrary(), points, point_vel, jerk)
    with pytest.raises(ValueError):
        nb.StepperBatch.tides(_NoLibrary(), points, point_vel, jerk)
