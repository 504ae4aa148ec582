"""The field oracle of tests/field_cases.py against closed forms, and what of nbody_get_field / nbody_batch_get_field and
their Python wrappers can be checked without a device: argument handling and the record layout."""
import ctypes

import numpy as np
import pytest

import field_cases as fc
from field_cases import G, LD, U

INVALID = -1


def setup_module(module):
    fc.require_long_double()


@pytest.mark.parametrize("e", [-40, -3, 0, 1, 7, 60])
def test_two_bodies_at_power_of_two_separations(e):
    """a = G m / d^2 along the axis towards the other body, phi = -G m / d: d a power of two, so the closed form is
    exact but for the one product with G."""
    d, m0, m1 = 2.0 ** e, 3.0, 5.0
    P = np.array([[0.0, 2.0], [d, 2.0]])                      # exact in double for every d
    M = np.array([m0, m1])
    acc, phi, mag, coin = fc.exact_field(P, M, rows=[0, 1])
    assert coin == 0
    want_a0, want_a1 = LD(G) * LD(m1) / LD(d) / LD(d), -LD(G) * LD(m0) / LD(d) / LD(d)
    for got, want in ((acc[0, 0], want_a0), (acc[1, 0], want_a1), (phi[0], -LD(G) * LD(m1) / LD(d)),
                      (phi[1], -LD(G) * LD(m0) / LD(d))):
        assert abs(got - want) <= 4 * LD(2.0) ** -63 * abs(want), (e, got, want)
    assert acc[0, 1] == 0 and acc[1, 1] == 0
    assert mag[0, 0] == abs(acc[0, 0]) and mag[1, 0] == abs(acc[1, 0])
    # the same bodies seen from an explicit point on the axis, at distance d from body 0 and 2 d from body 1
    acc, phi, mag, coin = fc.exact_field(P, M, points=[[-d, 2.0]])
    want = LD(G) * (LD(m0) / LD(d) / LD(d) + LD(m1) / LD(2 * d) / LD(2 * d))
    assert coin == 0 and abs(acc[0, 0] - want) <= 8 * LD(2.0) ** -63 * want
    assert abs(phi[0] + LD(G) * (LD(m0) / LD(d) + LD(m1) / LD(2 * d))) <= 8 * LD(2.0) ** -63 * abs(phi[0])


@pytest.mark.parametrize("n", [3, 4, 7, 128, 129])
def test_centre_of_a_regular_polygon(n):
    """Equal masses on a regular polygon: the acceleration at the centre vanishes within the bound (the vertices are
    rounded to double), phi = -G n m / R."""
    R, m = 1024.0, 7.0
    k = np.arange(n)
    P = np.stack([R * np.cos(2 * np.pi * k / n), R * np.sin(2 * np.pi * k / n)], axis=1)
    M = np.full(n, m)
    acc, phi, mag, coin = fc.exact_field(P, M, points=[[0.0, 0.0]])
    assert coin == 0
    # vertices within 2 u of the circle: each term moves by at most 3 * 2 u of its size
    assert (np.abs(acc[0]) <= 8 * U * mag[0] + LD(G) * n * m / R / R * 8 * U).all(), acc
    want = -LD(G) * n * m / R
    assert abs(phi[0] - want) <= 4 * U * abs(want)
    fc.check_field(np.zeros((1, 2)), np.array([float(want)]), acc, phi,
                   mag + LD(G) * n * m / R / R, n, "polygon %d" % n)   # 0 is inside the bound once the rounding of the vertices counts


def test_probe_on_a_body_is_skipped_and_counted():
    P = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0], [-6.0, 8.0]])
    M = np.array([2.0, 5.0, 11.0, 13.0])
    acc, phi, mag, coin = fc.exact_field(P, M, points=[[3.0, 4.0], [0.0, 0.0], [1.0, 1.0]])
    assert coin == 3                                            # two sources under the first point, one under the second
    want = -LD(G) * (LD(2.0) / 5 + LD(13.0) / LD(np.sqrt(LD(81.0) + 16)))
    assert abs(phi[0] - want) <= 4 * LD(2.0) ** -63 * abs(want)
    # own positions: the self term is not counted, the coincident partner is
    acc, phi, mag, coin = fc.exact_field(P, M, rows=[0, 1, 2, 3])
    assert coin == 2
    assert abs(phi[1] + LD(G) * (LD(2.0) / 5 + LD(13.0) / LD(np.sqrt(LD(81.0) + 16)))) <= 1e-18 * abs(phi[1])
    one = fc.exact_field(P[:1], M[:1], rows=[0])
    assert one[3] == 0 and one[1][0] == 0 and (one[0] == 0).all()


def test_bound_constants():
    assert fc.ACC_C == 14 and fc.PHI_C == 4 and fc.U == 2.0 ** -53


def test_field_record_layout(nb):
    assert ctypes.sizeof(nb.Field) == 24
    assert nb.FIELD_DTYPE.itemsize == 24 and nb.FIELD_DTYPE["acc"].shape == (2,)
    assert nb.FIELD_DTYPE.fields["acc"][1] == 0 and nb.FIELD_DTYPE.fields["phi"][1] == 16
    assert [f[0] for f in nb.Field._fields_] == ["ax", "ay", "phi"]


def test_null_handles_are_invalid(nb):
    out = (nb.Field * 4)()
    n, coin = ctypes.c_int(7), ctypes.c_int64(7)
    assert nb.lib.nbody_get_field(None, None, 4, out, ctypes.byref(n), ctypes.byref(coin)) == INVALID
    assert b"nbody_get_field" in nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_batch_get_field(None, None, 4, out, ctypes.byref(coin)) == INVALID
    assert b"nbody_batch_get_field" in nb.lib.nbody_last_error_string()
    assert n.value == 7 and coin.value == 7


class _NoLibrary:
    """Stands where a context handle would: the wrappers must raise before they reach the library."""
    capacity, systems, _ctx, _b = 8, 2, None, None


@pytest.mark.parametrize("points", [[1.0, 2.0], [[1.0, 2.0, 3.0]], np.zeros((2, 2, 2)), 5.0, np.zeros((2, 0))])
def test_wrong_points_shape_raises_before_the_library(nb, points):
    with pytest.raises(ValueError):
        nb.Stepper.field(_NoLibrary(), points)
    with pytest.raises(ValueError):
        nb.StepperBatch.field(_NoLibrary(), points)
