"""The states of ordered_cases.py without a device: the planted coincidences are there and nothing else coincides, and the
numpy models of the field and the tides count what the GPU test expects every kernel to count."""
import numpy as np
import pytest

import field_cases as fc
import ordered_cases as oc
import tide_cases as tc


def setup_module(module):
    fc.require_long_double()


@pytest.mark.parametrize("n", oc.SIZES)
def test_planted_coincidences_and_counts(n):
    P, V, M, R = oc.state(n)
    assert P.shape == V.shape == (n, 2) and M.shape == R.shape == (n,)
    for a in (P, V, M, R):                                      # fp32 values: the same state in either precision
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert (M > 0).all()
    same = (P[:, None, :] == P[None, :, :]).all(axis=2) & ~np.eye(n, dtype=bool)
    pairs = {(int(i), int(j)) for i, j in np.argwhere(same)}
    assert pairs == {p for k, on in oc.planted(n) for p in ((k, on), (on, k))}
    assert len(pairs) == oc.expected_coincident(n) == {5: 2, 130: 2, 321: 4}[n]
    assert oc.flagged_rows(n) == sorted({i for i, _ in pairs})
    # where the flagged rows and their partners lie: tiles of 128 bodies, workgroups of 256 rows
    if n == 321:
        assert [(k // 128, on // 128, k // 256, on // 256) for k, on in oc.planted(n)] == [(2, 0, 1, 0), (2, 2, 1, 1)]
    acc, phi, mag, coin = fc.exact_field(P, M, rows=np.arange(n))
    assert coin == oc.expected_coincident(n)
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, rows=np.arange(n))
    assert coin == oc.expected_coincident(n)
    assert np.isfinite(acc.astype(np.float64)).all() and np.isfinite(tide.astype(np.float64)).all()


@pytest.mark.parametrize("n", oc.SIZES)
def test_points_are_the_bodies_and_free_points(n):
    P, V, M, R = oc.state(n)
    pts, pv = oc.points(P)
    assert pts.shape == pv.shape == (n + oc.FREE_POINTS, 2) and np.array_equal(pts[:n], P)
    free = pts[n:]
    assert not (free[:, None, :] == P[None, :, :]).all(axis=2).any()
    # a point on a body has that body as a source at distance 0, and every body placed on it or under it
    _, _, _, coin = fc.exact_field(P, M, points=pts)
    assert coin == n + oc.expected_coincident(n)
    assert tc.exact_tides(P, V, M, points=pts, point_vel=pv)[2] == coin


def test_the_empty_state():
    P, V, M, R = oc.state(0)
    assert P.shape == (0, 2) and M.shape == (0,)
