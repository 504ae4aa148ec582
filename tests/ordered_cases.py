"""The states of tests/test_gpu_ordered_family.py: what the kernels that sum over j = 0 .. n-1 in ascending order
(diag_potential, batch_diag_potential, track_potential, field_at, tracers_advance, tides_at, group_potential; DESIGN.md 4.4,
4.8b) are all asked about, so that one state goes through the ordered walk and the exact walk of every one of them.

Sizes (128-body tiles, 256-row workgroups): 5 - a remainder after one group of four; 130 - two tiles with a ragged second;
321 - three tiles over two workgroups, rows 256 .. 320 with self tile 2.  Body n-1 lies exactly on body 0, and for n = 321
body 300 on body 257: a flagged row in a full tile and in the ragged tile, its partner in the same tile, in another tile
and in another workgroup.  Every value is an fp32 number, so that an fp32 and an fp64 context hold the same state."""
import numpy as np

SIZES = (5, 130, 321)
FIELD = 1000.0                          # the square the bodies lie in
FREE_POINTS = 3                         # explicit points that are on no body


def planted(n):
    """(body, the lower body it is placed on), ..."""
    return ((n - 1, 0),) + (((300, 257),) if n == 321 else ())


def expected_coincident(n):
    """Ordered pairs (i, j), j != i, at distance 0: each planted pair counts from both sides."""
    return 2 * len(planted(n))


def flagged_rows(n):
    return sorted(k for pair in planted(n) for k in pair)


def state(n, seed=11):
    """-> P (n, 2), V (n, 2), M (n,), R (n,) as float64 arrays of fp32 values; n = 0: empty arrays."""
    rng = np.random.default_rng(seed + n)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    P = f32(rng.uniform(0.0, FIELD, size=(n, 2)))
    V = f32(rng.uniform(-3.0, 3.0, size=(n, 2)))
    M = f32(rng.uniform(1.0e3, 1.0e6, size=n))
    R = f32(np.full(n, 0.25))
    if n:
        assert len(np.unique(P, axis=0)) == n                   # no coincidence but the planted ones
        for k, on in planted(n):
            P[k] = P[on]
    return P, V, M, R


def points(P, seed=12):
    """The bodies' positions followed by FREE_POINTS points on no body (the last far outside the field), and velocities
    for all of them."""
    rng = np.random.default_rng(seed + len(P))
    free = rng.uniform(0.0, FIELD, size=(FREE_POINTS, 2))
    free[-1] = [-7.5 * FIELD, 11.25 * FIELD]
    pts = np.concatenate([np.asarray(P, dtype=np.float64).reshape(-1, 2), free])
    return pts, rng.uniform(-4.0, 4.0, size=pts.shape)
