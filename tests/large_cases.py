"""The states of the large-N tests of the row queries (pair counts, groups, encounters, k nearest, neighbours, field, tracers;
DESIGN.md 4.8 to 4.14) and their references, computed once per process and never written to.

The size.  N = 100 003, chosen because it is the smallest convenient size at which
  * a row or source index passes 2^16 (N > 65 536);
  * the pair total passes 2^32: N > 92 683 (92 683 * 92 682 / 2 = 4 295 022 903), PAIRS = 5 000 250 003 > 2^32;
  * the walk stages hundreds of source tiles: 782 tiles of 128, the last one holding 35 bodies (781 * 128 = 99 968);
  * the grid has more workgroups than the chip has CUs: 391 workgroups of 256 rows, every one flushing into the one histogram,
    the one append counter and the one log;
  * the last workgroup is ragged: 163 rows (390 * 256 = 99 840) = two full waves, one wave of 35 rows and one wave with no row
    that only loads tiles.
An n x n model is out of reach here; the references are the window forms of pair_cases, group_cases and encounter_cases and the
rows= argument of model_knn and model_neighbors, which test_pair_cases_cpu.py, test_group_cases_cpu.py and
test_encounter_cases_cpu.py prove equal to the full models, and which test_large_cases_cpu.py proves equal again on a
1500-body state of this module's own generator.

State A (uploaded).  make_state(): positions uniform over a square field of mean spacing 63.2 (20 000 wide at N), radii uniform
in [0, 1.5), velocities uniform in +-25 - bounded, because window_encounters' reach is 2 max R + 2 max |VX| h -, masses 1, the
index order unrelated to the geometry.  On top of it 3 * per_kind planted pairs at randomly chosen indices (so the two bodies
of a pair sit in different workgroups), radii in [0.3, 0.75), s = R_a + R_b, e the unit vector from a to b, H = 0.2:
    kind 0 "now"     d = u s, u in (0.2, 0.8): overlapping; every third one has a third body overlapping b (a chain of three)
    kind 1 "end"     d = s (1 + delta), delta in (0.2, 1.0), head-on with closing speed (d - f s) / H, f in (0.2, 0.8): apart
                     now, f s apart at H
    kind 2 "missed"  d = s (1 + delta), head-on with closing speed (d + g s) / H, g in (1.3, 2.0): through each other and g s
                     apart again at H - neither flag
the pair's common drift uniform in +-5, so no velocity component passes 20.  Every value is rounded to fp32 and widened back:
the fp32 and the fp64 context hold the same doubles and share one reference.  The margins (0.2 s >= 0.12) are far above the
fp32 spacing of a coordinate (2^-9 at 16 384).

The "touching" groups (link, radius_scale) = (0, 1) are the planted pairs and chains and the few chance overlaps: small and
many.  The centre link CENTRE_LINK = 1.5 mean spacings is above the percolation length (about 1.2): one component of most
bodies, spread over every workgroup, next to more than 100 others.

References of state A (reference(name)), seconds on a CPU-only machine (numpy, one thread), printed by
test_large_cases_cpu.py::test_references_within_budget - none may pass BUDGET_S = 10:
    pairs16 0.5   pairs256 0.6   pairs_below 0.4   pairs_points 0.6   touching 0.0   centres 0.7
    enc_0 0.1   enc_dt 0.3   enc_h 0.7   neighbors 1.3   knn32 5.5   neighbors_points 0.8   knn32_points 4.1
model_knn sorts all n distances of a row whatever k is: the k = 32 reference is taken once on 394 of the 594 sampled rows and
its first k columns are the model for k = 1 and 8 (knn_prefix).
"""
import functools
import time

import numpy as np

import encounter_cases as ec
import group_cases as gc
import knn_cases as kc
import neighbor_cases as nc
import pair_cases as pc

N = 100003
TILE, WG, WAVE = 128, 256, 64
PAIRS = N * (N - 1) // 2
SPACING = 20000.0 / np.sqrt(N)                                  # the mean spacing of every state of make_state
VMAX = 25.0
PER_KIND = 700
H = 0.2                                                         # the test's horizon
DT = 0.0625                                                     # the time step of the contexts of state A: exact in fp32
CENTRE_LINK = 1.5 * SPACING
BUDGET_S = 10.0
SEED = 100003

# squared edges
E2_16 = np.concatenate([[0.0], np.geomspace(1.0, 100.0 ** 2, 16)])     # first edge 0: below == 0
E2_256 = np.geomspace(0.01, 60.0 ** 2, 257)                     # every trip count of the edge search
E2_BELOW = np.geomspace(4.0, 100.0 ** 2, 9)                     # the planted pairs lie under the first edge
E2_ALL = np.array([0.0, np.inf])

# the small system under many rows
SMALL_N, MANY, FEW = 300, 70001, 300
SMALL_FIELD = 100.0


def field_of(n):
    return SPACING * np.sqrt(n)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_state(n=N, per_kind=PER_KIND, seed=SEED):
    """-> P (n, 2), V (n, 2), M (n,), R (n,) float64, every value fp32-representable; see the module docstring."""
    rng = np.random.default_rng(seed)
    field = field_of(n)
    P = rng.uniform(0.0, field, size=(n, 2))
    V = rng.uniform(-VMAX, VMAX, size=(n, 2))
    R = rng.uniform(0.0, 1.5, size=n)
    K = 3 * per_kind
    perm = rng.permutation(n)
    a, b, c = perm[:K], perm[K:2 * K], perm[2 * K:2 * K + per_kind // 3]
    kind = np.repeat(np.arange(3), per_kind)
    R[a], R[b], R[c] = rng.uniform(0.3, 0.75, size=K), rng.uniform(0.3, 0.75, size=K), rng.uniform(0.3, 0.75, size=len(c))
    P[a] = rng.uniform(0.05 * field, 0.95 * field, size=(K, 2))   # room for the partner inside the field
    s = R[a] + R[b]
    ang = rng.uniform(0.0, 2.0 * np.pi, size=K)
    e = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    d = np.where(kind == 0, rng.uniform(0.2, 0.8, size=K), 1.0 + rng.uniform(0.2, 1.0, size=K)) * s
    P[b] = P[a] + d[:, None] * e
    f = rng.uniform(0.2, 0.8, size=K)
    g = rng.uniform(1.3, 2.0, size=K)
    w = np.where(kind == 1, d - f * s, d + g * s) / H             # the closing speed of kinds 1 and 2
    drift = rng.uniform(-5.0, 5.0, size=(K, 2))
    moving = kind > 0
    V[a[moving]] = drift[moving] + 0.5 * w[moving, None] * e[moving]
    V[b[moving]] = drift[moving] - 0.5 * w[moving, None] * e[moving]
    bc = b[:len(c)]                                               # the first kind-0 pairs get a third body beyond b
    ang = rng.uniform(0.0, 2.0 * np.pi, size=len(c))
    P[c] = P[bc] + (rng.uniform(0.2, 0.8, size=len(c)) * (R[bc] + R[c]))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return _f32(P), _f32(V), np.ones(n), _f32(R)


def sample_rows(n=N, random=300, seed=7):
    """The rows of the row-wise comparisons: the first 130, the last 130, 65 530 .. 65 545, the rows around three workgroup
    edges and a seeded random few hundred -> (rows, knn_rows): sorted, unique; knn_rows leaves out two thirds of the random
    ones (the model sorts all n distances of every row)."""
    rng = np.random.default_rng(seed)
    chosen = rng.choice(n, size=random, replace=False)
    fixed = [np.arange(min(130, n)), np.arange(max(n - 130, 0), n), np.arange(65530, 65546)]
    fixed += [np.arange(w * WG - 3, w * WG + 3) for w in (1, 255, n // WG)]
    fixed = np.concatenate(fixed)
    fixed = fixed[(fixed >= 0) & (fixed < n)]
    return np.unique(np.concatenate([fixed, chosen])), np.unique(np.concatenate([fixed, chosen[:random // 3]]))


def points_over(P, m, field, seed):
    """m probe points over a state: neighbor_cases.probe_points (the first ones ON bodies, two far outside, one twice)."""
    return nc.probe_points(P, m, seed=seed, field=field)


def small_system(seed=300):
    """(P, V, M, R) of the 300 bodies under the many rows, fp32-representable."""
    rng = np.random.default_rng(seed)
    P, R = nc.random_state(SMALL_N, np.float32, seed=seed, field=SMALL_FIELD)
    M = _f32(rng.uniform(1e3, 1e6, size=SMALL_N))
    return P, np.zeros((SMALL_N, 2)), M, R


# ---------------------------------------------------------------------------------------------------------------------
# the cached references
# ---------------------------------------------------------------------------------------------------------------------
TIMES = {}                                                      # name -> seconds its reference took


def freeze(x):
    """Marks every array inside x read-only; -> x."""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            freeze(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            freeze(v)
    return x


@functools.lru_cache(maxsize=None)
def state_a():
    return freeze(make_state())


@functools.lru_cache(maxsize=None)
def rows_a():
    return freeze(sample_rows())


@functools.lru_cache(maxsize=None)
def points_a():
    return freeze(points_over(state_a()[0], FEW, field_of(N), seed=11))


def _knn32(P, **kw):
    return kc.model_knn(P, 32, chunk=8, **kw)


def builders(P, V, R, rows, knn_rows, pts):
    """name -> the call that computes that reference of the state (P, V, R): the one table behind reference() for state A,
    the stepped state and the 1500-body state of the CPU test."""
    return {
        "pairs16": lambda: pc.window_pair_counts(P, E2_16),
        "pairs256": lambda: pc.window_pair_counts(P, E2_256),
        "pairs_below": lambda: pc.window_pair_counts(P, E2_BELOW),
        "pairs_points": lambda: pc.model_pair_counts(P, E2_BELOW, pts),
        "touching": lambda: gc.window_groups(P, R, 0.0, 1.0),
        "centres": lambda: gc.window_groups(P, R, CENTRE_LINK, 0.0),
        "enc_0": lambda: ec.window_encounters(P, V, R, 0.0),
        "enc_dt": lambda: ec.window_encounters(P, V, R, DT),
        "enc_h": lambda: ec.window_encounters(P, V, R, H),
        "neighbors": lambda: nc.model_neighbors(P, R, rows=rows),
        "knn32": lambda: _knn32(P, rows=knn_rows),
        "neighbors_points": lambda: nc.model_neighbors(P, R, points=pts),
        "knn32_points": lambda: _knn32(P, points=pts),
    }


NAMES = tuple(builders(*[None] * 6))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference `name` of state A: computed on the first call, timed into TIMES, read-only."""
    P, V, _, R = state_a()
    rows, knn_rows = rows_a()
    t0 = time.perf_counter()
    out = builders(P, V, R, rows, knn_rows, points_a())[name]()
    TIMES[name] = time.perf_counter() - t0
    return freeze(out)


def knn_prefix(ref32, k):
    """model_knn(.., k) from model_knn(.., 32) of the same rows: the first k of the same stable order (the definition; the CPU
    test proves it on the model)."""
    return {"d2": ref32["d2"][:, :k], "index": ref32["index"][:, :k]}


@functools.lru_cache(maxsize=None)
def many_points():
    """The m = 70 001 points over the small system (above 2^16, no multiple of 64) and their 2000-point sample for the
    long-double field oracle: the points on bodies, the ones outside the field and a seeded rest."""
    P = small_system()[0]
    pts = points_over(P, MANY, SMALL_FIELD, seed=21)
    rng = np.random.default_rng(22)
    fixed = np.concatenate([np.arange(400), np.arange(65500, 65600), np.arange(MANY - 100, MANY)])
    rest = np.setdiff1d(np.arange(MANY), fixed)
    sample = np.sort(np.concatenate([fixed, rng.choice(rest, size=2000 - len(fixed), replace=False)]))
    return freeze((pts, sample))
