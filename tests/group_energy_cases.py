"""The numpy model of the group energies (nbody_get_group_potential, nbody_batch_get_group_potential, nbody_group_catalog;
include/nbody.h) and the states its tests share.

Labels: group_cases' union-find over the definition's float64 links, bit for bit.

phi_in[i] = -G sum_{j != i, label[j] == label[i], r_ij > 0} m_j / r_ij.  The device sums it with fma-contracted terms, so
the model is an oracle with a bound, not a restatement: every term in np.longdouble in the style of
field_cases.exact_field, with the mask.  The bound is the diagnostics' derivation (test_gpu_diagnostics.py)
with n replaced by the number of terms actually summed: every term within 4 u of its exact value, one sign, the n_g fmas of
the running sum (non-members never reach it) at most n_g u of the sum:  |error| <= (n_g + 4) u |phi_in|,  n_g the size of
the body's group, u = 2^-53.  The bits themselves are pinned by the sub-state rule, product against product, in the GPU test.

The catalogue (nbody_group_catalog) has no fma and plain running sums in ascending member order: loop_catalog restates it
as a scalar loop over Python floats, model_catalog as numpy with np.add.at (unbuffered, in index order), and the two are
asserted equal in test_group_energy_cases_cpu.py."""
import numpy as np

import group_cases as gc
from field_cases import G, LD, U, require_long_double  # noqa: F401

PHI_C = 4
LINK, SCALE = 1.0, 1.0                                          # the test link of standard_state
STANDARD_N = (1, 2, 63, 64, 65, 127, 128, 129, 300)
GPU_N = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1500)
DTYPE_OF = {0: np.float32, 1: np.float64}
BIG = 130                                                       # members of standard_state's big group
BOUND = 1                                                       # NBODY_GROUP_BOUND

INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32),
                       ("coincident", np.int64)])
RECORD_DTYPE = np.dtype([("mass", np.float64), ("cx", np.float64), ("cy", np.float64), ("vx", np.float64),
                         ("vy", np.float64), ("kinetic", np.float64), ("potential", np.float64), ("energy", np.float64),
                         ("label", np.int32), ("count", np.int32), ("bound_members", np.int32), ("flags", np.int32)])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle of phi_in
# ---------------------------------------------------------------------------------------------------------------------
def exact_group_phi(P, M, label, rows=None):
    """-> (phi_in (k,) long double, coincident: ordered pairs (i, j) of one group at distance 0 over those rows, n_g (k,):
    the size of each row's group) for the bodies `rows` (None: all) of the state P (n, 2), M (n,), float64."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    label = np.asarray(label)
    n = len(label)
    x, y, m = P[:, 0].astype(LD), P[:, 1].astype(LD), np.asarray(M, dtype=np.float64).astype(LD)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    k = len(rows)
    phi = np.zeros(k, dtype=LD)
    coincident = 0
    for a in range(0, k, 16):
        r = rows[a:a + 16]
        dx = x[None, :] - x[r, None]
        dy = y[None, :] - y[r, None]
        member = label[None, :] == label[r, None]
        member[np.arange(len(r)), r] = False                    # the self term: left out by index, not counted
        same = member & (dx == 0) & (dy == 0)
        coincident += int(same.sum())
        take = member & ~same
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            d = np.sqrt(dx * dx + dy * dy)
            d[~take] = 1
            phi[a:a + 16] = -(LD(G) * np.where(take, m[None, :], LD(0)) / d).sum(axis=1)
    size = np.bincount(label, minlength=max(n, 1))[label[rows]] if n else np.zeros(0, dtype=np.int64)
    return phi, coincident, size


def phi_errors(got, phi, size):
    """-> error / bound per row; a bound of 0 asks for an exact 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(np.asarray(got).astype(LD) - phi)
        b = (size + PHI_C) * LD(U) * np.abs(phi)
        return np.where(e == 0, LD(0), e / b)


def assert_rows_within_bound(got_phi, P, M, label, what=""):
    """Every row, no sampling; -> the worst error / bound."""
    phi, coincident, size = exact_group_phi(P, M, label)
    r = phi_errors(got_phi, phi, size)
    worst = float(r.max()) if len(r) else 0.0
    print("%s: n %d worst error / bound %.3f" % (what, len(label), worst))
    assert np.isfinite(np.asarray(got_phi)).all() and worst <= 1.0, (what, worst, int(np.argmax(r)))
    alone = size == 1
    assert (bits(np.asarray(got_phi, dtype=np.float64)[alone]) == bits(np.float64(-0.0))).all(), what   # -G * +0
    return worst, coincident


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
def loop_catalog(P, V, M, label, phi):
    """nbody_group_catalog as a scalar loop over Python floats: one rounding per written operation, every sum over the
    group's members in ascending index starting from +0."""
    n = len(label)
    X, Y = [float(v) for v in np.asarray(P, dtype=np.float64).reshape(-1, 2)[:, 0]], [float(v) for v in np.asarray(P, dtype=np.float64).reshape(-1, 2)[:, 1]]
    VX, VY = [float(v) for v in np.asarray(V, dtype=np.float64).reshape(-1, 2)[:, 0]], [float(v) for v in np.asarray(V, dtype=np.float64).reshape(-1, 2)[:, 1]]
    Mm, Ph, L = [float(v) for v in M], [float(v) for v in phi], [int(v) for v in label]
    nan = float("nan")
    members = {}
    for i in range(n):
        members.setdefault(L[i], []).append(i)
    out = np.zeros(len(members), dtype=RECORD_DTYPE)
    for k, lab in enumerate(sorted(members)):
        mass = sx = sy = svx = svy = 0.0
        for i in members[lab]:
            mass = mass + Mm[i]
            sx = sx + (Mm[i] * X[i])
            sy = sy + (Mm[i] * Y[i])
            svx = svx + (Mm[i] * VX[i])
            svy = svy + (Mm[i] * VY[i])
        if mass == 0.0:
            cx = cy = vx = vy = nan
        else:
            cx, cy, vx, vy = sx / mass, sy / mass, svx / mass, svy / mass
        K2 = Pp = 0.0
        bound = 0
        for i in members[lab]:
            dvx = VX[i] - vx
            dvy = VY[i] - vy
            w = (dvx * dvx) + (dvy * dvy)
            K2 = K2 + (Mm[i] * w)
            Pp = Pp + (Mm[i] * Ph[i])
            bound += ((0.5 * w) + Ph[i]) < 0.0
        kin, pot = 0.5 * K2, 0.5 * Pp
        energy = kin + pot
        out[k] = (mass, cx, cy, vx, vy, kin, pot, energy, lab, len(members[lab]), bound, BOUND if energy < 0.0 else 0)
    return out


def model_catalog(P, V, M, label, phi):
    """The same in numpy: np.add.at adds in index order, unbuffered, so each group's sum runs over its members ascending."""
    P, V = np.asarray(P, dtype=np.float64).reshape(-1, 2), np.asarray(V, dtype=np.float64).reshape(-1, 2)
    M, phi, label = np.asarray(M, dtype=np.float64), np.asarray(phi, dtype=np.float64), np.asarray(label, dtype=np.int64)
    n = len(label)
    labs = np.flatnonzero(label == np.arange(n))
    out = np.zeros(len(labs), dtype=RECORD_DTYPE)
    if n == 0:
        return out
    slot = np.zeros(n, dtype=np.int64)
    slot[labs] = np.arange(len(labs))
    s = slot[label]
    sums = np.zeros((5, len(labs)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for row, term in enumerate((M, M * P[:, 0], M * P[:, 1], M * V[:, 0], M * V[:, 1])):
            np.add.at(sums[row], s, term)
        mass = sums[0]
        c = np.where(mass == 0.0, np.nan, sums[1:] / mass)
        dvx, dvy = V[:, 0] - c[2][s], V[:, 1] - c[3][s]
        w = (dvx * dvx) + (dvy * dvy)
        K2, Pp = np.zeros(len(labs)), np.zeros(len(labs))
        np.add.at(K2, s, M * w)
        np.add.at(Pp, s, M * phi)
        bound = np.bincount(s, weights=(((0.5 * w) + phi) < 0.0), minlength=len(labs))
        kin, pot = 0.5 * K2, 0.5 * Pp
        energy = kin + pot
    out["mass"], out["cx"], out["cy"], out["vx"], out["vy"] = mass, c[0], c[1], c[2], c[3]
    out["kinetic"], out["potential"], out["energy"] = kin, pot, energy
    out["label"], out["count"] = labs, np.bincount(s, minlength=len(labs))
    out["bound_members"], out["flags"] = bound.astype(np.int32), np.where(energy < 0.0, BOUND, 0)
    return out


def assert_same_catalog(got, want, what=""):
    """Zero tolerance on every field, NaN equal to NaN."""
    assert got.dtype == RECORD_DTYPE and want.dtype == RECORD_DTYPE and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    for f in RECORD_DTYPE.names:
        g, w = got[f], want[f]
        if g.dtype == np.float64:
            same = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
        else:
            same = g == w
        bad = np.flatnonzero(~same)
        assert bad.size == 0, (what, f, "%d records differ, first %d" % (bad.size, bad[0]), g[bad[:3]], w[bad[:3]])


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
SMALL_SIZES = (1, 2, 1, 3, 2, 5, 1, 2, 8, 2, 1, 4)            # of the groups next to the big one, in turns
CELL = 40.0                                                     # between the groups' cells: far above any link
SPACING = 0.5                                                   # between neighbours inside a group: linked at LINK
RADIUS = 0.05
MASS = 1e10                                                     # G m / SPACING is about 1.3: velocities of order 1 matter
FAST = 20                                                       # which member of the big group is the fast one


def standard_plan(n):
    """The groups standard_state is built to have at (LINK, SCALE): a list of ascending index arrays.
      * n >= 131: one group of BIG members - for n >= 300 the indices 40, 42, ..., 298 (every other one: across the tile
        boundaries 128 and 256, the second a workgroup boundary), below that the last BIG indices (across 128 or 256);
      * the other indices, shuffled by a fixed seed, cut into groups of SMALL_SIZES in turns: singletons, pairs and a few
        larger ones, with scattered members."""
    big = np.zeros(0, dtype=np.int64)
    if n >= 300:
        big = np.arange(40, 300, 2)
    elif n >= BIG + 1:
        big = np.arange(n - BIG, n)
    rest = np.setdiff1d(np.arange(n), big)
    rest = rest[np.random.default_rng(1000 + n).permutation(len(rest))]
    groups = [big] if len(big) else []
    a = k = 0
    while a < len(rest):
        size = SMALL_SIZES[k % len(SMALL_SIZES)]
        groups.append(np.sort(rest[a:a + size]))
        a += size
        k += 1
    return groups


def standard_state(n, dtype=np.float32):
    """-> (P (n, 2), V (n, 2), M (n,), R (n,)) float64 holding values of `dtype`.  Every group of standard_plan(n) sits in a
    cell of its own, CELL apart; its members are SPACING apart (a jittered lattice for the big group, a jittered row for
    the others), so at (LINK, SCALE) the groups are exactly the plan's.  Masses about MASS.  Velocities: a common drift per
    group plus, in turns, a cold (bound), a hot (unbound) and a cold spread; the big group is cold with ONE fast member -
    a bound group with an unbound member."""
    rng = np.random.default_rng(77 + n)
    groups = standard_plan(n)
    side = int(np.ceil(np.sqrt(max(len(groups), 1))))
    P, V = np.zeros((n, 2)), np.zeros((n, 2))
    for g, idx in enumerate(groups):
        k = len(idx)
        origin = np.array([10.0 + CELL * (g % side), 10.0 + CELL * (g // side)])
        if k == BIG:
            local = np.stack([np.arange(k) % 12, np.arange(k) // 12], axis=1) * SPACING
            spread = 0.05
        else:
            local = np.stack([np.arange(k) * SPACING, np.zeros(k)], axis=1)
            spread = (0.02, 30.0, 0.02)[g % 3]
        P[idx] = origin + local + rng.uniform(-0.05, 0.05, (k, 2))
        V[idx] = rng.uniform(-3.0, 3.0, 2) + rng.uniform(-spread, spread, (k, 2))
        if k == BIG:
            V[idx[FAST]] += (25.0, 0.0)
    M = MASS * rng.uniform(0.5, 1.5, n)
    R = np.full(n, RADIUS)
    return tuple(np.asarray(a, dtype=dtype).astype(np.float64) for a in (P, V, M, R))


def labels_of_plan(n):
    label = np.zeros(n, dtype=np.int32)
    for idx in standard_plan(n):
        label[idx] = idx[0]
    return label


# hand cases: (name, precision or None for both, P, V, M, R, link, radius_scale, expected phi bits or None, coincident)
def hand_cases():
    z2 = np.zeros((2, 2))
    yield ("a: two coincident bodies", None, np.array([[3.0, 4.0], [3.0, 4.0]]), z2, np.array([2.0, 5.0]), np.zeros(2), 0.0, 1.0,
           [-0.0, -0.0], [0, 0], 2)
    tiny = np.array([[1.0, 1.0], [1.0 + 0.0, 1.0], [2.0, 1.0]])
    tiny[0, 0], tiny[1, 0] = 0.0, 1e-155                        # d2 = 1e-310: subnormal and positive, not linked at link 0
    yield ("b: subnormal d2, not linked", 1, tiny, np.zeros((3, 2)), np.ones(3), np.zeros(3), 0.0, 1.0,
           [-0.0, -0.0, -0.0], [0, 1, 2], 0)
    P = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5], [9.0, 9.0]])
    yield ("c: all masses 0", None, P, np.zeros((4, 2)), np.zeros(4), np.zeros(4), 1.0, 0.0,
           [-0.0, -0.0, -0.0, -0.0], [0, 0, 0, 3], 0)
    yield ("d: one body", None, np.array([[3.0, 4.0]]), np.zeros((1, 2)), np.array([7.0]), np.array([1.0]), 5.0, 1.0,
           [-0.0], [0], 0)
