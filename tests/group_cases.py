"""The numpy model of group finding (nbody_get_groups, nbody_batch_get_groups; include/nbody.h) and the states
its tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare labels with zero tolerance.  Bodies i != j with records
(X, Y, R), an fp32 state widened exactly:
    dx = X_j - X_i;  dy = Y_j - Y_i;  d2 = (dx*dx) + (dy*dy)
    s  = (radius_scale * (R_i + R_j)) + link
    linked(i, j)  <=>  d2 <= s*s
A group is a connected component of the undirected graph of links; label[i] is the lowest index in body i's group.

A NaN d2 or a NaN s*s fails the comparison: such a pair is not linked.  With (link, radius_scale) = (0, 1) the predicate is
the overlap predicate of neighbor_cases.model_neighbors."""
import numpy as np

from neighbor_cases import lattice, random_state, widen  # noqa: F401  (the states the two models share)

INFO_DTYPE = np.dtype([("n_bodies", np.int32), ("n_groups", np.int32), ("largest", np.int32), ("sweeps", np.int32)])


def adjacency(P, R, link, radius_scale):
    """linked(i, j) for every ordered pair, (n, n) bool with a False diagonal: the definition, elementwise in float64."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    X, Y = P[:, 0], P[:, 1]
    link, radius_scale = np.float64(link), np.float64(radius_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = X[None, :] - X[:, None]                            # [i, j] = X_j - X_i
        dy = Y[None, :] - Y[:, None]
        d2 = (dx * dx) + (dy * dy)
        s = (radius_scale * (R[:, None] + R[None, :])) + link
        A = d2 <= s * s
    A[np.arange(len(R)), np.arange(len(R))] = False
    return A


def labels_of(A):
    """Connected components of a symmetric adjacency by union-find with the lower root kept: label[i] = the lowest index
    of i's component."""
    n = len(A)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(A, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def summary(label):
    """(n_groups, largest) of a label array."""
    label = np.asarray(label)
    if len(label) == 0:
        return 0, 0
    return int((label == np.arange(len(label))).sum()), int(np.bincount(label).max())


def model_groups(P, R, link, radius_scale=1.0):
    """-> {"label": int32 (n,), "n_groups", "largest"}: the definition over the bodies P (n, 2), R (n,), float64."""
    label = labels_of(adjacency(P, R, link, radius_scale))
    n_groups, largest = summary(label)
    return {"label": label, "n_groups": n_groups, "largest": largest}


def loop_groups(P, R, link, radius_scale=1.0):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation) and a breadth-first
    search from every unlabelled body in ascending order, so the seed of a group is its lowest index."""
    n = len(R)
    X, Y, Rr = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]], [float(v) for v in R]
    link, radius_scale = float(link), float(radius_scale)

    def linked(i, j):
        dx = X[j] - X[i]
        dy = Y[j] - Y[i]
        try:
            d2 = (dx * dx) + (dy * dy)
        except OverflowError:                                    # Python raises where IEEE gives +inf
            d2 = float("inf")
        s = (radius_scale * (Rr[i] + Rr[j])) + link
        try:
            s2 = s * s
        except OverflowError:
            s2 = float("inf")
        return d2 <= s2

    label = [-1] * n
    for seed in range(n):
        if label[seed] >= 0:
            continue
        label[seed] = seed
        todo = [seed]
        while todo:
            i = todo.pop()
            for j in range(n):
                if label[j] < 0 and j != i and linked(i, j):
                    label[j] = seed
                    todo.append(j)
    label = np.array(label, dtype=np.int32).reshape(n)
    n_groups, largest = summary(label)
    return {"label": label, "n_groups": n_groups, "largest": largest}


def assert_same(got, want, what=""):
    """Zero tolerance: every label, and the two counts that follow from them."""
    g, w = np.asarray(got["label"]), np.asarray(want["label"])
    assert g.dtype == np.int32 and g.shape == w.shape, (what, g.dtype, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, "%d labels differ, first at %d" % (bad.size, bad[0]), g[bad[:4]], w[bad[:4]])
    assert (got["n_groups"], got["largest"]) == (want["n_groups"], want["largest"]), what


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
def shuffled_chain(n=300, spacing=1.0, radius=0.25, seed=5):
    """n bodies on a line, `spacing` apart, in a random order of the indices: consecutive positions are linked from
    link = spacing - 2 * radius on (radius_scale 1), and then the one group's lowest index is 0 wherever body 0 lies - a
    label has up to n - 1 links to travel."""
    order = np.random.default_rng(seed).permutation(n)
    P = np.zeros((n, 2))
    P[order, 0] = np.arange(n) * spacing
    P[:, 1] = 3.0
    return P, np.full(n, radius)


def window_groups(P, R, link, radius_scale=1.0):
    """model_groups for states too large for an n x n matrix (finite values, a finite link): the bodies sorted by x, and body
    a paired with its k-th successor for k = 1, 2, ... as long as any successor lies within the largest possible s in x.
    Every candidate pair goes through the definition's own float64 arithmetic (the same bits as `adjacency`: dx only changes
    sign with the order of the pair); the pairs left out have |dx| > every s, so d2 > s*s.  Labels by hooking roots and
    pointer jumping until every linked pair shares a root."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    R = np.asarray(R, dtype=np.float64).reshape(-1)
    n = len(R)
    link, radius_scale = np.float64(link), np.float64(radius_scale)
    assert np.isfinite(P).all() and np.isfinite(R).all() and np.isfinite(link)
    label = np.arange(n, dtype=np.int64)
    if n < 2:
        return model_groups(P, R, link, radius_scale)
    order = np.argsort(P[:, 0], kind="stable")
    X, Y, Rs = P[order, 0], P[order, 1], R[order]
    reach = (radius_scale * (2.0 * np.abs(R).max()) + link) * (1 + 2.0 ** -40)      # above every s, roundings included
    A, B = [], []
    for k in range(1, n):
        dx = X[k:] - X[:-k]
        near = dx <= reach
        if not near.any():
            break
        a = np.flatnonzero(near)
        dxa = dx[a]
        dy = Y[a + k] - Y[a]
        d2 = (dxa * dxa) + (dy * dy)
        s = (radius_scale * (Rs[a] + Rs[a + k])) + link
        hit = d2 <= s * s
        A.append(order[a[hit]])
        B.append(order[a[hit] + k])
    A, B = (np.concatenate(A), np.concatenate(B)) if A else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    while True:
        ra, rb = label[A], label[B]
        if (ra == rb).all():
            break
        np.minimum.at(label, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = label[label]
            if np.array_equal(up, label):
                break
            label = up
    label = label.astype(np.int32)
    n_groups, largest = summary(label)
    return {"label": label, "n_groups": n_groups, "largest": largest, "links": int(len(A))}
