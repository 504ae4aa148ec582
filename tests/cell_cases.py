"""The numpy model of the cell sums (nbody_get_cells, nbody_batch_get_cells; include/nbody.h) and the states
their tests share.

The definition uses IEEE fp64 operations only, every one rounded on its own, no fma - numpy's elementwise float64 arithmetic
- so the model restates it bit for bit and the GPU tests compare with zero tolerance: integers exactly, doubles by their
bits.  Body j with the record (X, Y, M) and the velocity (VX, VY), an fp32 state widened exactly, on the grid {x0, y0, sx, sy,
nx, ny}:
    tx = (X - x0) * sx;  ty = (Y - y0) * sy
    inside(j)  <=>  0 <= tx && tx < nx && 0 <= ty && ty < ny        on the doubles; a NaN is outside
    cell(j) = (int)ty * nx + (int)tx  if inside(j), else -1          converted only after the compares
and per cell, over its members in ascending j, every accumulator from +0.0:
    mass = mass + M;  px = px + (M*VX);  py = py + (M*VY);  k2 = k2 + (M*((VX*VX) + (VY*VY)))
count the members, first the lowest of them (-1: none); cell_of[j] = cell(j); start the exclusive prefix sum of the counts;
order the members cell by cell, ascending inside a cell.

The ORDER of the sums is the contract.  model_cells takes them with np.cumsum over a cell's members, which adds one element
after the other (np.sum adds pairwise and is not used); loop_cells is the definition as a scalar loop over Python floats, and
test_cell_cases_cpu.py holds the one against the other."""
import numpy as np

from shell_cases import bits, lattice, order_sensitive_state, tenth_field  # noqa: F401  (the states the models share)

CELL_FIELDS = ("mass", "px", "py", "k2")
INFO_FIELDS = ("n", "inside", "outside", "occupied", "largest", "largest_cell")
CELL_DTYPE = np.dtype([("mass", np.float64), ("px", np.float64), ("py", np.float64), ("k2", np.float64), ("count", np.int32),
                       ("first", np.int32)])
VEL_SEED = 4409


def grid_of(nx, ny, bounds):
    """(x0, y0, sx, sy, nx, ny) as make_grid computes it: sx = nx / (x1 - x0) once, in fp64."""
    x0, x1, y0, y1 = (np.float64(v) for v in bounds)
    return (x0, y0, np.float64(nx) / (x1 - x0), np.float64(ny) / (y1 - y0), int(nx), int(ny))


def grid_tuple(g):
    """A GRID_DTYPE record (what Stepper.cells returns as "grid"), or a tuple -> the tuple."""
    if isinstance(g, tuple):
        return g
    return (np.float64(g["x0"]), np.float64(g["y0"]), np.float64(g["sx"]), np.float64(g["sy"]), int(g["nx"]), int(g["ny"]))


def cell_index(P, grid):
    """cell(j) for every body: int64 (n,), -1 outside."""
    x0, y0, sx, sy, nx, ny = grid_tuple(grid)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        tx = (P[:, 0] - x0) * sx
        ty = (P[:, 1] - y0) * sy
        inside = (0.0 <= tx) & (tx < np.float64(nx)) & (0.0 <= ty) & (ty < np.float64(ny))
    ix = np.where(inside, tx, 0.0).astype(np.int64)             # converted only after the compares
    iy = np.where(inside, ty, 0.0).astype(np.int64)
    return np.where(inside, iy * nx + ix, -1)


def model_cells(P, V, M, grid, moments=True, descending=False):
    """The definition over the bodies P (n, 2), V (n, 2), M (n,), float64 (an fp32 state widened exactly) -> what
    Stepper.cells(lists=True) returns: {"cells": CELL_DTYPE (ny, nx), "cell_of", "start", "order", "info"}.  descending=True
    adds every cell's members in descending j instead: NOT the contract, only what the tests hold a state's sensitivity to
    the order against."""
    x0, y0, sx, sy, nx, ny = grid_tuple(grid)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 2)
    M = np.asarray(M, dtype=np.float64).reshape(-1)
    n, C = len(P), nx * ny
    cell = cell_index(P, grid)
    members = np.flatnonzero(cell >= 0)
    order = members[np.argsort(cell[members], kind="stable")]   # cell by cell, ascending inside a cell
    count = np.bincount(cell[members], minlength=C).astype(np.int64)
    start = np.zeros(C + 1, dtype=np.int64)
    start[1:] = np.cumsum(count)
    out = np.zeros(C, dtype=CELL_DTYPE)
    out["count"] = count
    out["first"] = -1
    with np.errstate(over="ignore", invalid="ignore"):
        terms = {"mass": M, "px": M * V[:, 0], "py": M * V[:, 1], "k2": M * ((V[:, 0] * V[:, 0]) + (V[:, 1] * V[:, 1]))}
        for c in np.flatnonzero(count):
            seg = order[start[c]:start[c + 1]]
            out["first"][c] = seg[0]
            if descending:
                seg = seg[::-1]
            for f in CELL_FIELDS if moments else ("mass",):
                out[f][c] = np.cumsum(np.concatenate(([0.0], terms[f][seg])))[-1]   # from +0.0, one after the other
    inside = int(len(members))
    largest = int(count.max()) if C else 0
    info = {"n": n, "inside": inside, "outside": n - inside, "occupied": int((count > 0).sum()), "largest": largest,
            "largest_cell": int(np.argmax(count))}              # argmax: the lowest cell that has it
    return {"cells": out.reshape(ny, nx), "cell_of": cell.astype(np.int32), "start": start.astype(np.int32),
            "order": order.astype(np.int32), "info": info}


def loop_cells(P, V, M, grid, moments=True):
    """The definition as a plain scalar loop over Python floats (IEEE doubles, one rounding per operation)."""
    x0, y0, sx, sy, nx, ny = (float(v) if k < 4 else int(v) for k, v in enumerate(grid_tuple(grid)))
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    V = np.asarray(V, dtype=np.float64).reshape(-1, 2)
    X, Y = [float(v) for v in P[:, 0]], [float(v) for v in P[:, 1]]
    VX, VY = [float(v) for v in V[:, 0]], [float(v) for v in V[:, 1]]
    Mm = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)]
    n, C = len(X), nx * ny
    acc = [[0.0, 0.0, 0.0, 0.0] for _ in range(C)]
    count, first, cell_of = [0] * C, [-1] * C, [-1] * n
    lists = [[] for _ in range(C)]
    for j in range(n):
        tx = (X[j] - x0) * sx
        ty = (Y[j] - y0) * sy
        if not (0.0 <= tx and tx < nx and 0.0 <= ty and ty < ny):
            continue
        c = int(ty) * nx + int(tx)
        cell_of[j] = c
        if count[c] == 0:
            first[c] = j
        count[c] += 1
        lists[c].append(j)
        a = acc[c]
        a[0] = a[0] + Mm[j]
        if moments:
            a[1] = a[1] + (Mm[j] * VX[j])
            a[2] = a[2] + (Mm[j] * VY[j])
            a[3] = a[3] + (Mm[j] * ((VX[j] * VX[j]) + (VY[j] * VY[j])))
    out = np.zeros(C, dtype=CELL_DTYPE)
    for c in range(C):
        out[c] = (acc[c][0], acc[c][1], acc[c][2], acc[c][3], count[c], first[c])
    start = [0]
    for c in range(C):
        start.append(start[-1] + count[c])
    order = [j for c in range(C) for j in lists[c]]
    inside = start[-1]
    largest = max(count) if C else 0
    info = {"n": n, "inside": inside, "outside": n - inside, "occupied": sum(1 for v in count if v), "largest": largest,
            "largest_cell": count.index(largest)}
    return {"cells": out.reshape(ny, nx), "cell_of": np.asarray(cell_of, dtype=np.int32), "start": np.asarray(start, dtype=np.int32),
            "order": np.asarray(order, dtype=np.int32), "info": info}


def info_dict(info):
    """The info of a result - a dict, or a CELLS_INFO_DTYPE record of a batch - as a dict of ints."""
    return {k: int(info[k]) for k in INFO_FIELDS}


def assert_same(got, want, what="", lists=True):
    """Zero tolerance: integers exactly, doubles by their bits."""
    gc, wc = np.asarray(got["cells"]), np.asarray(want["cells"])
    assert gc.dtype == CELL_DTYPE and gc.shape == wc.shape, (what, gc.dtype, gc.shape, wc.shape)
    for f in ("count", "first"):
        bad = np.argwhere(gc[f] != wc[f])
        assert len(bad) == 0, (what, "%d cells differ in %s, first at %s" % (len(bad), f, bad[0]), gc[f][tuple(bad[0])],
                               wc[f][tuple(bad[0])])
    for f in CELL_FIELDS:
        bad = np.argwhere(bits(gc[f]) != bits(wc[f]))
        assert len(bad) == 0, (what, "%d cells differ by bits in %s, first at %s" % (len(bad), f, bad[0]),
                               repr(gc[f][tuple(bad[0])]), repr(wc[f][tuple(bad[0])]))
    assert info_dict(got["info"]) == info_dict(want["info"]), (what, info_dict(got["info"]), info_dict(want["info"]))
    if lists:
        for f in ("cell_of", "start", "order"):
            g, w = np.asarray(got[f]), np.asarray(want[f])
            assert g.dtype == np.int32 and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (what, "%d entries of %s differ, first at %d" % (len(bad), f, bad[0]), g[bad[0]], w[bad[0]])


def lists_consistent(res):
    """The lists against the sums of one result: start is the prefix sum of count, order's segments are the ascending indices
    where cell_of == c, first is each segment's head."""
    cells = np.asarray(res["cells"]).reshape(-1)
    cell_of, start, order = res["cell_of"], res["start"], res["order"]
    assert start[0] == 0 and np.array_equal(np.diff(start), cells["count"])
    assert start[-1] == info_dict(res["info"])["inside"] == len(order)
    for c in range(len(cells)):
        seg = order[start[c]:start[c + 1]]
        assert np.array_equal(seg, np.flatnonzero(cell_of == c)), c
        assert cells["first"][c] == (seg[0] if len(seg) else -1), c
    return True


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
def velocities(n, dtype, seed=VEL_SEED):
    """n velocities, normal with a spread of 30, rounded to dtype -> (n, 2) float64."""
    return np.random.default_rng(seed).normal(0.0, 30.0, size=(n, 2)).astype(dtype).astype(np.float64)


def moving_state(n, dtype, field=None):
    """order_sensitive_state(n, dtype) - masses over thirteen decades - with velocities -> (P, V, M) float64."""
    P, M = order_sensitive_state(n, dtype, field=field)
    return P, velocities(n, dtype), M


def sized_state(sizes, dtype, nx=8, seed=23):
    """A state by construction on the nx x nx grid over [0, nx)^2: cell k gets exactly sizes[k] members, placed well inside
    it, the bodies in a random order - a cell's members are spread over the whole index range, so its segment is filled by
    many waves and workgroups.  Masses over thirteen decades and random velocities -> (P, V, M) float64, the grid bounds."""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.arange(len(sizes)), sizes)
    n = len(cell)
    cell = cell[rng.permutation(n)]
    off = rng.uniform(0.125, 0.875, size=(n, 2))
    P = (np.stack([cell % nx, cell // nx], axis=1) + off).astype(dtype).astype(np.float64)
    M = (10.0 ** rng.uniform(4.0, 17.0, size=n)).astype(dtype).astype(np.float64)
    return P, velocities(n, dtype, seed + 1), M, (0.0, float(nx), 0.0, float(nx))


def order_matters(P, V, M, grid):
    """How many cells' mass and px differ by bits from the same sums taken in descending j."""
    up, down = model_cells(P, V, M, grid), model_cells(P, V, M, grid, descending=True)
    assert np.array_equal(up["cells"]["count"], down["cells"]["count"])
    return (int((bits(up["cells"]["mass"]) != bits(down["cells"]["mass"])).sum()),
            int((bits(up["cells"]["px"]) != bits(down["cells"]["px"])).sum()))
