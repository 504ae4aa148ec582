"""Encounters on the cell list (nbody_get_encounters_grid, nbody_batch_get_encounters_grid; encounters(grid=...) of Stepper and
StepperBatch) on the MI355X.

Counts are integers and the list is sorted by (t, i, j) on the host from values that do not depend on which end of a pair
evaluated it: zero tolerance throughout - against the numpy model of encounters_grid_cases.py (the plain model on the inside
bodies) and product against product (the plain call, another grid, a Stepper holding only the inside bodies, a batch against a
Stepper).  test_encounters_grid_cases_cpu.py holds, for every constructed case and grid used here, that every swept pair lies
inside its owner's window; the test on a stepped state holds it on the downloaded state before it asks."""
import numpy as np
import pytest

import encounter_cases as ec
import encounters_grid_cases as eg
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
INF = float("inf")
PREC = {"f32": 0, "f64": 1}
TAGS = tuple(PREC)


def small_stepper(nb, precision, capacity, **kw):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=eg.TIME_STEP, growthRate=0.1, fieldWidth=1000000,
                      fieldHeight=1000000, **kw)


def bodies_of(nb, P, V, R, precision):
    n = len(R)
    return nb.BodiesData.from_arrays(P, V, np.ones(n), R, precision) if n else nb.BodiesData(0, precision)


def enc_bytes(r):
    lst, info = r
    return (lst.tobytes(), tuple(info[f] for f in ec.COUNTS[1:]), np.float64(info["horizon"]).tobytes())


def ask(st, S, grid, h, what="", cap=None):
    got = st.encounters(h, grid=grid, cap=cap)
    want = eg.model_encounters_grid(*S, got[1]["grid"], h)
    print("%s encounters: %s" % (what, {k: v for k, v in got[1].items() if k != "grid"}))
    eg.assert_same(got, want, what)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. workgroup and wave edges: 8 x 8, 1 x 1 and a grid that leaves bodies outside
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", eg.BODY_COUNTS)
def test_body_edges(nb, n, tag):
    S = eg.standard(n, tag)
    P = S[0]
    grids = [nb.make_grid(*a) for a in eg.standard_grids(n)]
    with small_stepper(nb, PREC[tag], n) as st, small_stepper(nb, PREC[tag], n) as sub:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        got = [ask(st, S, g, eg.H, what="n %d grid %d" % (n, k)) for k, g in enumerate(grids)]
        plain = st.encounters(eg.H)
        assert got[0][1]["outside"] == 0 == got[1][1]["outside"] and got[0][1]["inside"] == n
        assert enc_bytes(got[0]) == enc_bytes(got[1]) == enc_bytes(plain)
        # the partial grid: what the plain call gives on a context holding exactly the inside bodies
        idx = np.flatnonzero(eg.inside_of(P, grids[2][0]))
        assert got[2][1]["inside"] == len(idx)
        sub.upload(bodies_of(nb, *[a[idx] for a in S], PREC[tag]))
        lst, info = sub.encounters(eg.H)
        lst = lst.copy()
        lst["i"], lst["j"] = idx[lst["i"]], idx[lst["j"]]
        assert enc_bytes((lst, info)) == enc_bytes(got[2])
        if n >= 63:
            assert 0 < len(idx) < n and 0 < got[2][1]["pairs"] < got[0][1]["pairs"] and got[0][1]["pairs"] >= 33


# ---------------------------------------------------------------------------------------------------------------------
# 2. the constructed cases, each on every grid shape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.case_names())
def test_constructed_cases(nb, name):
    c = eg.cases()[name]
    with small_stepper(nb, PREC[c.tag], 16) as st:
        st.upload(bodies_of(nb, *c.state, PREC[c.tag]))
        plain = st.encounters(c.h)
        for k in c.asks:
            got = ask(st, c.state, nb.make_grid(*k), c.h, what="%s %d x %d" % (name, k[0], k[1]))
            for f, v in c.expect.items():
                assert got[1][f] == v, (name, k, f, got[1][f], v)
            if got[1]["outside"] == 0:
                assert enc_bytes(got) == enc_bytes(plain), (name, k)
            counts = st.encounters(c.h, grid=nb.make_grid(*k), cap=0)      # cap 0 first: the counts, then the list
            assert enc_bytes(counts) == enc_bytes(got), (name, k)


# ---------------------------------------------------------------------------------------------------------------------
# 3. horizons
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_horizons(nb, tag):
    S = eg.horizon_state(tag)
    full, one, part = (nb.make_grid(*a) for a in eg.standard_grids(300))
    with small_stepper(nb, PREC[tag], 300) as st:
        st.upload(bodies_of(nb, *S, PREC[tag]))
        for h in eg.HORIZONS + (1e-300,):
            a = ask(st, S, full, h, what="h %g" % h)
            ask(st, S, part, h, what="h %g partial" % h)
            assert enc_bytes(a) == enc_bytes(st.encounters(h)) and a[1]["pairs"] > 0
            if h == 0.0:
                assert a[1]["pairs"] == a[1]["now"] == a[1]["end"] and 2 * a[1]["now"] == int(st.neighbors()["overlaps"].sum())
        assert enc_bytes(st.encounters(grid=full)) == enc_bytes(st.encounters())       # horizon=None: the context's time step
        assert st.encounters(grid=full)[1]["horizon"] == (float(np.float32(eg.TIME_STEP)) if tag == "f32" else eg.TIME_STEP)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cap
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity(nb):
    n = 300
    S = eg.standard(n, "f32")
    full, _, part = (nb.make_grid(*a) for a in eg.standard_grids(n))
    call = nb.lib.nbody_get_encounters_grid
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, *S, 0))
        for grid in (full, part):
            want, winfo = eg.model_encounters_grid(*S, grid[0], eg.H)
            pairs = winfo["pairs"]
            counts = tuple(winfo[f] for f in ec.COUNTS) + (eg.H, winfo["inside"], winfo["outside"])
            out = np.frombuffer(bytes([0x77]) * (24 * (pairs + 4)), dtype=ec.RECORD_DTYPE).copy()
            before = out.tobytes()
            info = np.full(1, -7, dtype=nb.ENCOUNTER_GRID_INFO_DTYPE)
            assert call(st._ctx, grid.ctypes.data, eg.H, out.ctypes.data, pairs - 1, info.ctypes.data) == CAPACITY_ERR
            assert out.tobytes() == before and tuple(info[0]) == counts   # out untouched, info complete
            info[:] = -7
            assert call(st._ctx, grid.ctypes.data, eg.H, None, 0, info.ctypes.data) == 0   # the counts only
            assert tuple(info[0]) == counts
            info[:] = -7
            assert call(st._ctx, grid.ctypes.data, eg.H, out.ctypes.data, pairs, info.ctypes.data) == 0   # it still answers
            assert tuple(info[0]) == counts and out[pairs:].tobytes() == before[24 * pairs:]
            for f in ("i", "j", "flags"):
                assert np.array_equal(out[f][:pairs], want[f])
            assert np.array_equal(out["t"][:pairs].view(np.uint64), want["t"].view(np.uint64))
            # the wrapper: a guess that is too small is repeated once with info.pairs
            for cap in (3 * n, 1, 0, pairs):
                ask(st, S, grid, eg.H, what="cap %d" % cap, cap=cap)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a stepped state, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
def test_resident_state_after_collisions(nb):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=7013)
    w = float(dense_field(n))
    dt = float(np.float32(cfg.timestep))
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as twin:
        st.upload(b)
        twin.upload(b)
        st.step(3)
        twin.step(3)
        S = ec.widen(st.download())
        P, V, R = S
        assert len(R) < n and np.abs(V).max() > 0                 # compaction has run, the bodies move
        r_typical, v_typical = float(np.median(np.abs(R))), float(np.median(np.abs(V[:, 0]) + np.abs(V[:, 1])))
        lo, hi = P.min(axis=0) - 1.0, P.max(axis=0) + 1.0
        for h in (dt, 10 * dt):
            matched = nb.encounters_grid((w, w), h, r_typical, v_typical)
            fitted = nb.make_grid(int(matched["nx"][0]), int(matched["ny"][0]), (lo[0], hi[0], lo[1], hi[1]))
            plain = st.encounters(h)
            for grid in (matched, fitted):
                swept = eg.window_holds(P, V, R, grid[0], h, np.float32)   # on the downloaded state first
                got = ask(st, S, grid, h, what="stepped h %g" % h)
                assert got[1]["outside"] == 0 and got[1]["pairs"] == swept > 0, grid   # both grids hold every body
                assert enc_bytes(got) == enc_bytes(plain), grid
        assert enc_bytes(st.encounters(grid=matched)) == enc_bytes(st.encounters())
        st.step(2)
        twin.step(2)
        assert st.download().block.tobytes() == twin.download().block.tobytes()
        assert int(st.stats().pairs) == int(twin.stats().pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_equals_steppers_and_model(nb):
    cap, Sn = eg.BATCH_CAP, len(eg.BATCH_COUNTS)
    states = eg.batch_states()
    bodies = [bodies_of(nb, *s, 0) for s in states]
    with nb.StepperBatch(Sn, cap, params=[(eg.TIME_STEP, 0.1, 1000000, 1000000)] * Sn) as batch, small_stepper(nb, 0, cap) as one:
        batch.upload(bodies)
        assert batch.counts().tolist() == list(eg.BATCH_COUNTS)
        for k, a in enumerate(eg.batch_grids()):
            grid = nb.make_grid(*a)
            gb = batch.encounters(eg.H, grid=grid)
            assert len(gb) == Sn
            worst = max(b[1]["pairs"] for b in gb)
            # the C call into a prefilled buffer: the tails stay
            out = np.frombuffer(bytes([0x77]) * (24 * Sn * (worst + 3)), dtype=ec.RECORD_DTYPE).copy().reshape(Sn, worst + 3)
            binfo = np.zeros(Sn, dtype=nb.ENCOUNTER_GRID_INFO_DTYPE)
            call = nb.lib.nbody_batch_get_encounters_grid
            assert call(batch._b, grid.ctypes.data, eg.H, out.ctypes.data, worst + 3, binfo.ctypes.data) == 0
            assert worst > 0 and call(batch._b, grid.ctypes.data, eg.H, out.ctypes.data, worst - 1, binfo.ctypes.data) == CAPACITY_ERR
            for s, S in enumerate(states):
                n = eg.BATCH_COUNTS[s]
                what = "system %d (n %d) grid %r" % (s, n, a)
                eg.assert_same(gb[s], eg.model_encounters_grid(*S, grid[0], eg.H), what)
                p = gb[s][1]["pairs"]
                assert int(binfo["pairs"][s]) == p and (out[s, p:].view(np.uint8) == 0x77).all(), what
                assert np.array_equal(out[s, :p]["i"], gb[s][0]["i"]) and np.array_equal(out[s, :p]["j"], gb[s][0]["j"]), what
                assert (int(binfo["inside"][s]), int(binfo["outside"][s])) == (gb[s][1]["inside"], gb[s][1]["outside"]), what
                if n == 0:
                    assert (gb[s][1]["pairs"], gb[s][1]["inside"], gb[s][1]["outside"]) == (0, 0, 0)
                    continue
                one.upload(bodies[s])                             # a Stepper holding the same state
                assert enc_bytes(one.encounters(eg.H, grid=grid)) == enc_bytes(gb[s]), what
            if k == 0:
                assert all(g[1]["outside"] == 0 for g in gb)
                assert all(enc_bytes(x) == enc_bytes(y) for x, y in zip(gb, batch.encounters(eg.H)))
            else:
                assert gb[2][1]["outside"] > 0 and gb[3][1]["outside"] > 0 and gb[3][1]["pairs"] > 0
            counts = batch.encounters(eg.H, grid=grid, cap=0)
            assert all(enc_bytes(x) == enc_bytes(y) for x, y in zip(gb, counts))


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors on live handles
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    S = eg.standard(300, "f32")
    grid = nb.make_grid(*eg.standard_grids(300)[0])
    bad_grid = nb.make_grid(0, 4, (0, 1, 0, 1))
    call, bcall = nb.lib.nbody_get_encounters_grid, nb.lib.nbody_batch_get_encounters_grid
    out = np.frombuffer(bytes([0x77]) * (24 * 512), dtype=ec.RECORD_DTYPE).copy()
    info = np.full(2, -7, dtype=nb.ENCOUNTER_GRID_INFO_DTYPE)
    untouched = (out.tobytes(), info.tobytes())
    G, O, I = grid.ctypes.data, out.ctypes.data, info.ctypes.data

    def bad_arguments(fn, handle):
        for h in (float("nan"), -1.0, -INF):
            assert fn(handle, G, h, O, 512, I) == INVALID and b"horizon" in nb.lib.nbody_last_error_string()
        assert fn(handle, bad_grid.ctypes.data, eg.H, O, 512, I) == INVALID
        assert fn(handle, None, eg.H, O, 512, I) == INVALID
        assert fn(handle, G, eg.H, O, 512, None) == INVALID
        assert fn(handle, G, eg.H, O, -1, I) == INVALID
        assert fn(handle, G, eg.H, None, 4, I) == INVALID
        assert (out.tobytes(), info.tobytes()) == untouched

    want = eg.model_encounters_grid(*S, grid[0], eg.H)
    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, G, eg.H, O, 512, I) == STATE_ERR and b"before" in nb.lib.nbody_last_error_string()
        bad_arguments(call, st._ctx)                                # refused before the state is looked at
        st.upload(bodies_of(nb, *S, 0))
        bad_arguments(call, st._ctx)
        eg.assert_same(st.encounters(eg.H, grid=grid), want, "after the refusals")
        st.upload(nb.BodiesData(0))                                 # no bodies: nothing launched
        assert call(st._ctx, G, eg.H, None, 0, I) == 0 and tuple(info[0]) == (0, 0, 0, 0, 0, eg.H, 0, 0)
        info[:] = -7
    with nb.StepperBatch(2, 300, params=[(eg.TIME_STEP, 0.1, 1000000, 1000000)] * 2) as batch:
        assert bcall(batch._b, G, eg.H, O, 256, I) == STATE_ERR
        batch.upload([bodies_of(nb, *S, 0), nb.BodiesData(0)])
        bad_arguments(bcall, batch._b)
        got = batch.encounters(eg.H, grid=grid)
        eg.assert_same(got[0], want, "batch after the refusals")
        assert len(got[1][0]) == 0 and [got[1][1][f] for f in ec.COUNTS] == [0] * 5
    # a rank holds only its own velocities: a group-exchange context and a FORCE_COMM context are refused
    grp = nb.StepperGroup(2, capacity=300, timestep=eg.TIME_STEP, growthRate=0.1, fieldWidth=1000000, fieldHeight=1000000)
    try:
        grp.upload(bodies_of(nb, *S, 0))
        for r in grp.ranks:
            assert call(r._ctx, G, eg.H, O, 512, I) == STATE_ERR and b"single-rank" in nb.lib.nbody_last_error_string()
    finally:
        grp.close()
    with small_stepper(nb, 0, 300, comm_id=nb.comm_unique_id(), force_comm=True) as rc:
        rc.upload(bodies_of(nb, *S, 0))
        assert call(rc._ctx, G, eg.H, O, 512, I) == STATE_ERR and b"single-rank" in nb.lib.nbody_last_error_string()
    assert (out.tobytes(), info.tobytes()) == untouched


# ---------------------------------------------------------------------------------------------------------------------
# 8. reads only: stepping after several calls is what stepping without them is
# ---------------------------------------------------------------------------------------------------------------------
def test_no_effect_on_stepping(nb):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=7017)
    b.Velocities[:] = ec.standard_state(n, np.float32)[1]          # the stock generator leaves every body at rest
    w = float(dense_field(n))
    dt = float(np.float32(cfg.timestep))

    def run(with_calls):
        with nb.Stepper(cfg, record_events=True) as st:
            st.upload(b)
            for s in range(3):
                if s:
                    st.step(1)
                if with_calls:
                    for grid in (nb.encounters_grid((w, w), dt, 4.0, 40.0), nb.make_grid(1, 1, (-w, w, -w, w))):
                        st.encounters(grid=grid)
                        st.encounters(5.0, grid=grid, cap=0)
            d = st.download()
            return (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                    np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes())
    assert run(False) == run(True)
