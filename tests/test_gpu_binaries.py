"""Bound-pair queries (nbody_get_binaries, nbody_batch_get_binaries; Stepper.binaries, StepperBatch.binaries) on the MI355X:
the pairs of the resident state within a separation that are bound as a two-body system.

The definition has no fma and rounds every operation on its own; the device decides which pairs are near and bound with
subtractions, multiplies, additions and compares, the host computes the orbit with the C library's sqrt and division.  The
numpy model of binary_cases.py restates every bit: zero tolerance throughout - a, ecc, period and sep by bits, i, j, flags and
every field of info."""
import functools
import time

import numpy as np
import pytest

import binary_cases as bc
from lineage_cases import dense_bodies

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
INF = float("inf")
SEP2 = bc.SEP * bc.SEP
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


def small_stepper(nb, precision, capacity, **kw):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=1000000,
                      fieldHeight=1000000, **kw)


def bodies_of(nb, P, V, M, R, precision):
    return nb.BodiesData.from_arrays(P, V, M, R, precision) if len(R) else nb.BodiesData(0, precision)


@functools.lru_cache(maxsize=None)
def standard(n, precision, sep2):
    """The standard state and its model at sep2, computed once."""
    state = bc.standard_state(n, bc.DTYPE_OF[precision])
    return state, bc.model_binaries(*state, sep2)


def check(st, state, sep2, what):
    """binaries() of the resident state against the model of `state`; -> the result."""
    got = st.binaries(sep2, squared=True)
    bc.assert_same(got, bc.model_binaries(*state, sep2), what)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile, wave and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 5) + bc.STANDARD_N)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    with small_stepper(nb, precision, n) as st:
        state, want = standard(n, precision, SEP2)
        st.upload(bodies_of(nb, *state, precision))
        got = st.binaries(bc.SEP)                                   # the wrapper squares with one multiply
        print("n %d: %s" % (n, got[1]))
        bc.assert_same(got, want, "n %d" % n)
        if n in (129, 300):
            for sep2 in (0.0, INF):
                bc.assert_same(st.binaries(sep2, squared=True), standard(n, precision, sep2)[1], "n %d sep2 %g" % (n, sep2))
        # symmetry: the body order reversed, the indices mapped back: the same set with the same orbit bits
        st.upload(bodies_of(nb, *[a[::-1] for a in state], precision))
        lst, info = st.binaries(bc.SEP)
        bc.assert_same((bc.reversed_back(lst, n), info), want, "n %d reversed" % n)


# ---------------------------------------------------------------------------------------------------------------------
# 2. special states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_special_states(nb, precision):
    n = 300
    (P, V, M, R), (base, binfo) = standard(n, precision, SEP2)
    k = int(base["i"][len(base) // 2])                              # a body of a bound pair
    mine = (base["i"] == k) | (base["j"] == k)
    with small_stepper(nb, precision, n) as st:
        # a NaN position, velocity or mass removes exactly that body's pairs from the list; only the position from `near`
        for which, what in ((0, "position"), (1, "velocity"), (2, "mass")):
            S = [P.copy(), V.copy(), M.copy(), R.copy()]
            S[which][(k, 1) if which < 2 else k] = np.nan
            st.upload(bodies_of(nb, *S, precision))
            for sep2 in (SEP2, INF):
                lst, info = check(st, S, sep2, "NaN %s, sep2 %g" % (what, sep2))
            lst, info = check(st, S, SEP2, "NaN " + what)
            assert np.array_equal(lst, base[~mine]) and len(lst) < len(base)
            assert (info["near"] < binfo["near"]) == (which == 0)
        # coincident bodies: in different tiles, in different waves of a tile, in the same wave; counted, never listed
        S = [P.copy(), V.copy(), M.copy(), R.copy()]
        for a, b in ((3, 290), (3, 140), (40, 100), (200, 201), (200, 202)):
            S[0][b] = S[0][a]
        st.upload(bodies_of(nb, *S, precision))
        for sep2 in (0.0, SEP2, INF):
            lst, info = check(st, S, sep2, "coincident, sep2 %g" % sep2)
            assert info["coincident"] == 3 + 1 + 3 and 2 * info["coincident"] == st.diagnostics()["coincident_pairs"]
            assert not ((S[0][lst["i"]] == S[0][lst["j"]]).all(axis=1)).any()
        # all velocities zero: w = 0, every near pair with 0 < mu (and a finite k) is bound
        Z = np.zeros_like(V)
        st.upload(bodies_of(nb, P, Z, M, R, precision))
        lst, info = check(st, (P, Z, M, R), SEP2, "at rest")
        assert info["pairs"] == info["near"] == binfo["near"] and info["approaching"] == 0 and (lst["ecc"] == 1.0).all()
        # all masses at the fp32 maximum: mu = 9.1e28, k = 8.3e57 is finite in fp64: every near pair is bound
        H = np.full(n, float(np.finfo(np.float32).max))
        st.upload(bodies_of(nb, P, V, H, R, precision))
        lst, info = check(st, (P, V, H, R), SEP2, "fp32 maximum masses")
        assert info["pairs"] == info["near"] == binfo["near"]
        if precision == 1:                                          # fp32 cannot hold them
            Ph, Vh, Mh = P.copy(), V.copy(), M.copy()
            Ph[5], Vh[7], Mh[9] = [1e200, 3.0], [1e200, -1e200], 1e200   # d2 = +inf; v2 = +inf; k = +inf
            st.upload(bodies_of(nb, Ph, Vh, Mh, R, precision))
            for sep2 in (SEP2, INF):
                lst, info = check(st, (Ph, Vh, Mh, R), sep2, "1e200, sep2 %g" % sep2)
                assert not np.isin(lst["i"], (5, 7, 9)).any() and not np.isin(lst["j"], (5, 7, 9)).any()
            assert info["near"] == n * (n - 1) // 2                 # sep2 = +inf: d2 = +inf is near, and never bound


# ---------------------------------------------------------------------------------------------------------------------
# 3. cross-checks against the other read-outs
# ---------------------------------------------------------------------------------------------------------------------
def test_cross_checks(nb):
    n = 1500
    P, V, M, R = (a.copy() for a in bc.standard_state(n, np.float32))
    P[10] = P[11] = P[900]                                          # three coincident pairs
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, P, V, M, R, 0))
        lst, info = check(st, (P, V, M, R), SEP2, "n 1500")
        assert info["coincident"] == 3 and 2 * info["coincident"] == st.diagnostics()["coincident_pairs"]
        pc = st.pair_counts([0.0, np.nextafter(SEP2, INF)], squared=True)
        assert info["near"] + info["coincident"] == int(pc["counts"][0]) and pc["below"] == 0
        # OVERLAP: the neighbour query's predicate on the bound pairs
        i, j = lst["i"].astype(np.int64), lst["j"].astype(np.int64)
        dx, dy = P[j, 0] - P[i, 0], P[j, 1] - P[i, 1]
        s = R[i] + R[j]
        over = ((dx * dx) + (dy * dy)) <= s * s
        assert np.array_equal((lst["flags"] & bc.OVERLAP) != 0, over) and info["overlapping"] == int(over.sum()) >= 3
        half_overlaps = int(st.neighbors()["overlaps"].sum()) // 2
        all_lst, all_info = check(st, (P, V, M, R), INF, "n 1500, sep2 inf")
        assert info["overlapping"] <= all_info["overlapping"] <= half_overlaps
        assert all_info["near"] == n * (n - 1) // 2 - 3


# ---------------------------------------------------------------------------------------------------------------------
# 4. capacity
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity(nb):
    n = 300
    state, (want, winfo) = standard(n, 0, SEP2)
    pairs = winfo["pairs"]
    counts = tuple(winfo[f] for f in bc.COUNTS) + (SEP2,)
    call = nb.lib.nbody_get_binaries
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, *state, 0))
        out = np.frombuffer(bytes([0x77]) * (48 * (pairs + 4)), dtype=bc.RECORD_DTYPE).copy()
        before = out.tobytes()
        info = np.full(1, -7, dtype=bc.INFO_DTYPE)
        assert call(st._ctx, SEP2, out.ctypes.data, pairs - 1, info.ctypes.data) == CAPACITY_ERR
        assert out.tobytes() == before and tuple(info[0]) == counts   # out untouched, info complete
        info[:] = -7
        assert call(st._ctx, SEP2, None, 0, info.ctypes.data) == 0  # the counts only
        assert tuple(info[0]) == counts
        info[:] = -7
        assert call(st._ctx, SEP2, out.ctypes.data, pairs, info.ctypes.data) == 0
        assert tuple(info[0]) == counts
        assert out[pairs:].tobytes() == before[48 * pairs:] and (out["reserved"][:pairs] == 0).all()
        for f in ("i", "j", "flags"):
            assert np.array_equal(out[f][:pairs], want[f])
        for f in bc.ORBIT:
            assert np.array_equal(out[f][:pairs].view(np.uint64), want[f].view(np.uint64))
        # the wrapper: a guess that is too small is repeated once with info.pairs; a smaller log after a larger one
        bc.assert_same(st.binaries(bc.SEP, cap=3 * n), (want, winfo), "cap 3 n")
        bc.assert_same(st.binaries(bc.SEP, cap=1), (want, winfo), "cap 1")
        bc.assert_same(st.binaries(bc.SEP, cap=0), (want, winfo), "cap 0")
        bc.assert_same(st.binaries(INF, cap=7), standard(n, 0, INF)[1], "sep inf, cap 7")
        bc.assert_same(st.binaries(SEP2, squared=True, cap=pairs), (want, winfo), "exact cap after a larger log")


# ---------------------------------------------------------------------------------------------------------------------
# 5. after steps, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1500])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics, n):
    cfg, b = dense_bodies(nb, n, seed=7003)
    _, V, M, _ = bc.standard_state(n, np.float32)
    b.Velocities[:] = V                                             # the stock generator leaves every body at rest
    b.Masses[:] = M                                                 # and its masses bind no pair at these speeds

    def run(with_calls):
        seen = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            st.set_tracers(np.array([[10.0, 20.0], [300.0, -40.0]]))
            for s in range(4):
                if s:
                    st.step(1)
                if with_calls:
                    state = bc.widen(st.download())
                    # the stock radii are 50 to 200: at 400 the dense state has some 100 bound of 2300 near pairs
                    got = check(st, state, 400.0 ** 2, "n0 %d after %d steps" % (n, s))
                    check(st, state, SEP2, "n0 %d after %d steps, SEP" % (n, s))
                    seen.append(got[1])
            d = st.download()
            tr = st.tracers()
            end = (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                   np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes(), tr["pos"].tobytes(), tr["vel"].tobytes())
        return end, seen
    plain, _ = run(False)
    called, seen = run(True)
    print("n0 %d: %s" % (n, seen))
    assert plain == called                                          # state, count, pair counter, events, tracers
    assert seen[0]["n_bodies"] == n and seen[-1]["n_bodies"] == plain[0] < n
    assert seen[0]["pairs"] > 0 and seen[0]["near"] > seen[0]["pairs"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. a ring-kernel context
# ---------------------------------------------------------------------------------------------------------------------
def test_ring_kernel_context(nb):
    n = 8269                                                        # ragged: 64 tiles and 77 bodies
    cfg = nb.stock_config(particleCount=n, fieldWidth=12000, fieldHeight=12000)
    b = nb.init_bodies(cfg)
    b.Velocities[:] = bc.standard_state(n, np.float32)[1]
    with nb.Stepper(cfg) as st:
        assert "ring" in st.force_kernel_name()
        st.upload(b)
        got = st.binaries(bc.SEP)                                   # 65 tiles, 33 workgroups
        print("ring context at upload: %s" % (got[1],))
        bc.assert_same(got, bc.window_binaries(*bc.widen(b), bc.SEP), "ring kernel context at upload")
        assert got[1]["n_bodies"] == n and got[1]["near"] > 0
        st.step(2)
        state = bc.widen(st.download())
        got = st.binaries(bc.SEP)
        print("ring context after 2 steps: %s" % (got[1],))
        bc.assert_same(got, bc.window_binaries(*state, bc.SEP), "ring kernel context after 2 steps")
        assert got[1]["n_bodies"] == len(state[2]) <= n


# ---------------------------------------------------------------------------------------------------------------------
# 7. above 2^16 bodies and 2^32 pairs
# ---------------------------------------------------------------------------------------------------------------------
def test_above_2_32_pairs(nb):
    n = 92683
    total = n * (n - 1) // 2
    assert total > 2 ** 32
    P, _, M, R = bc.standard_state(n, np.float32)
    V = np.random.default_rng(n + 1).uniform(-4000.0, 4000.0, size=(n, 2)).astype(np.float32).astype(np.float64)   # bound pairs are rare
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, P, V, M, R, 0))
        st.binaries(0.0, cap=0)                                     # the first call allocates
        t0 = time.perf_counter()
        lst, info = st.binaries(INF, cap=0)
        t1 = time.perf_counter()
        got = st.binaries(bc.SEP, cap=4096)
        t2 = time.perf_counter()
        print("n %d: sep2 inf %.1f ms (two walks: the counts, then the list) %s; SEP %.1f ms %s"
              % (n, (t1 - t0) * 1e3, info, (t2 - t1) * 1e3, got[1]))
        assert info["near"] == total - info["coincident"] and info["pairs"] <= info["near"] and info["pairs"] == len(lst)
        bc.assert_same(got, bc.window_binaries(P, V, M, R, bc.SEP), "n %d at SEP" % n)
        assert got[1]["near"] > n and got[1]["pairs"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    state, (want, winfo) = standard(300, 0, SEP2)
    call, bcall = nb.lib.nbody_get_binaries, nb.lib.nbody_batch_get_binaries
    out = np.frombuffer(bytes([0x77]) * (48 * 512), dtype=bc.RECORD_DTYPE).copy()
    info = np.full(2, -7, dtype=bc.INFO_DTYPE)
    untouched = (out.tobytes(), info.tobytes())
    O, I = out.ctypes.data, info.ctypes.data

    def bad_arguments(fn, handle, systems):
        assert fn(None, SEP2, O, 512, I) == INVALID
        assert fn(handle, SEP2, O, 512, None) == INVALID
        for sep2 in (float("nan"), -1.0, -0.5, -INF):
            assert fn(handle, sep2, O, 512, I) == INVALID and b"sep2" in nb.lib.nbody_last_error_string()
        assert fn(handle, SEP2, O, -1, I) == INVALID
        assert fn(handle, SEP2, None, 4, I) == INVALID
        assert fn(handle, SEP2, O, (1 << 31) // (48 * systems) + 1, I) == INVALID     # cap x 48 bytes (x systems) above 2^31
        assert (out.tobytes(), info.tobytes()) == untouched

    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, SEP2, O, 512, I) == STATE_ERR and b"before" in nb.lib.nbody_last_error_string()
        bad_arguments(call, st._ctx, 1)                             # refused before the state is looked at
        st.upload(bodies_of(nb, *state, 0))
        bad_arguments(call, st._ctx, 1)
        bc.assert_same(st.binaries(bc.SEP), (want, winfo), "after the refusals")
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 1000000, 1000000)] * 2) as batch:
        assert bcall(batch._b, SEP2, O, 256, I) == STATE_ERR
        bad_arguments(bcall, batch._b, 2)
        batch.upload([bodies_of(nb, *state, 0), nb.BodiesData(0)])
        bad_arguments(bcall, batch._b, 2)
        got = batch.binaries(bc.SEP)
        bc.assert_same(got[0], (want, winfo), "batch after the refusals")
        assert len(got[1][0]) == 0 and [got[1][1][f] for f in bc.COUNTS] == [0] * 6
    grp = nb.StepperGroup(2, capacity=300, timestep=0.2, growthRate=0.1, fieldWidth=1000000, fieldHeight=1000000)
    grp.upload(bodies_of(nb, *state, 0))
    for r in grp.ranks:                                             # a rank holds only its own velocities
        assert call(r._ctx, SEP2, O, 512, I) == STATE_ERR and b"single-rank" in nb.lib.nbody_last_error_string()
    assert (out.tobytes(), info.tobytes()) == untouched
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_and_model(nb, semantics):
    cap, counts = 1024, (0, 1, 64, 129, 1024)
    S = len(counts)
    params = [(0.2, 0.1, 3000, 3000), (0.1, 0.0, 3000, 3000), (0.3, 0.2, 2000, 2500), (0.2, 0.1, 4000, 4000), (0.25, 0.1, 6000, 6000)]
    bodies = [bodies_of(nb, *bc.standard_state(k, np.float32, seed=100 + s), 0) if k else nb.BodiesData(0) for s, k in enumerate(counts)]
    sep = 12.5
    with nb.StepperBatch(S, cap, params=params, semantics=semantics) as batch:
        batch.upload(bodies)
        for steps in (0, 3):
            if steps:
                batch.step(steps)
            got = batch.binaries(sep)
            assert len(got) == S
            worst = 0
            for s in range(S):
                d = batch.download(s)
                what = "system %d (n %d) after %d steps" % (s, d.numBodies, steps)
                bc.assert_same(got[s], bc.model_binaries(*bc.widen(d), sep * sep), what + ": model")
                p = params[s]
                with nb.Stepper(capacity=cap, semantics=semantics, timestep=p[0], growthRate=p[1], fieldWidth=p[2], fieldHeight=p[3]) as one:
                    one.upload(d)
                    bc.assert_same(got[s], one.binaries(sep), what + ": Stepper")
                worst = max(worst, got[s][1]["pairs"])
            print("after %d steps: %s" % (steps, [g[1] for g in got]))
            assert got[0][1]["pairs"] == got[1][1]["pairs"] == 0 and got[3][1]["n_bodies"] <= 129
            assert steps or (got[4][1]["pairs"] > 100 and got[3][1]["pairs"] > 10 and got[2][1]["pairs"] > 5)
            worst = max(worst, 2)
            # the C call: the tails of out past each system's pairs stay untouched; one system over cap fails the whole call
            out = np.frombuffer(bytes([0x77]) * (48 * S * worst), dtype=bc.RECORD_DTYPE).copy().reshape(S, worst)
            info = np.full(S, -7, dtype=bc.INFO_DTYPE)
            assert nb.lib.nbody_batch_get_binaries(batch._b, sep * sep, out.ctypes.data, worst, info.ctypes.data) == 0
            for s in range(S):
                k = got[s][1]["pairs"]
                assert tuple(info[s])[:6] == tuple(got[s][1][f] for f in bc.COUNTS) and info["sep2"][s] == sep * sep
                assert np.array_equal(out["a"][s, :k].view(np.uint64), got[s][0]["a"].view(np.uint64)) and np.array_equal(out["j"][s, :k], got[s][0]["j"])
                assert out[s, k:].tobytes() == bytes([0x77]) * (48 * (worst - k))
            if max(g[1]["pairs"] for g in got) == worst:
                out[:] = np.frombuffer(bytes([0x77]) * 48, dtype=bc.RECORD_DTYPE)[0]
                info[:] = -7
                assert nb.lib.nbody_batch_get_binaries(batch._b, sep * sep, out.ctypes.data, worst - 1, info.ctypes.data) == CAPACITY_ERR
                assert out.tobytes() == bytes([0x77]) * (48 * S * worst)
                assert [tuple(info[s])[:6] for s in range(S)] == [tuple(got[s][1][f] for f in bc.COUNTS) for s in range(S)]


def test_batch_of_many_small_systems(nb):
    # 1024 systems of one wave's rows; then 64 systems on both sides of a wave (63, 65) and of a tile (127, 129) in one batch
    for S, sizes in ((1024, [64]), (64, [63, 65, 127, 129])):
        cfg = nb.stock_config(particleCount=max(sizes), fieldWidth=600, fieldHeight=600)
        states = [bc.standard_state(sizes[s % len(sizes)], np.float32, seed=5000 + s) for s in range(S)]
        with nb.StepperBatch(S, max(sizes), cfg=cfg) as batch:
            batch.upload([bodies_of(nb, *state, 0) for state in states])
            got = batch.binaries(bc.SEP)
            total = dict.fromkeys(bc.COUNTS[1:], 0)
            for s in range(S):
                bc.assert_same(got[s], bc.model_binaries(*states[s], SEP2), "system %d of %d" % (s, S))
                for f in total:
                    total[f] += got[s][1][f]
            print("%d x %s: %s" % (S, sizes, total))
            again = batch.binaries(bc.SEP, cap=0)                   # the counts first (no slot is taken), then the lists
            for s in range(0, S, 37):
                bc.assert_same(again[s], got[s], "system %d of %d, cap 0" % (s, S))
            assert total["pairs"] > 16 * S and total["near"] - total["pairs"] > 16 * S and total["overlapping"] > S and total["approaching"] > 4 * S
