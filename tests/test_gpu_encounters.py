"""Encounter queries (nbody_get_encounters, nbody_batch_get_encounters; Stepper.encounters, StepperBatch.encounters) on the
MI355X: the swept contacts of the resident state within a horizon.

The definition has no fma and rounds every operation on its own; the device decides which pairs are swept with subtractions,
multiplies, additions and compares, the host computes t with the C library's sqrt and division.  The numpy model of
encounter_cases.py restates every bit: zero tolerance throughout - t by bits, i, j, flags and every field of info."""
import functools

import numpy as np
import pytest

import encounter_cases as ec
from lineage_cases import dense_bodies

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
INF = float("inf")
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


def small_stepper(nb, precision, capacity, **kw):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=1000000,
                      fieldHeight=1000000, **kw)


def bodies_of(nb, P, V, R, precision, M=None):
    n = len(R)
    return nb.BodiesData.from_arrays(P, V, np.ones(n) if M is None else M, R, precision) if n else nb.BodiesData(0, precision)


@functools.lru_cache(maxsize=None)
def standard(n, precision, h):
    """The standard state and its model at horizon h, computed once."""
    P, V, R = ec.standard_state(n, ec.DTYPE_OF[precision])
    return (P, V, R), ec.model_encounters(P, V, R, h)


def check(st, state, h, what):
    """encounters() of the resident state against the model of `state`; -> the result."""
    got = st.encounters(h)
    ec.assert_same(got, ec.model_encounters(*state, h), what)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile, wave and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    with small_stepper(nb, precision, n) as st:
        state, _ = standard(n, precision, ec.H)
        st.upload(bodies_of(nb, *state, precision))
        for h in (0.0, ec.H, INF):
            _, want = standard(n, precision, h)
            got = st.encounters(h)
            print("n %d h %g: %s" % (n, h, got[1]))
            ec.assert_same(got, want, "n %d h %g" % (n, h))
            if n >= 63 and h == ec.H:
                assert min(ec.classes(got[0])) >= 3                # every class is there to be got wrong
        enc0, info0 = st.encounters(0.0)                            # h = 0: swept == now, half the sum of the overlaps
        assert info0["pairs"] == info0["now"] == info0["end"] and 2 * info0["now"] == int(st.neighbors()["overlaps"].sum())
        # symmetry: the body order reversed, the indices mapped back: the same set with the same t bits
        P, V, R = state
        st.upload(bodies_of(nb, P[::-1], V[::-1], R[::-1], precision))
        for h in (ec.H, INF):
            enc, info = st.encounters(h)
            ec.assert_same((ec.reversed_back(enc, n), info), standard(n, precision, h)[1], "n %d h %g reversed" % (n, h))


# ---------------------------------------------------------------------------------------------------------------------
# 2. special states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_special_states(nb, precision):
    n = 129
    (P, V, R), (base, _) = standard(n, precision, ec.H)

    def without(enc, body):
        return enc[(enc["i"] != body) & (enc["j"] != body)]

    with small_stepper(nb, precision, 140) as st:
        # coincident bodies: d2 = +0, NOW whatever they do; moving apart END goes once they have separated
        C = np.array([[3.0, 4.0], [50.0, 50.0], [3.0, 4.0], [3.0, 4.0]])
        R4 = np.full(4, 0.25)
        for VC, what in ((np.zeros((4, 2)), "at rest"), (np.array([[8.0, 0.0], [0.0, 0.0], [-8.0, 0.0], [0.0, 8.0]]), "moving apart")):
            st.upload(bodies_of(nb, C, VC, R4, precision))
            for h in (0.0, 0.01, ec.H, INF):
                enc, info = check(st, (C, VC, R4), h, "coincident, %s, h %g" % (what, h))
                assert info["pairs"] == info["now"] == 3 and (enc["t"] == 0.0).all()
                assert info["end"] == (3 if h <= 0.01 or (what == "at rest" and h < INF) else 0)
        # all velocities zero: swept == now
        Z = np.zeros_like(V)
        st.upload(bodies_of(nb, P, Z, R, precision))
        for h in (ec.H, 1e6):
            enc, info = check(st, (P, Z, R), h, "at rest, h %g" % h)
            assert info["pairs"] == info["now"] == info["end"] >= 3 and info["missed"] == 0
        # a NaN coordinate or radius removes exactly that body's pairs
        k = int(base["i"][base["flags"] == 0][0])                   # a body of a missed pair ...
        assert not (((base["i"] == k) | (base["j"] == k)) & ((base["flags"] & ec.NOW) != 0)).any()   # ... that overlaps nobody
        for which, what in ((0, "coordinate"), (2, "radius")):
            S = [P.copy(), V.copy(), R.copy()]
            if which == 0:
                S[0][k, 1] = np.nan
            else:
                S[2][k] = np.nan
            st.upload(bodies_of(nb, *S, precision))
            enc, info = check(st, S, ec.H, "NaN " + what)
            assert np.array_equal(enc, without(base, k)) and len(enc) < len(base)
        # a NaN velocity: end and mid fail; `now` does not read it, and this body overlaps nobody: exactly its pairs go
        S = [P.copy(), V.copy(), R.copy()]
        S[1][k, 0] = np.nan
        st.upload(bodies_of(nb, *S, precision))
        enc, info = check(st, S, ec.H, "NaN velocity")
        assert np.array_equal(enc, without(base, k))
        o = int(base["i"][(base["flags"] & ec.NOW) != 0][0])        # ... and one that overlaps keeps its NOW pairs, t = +0
        S = [P.copy(), V.copy(), R.copy()]
        S[1][o] = np.nan
        st.upload(bodies_of(nb, *S, precision))
        enc, info = check(st, S, ec.H, "NaN velocity of an overlapping body")
        mine = enc[(enc["i"] == o) | (enc["j"] == o)]
        assert len(mine) >= 1 and ((mine["flags"] & ec.NOW) != 0).all() and (mine["t"] == 0.0).all()
        # a NaN mass changes nothing
        M = np.ones(n)
        M[k] = np.nan
        st.upload(bodies_of(nb, P, V, R, precision, M))
        ec.assert_same(st.encounters(ec.H), standard(n, precision, ec.H)[1], "NaN mass")
        if precision == 1:                                          # fp32 cannot hold it
            Ph, Vh = P.copy(), V.copy()
            Ph[5], Vh[7] = [1e200, 3.0], [1e200, -1e200]
            st.upload(bodies_of(nb, Ph, Vh, R, precision))
            for h in (0.0, ec.H, INF):
                enc, _ = check(st, (Ph, Vh, R), h, "1e200, h %g" % h)
                assert not ((enc["i"] == 5) | (enc["j"] == 5)).any()
            Pe, Ve = np.array([[0.0, 0.0], [1e200, 0.0]]), np.array([[0.0, 0.0], [-1e200, 0.0]])
            st.upload(bodies_of(nb, Pe, Ve, np.ones(2), precision))
            enc, info = check(st, (Pe, Ve, np.ones(2)), 1.0, "1e200 and back")
            assert info["pairs"] == info["end"] == 1 and enc["t"][0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. capacity
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity(nb):
    n = 300
    state, (want, winfo) = standard(n, 0, ec.H)
    pairs = winfo["pairs"]
    call = nb.lib.nbody_get_encounters
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, *state, 0))
        out = np.frombuffer(bytes([0x77]) * (24 * (pairs + 4)), dtype=ec.RECORD_DTYPE).copy()
        before = out.tobytes()
        info = np.full(1, -7, dtype=ec.INFO_DTYPE)
        assert call(st._ctx, ec.H, out.ctypes.data, pairs - 1, info.ctypes.data) == CAPACITY_ERR
        assert out.tobytes() == before                              # out untouched, info complete
        assert tuple(info[0]) == (n, pairs, winfo["now"], winfo["end"], winfo["missed"], ec.H)
        info[:] = -7
        assert call(st._ctx, ec.H, None, 0, info.ctypes.data) == 0  # the counts only
        assert tuple(info[0]) == (n, pairs, winfo["now"], winfo["end"], winfo["missed"], ec.H)
        info[:] = -7
        assert call(st._ctx, ec.H, out.ctypes.data, pairs, info.ctypes.data) == 0
        assert tuple(info[0]) == (n, pairs, winfo["now"], winfo["end"], winfo["missed"], ec.H)
        assert out[pairs:].tobytes() == before[24 * pairs:] and (out["reserved"][:pairs] == 0).all()
        for f in ("i", "j", "flags"):
            assert np.array_equal(out[f][:pairs], want[f])
        assert np.array_equal(out["t"][:pairs].view(np.uint64), want["t"].view(np.uint64))
        # the wrapper: a guess that is too small is repeated once with info.pairs; a smaller log after a larger one
        ec.assert_same(st.encounters(ec.H, cap=1), (want, winfo), "cap 1")
        ec.assert_same(st.encounters(ec.H, cap=0), (want, winfo), "cap 0")
        ec.assert_same(st.encounters(INF, cap=7), standard(n, 0, INF)[1], "h inf, cap 7")
        ec.assert_same(st.encounters(ec.H, cap=3 * n), (want, winfo), "cap 3 n")
        fc = nb.first_contacts(want, n)
        assert np.array_equal(fc["t"], ec.first_contacts(want, n)["t"]) and fc["count"].sum() == 2 * pairs


# ---------------------------------------------------------------------------------------------------------------------
# 4. after steps, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1500])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics, n):
    cfg, b = dense_bodies(nb, n, seed=7003)
    b.Velocities[:] = ec.standard_state(n, np.float32)[1]           # the stock generator leaves every body at rest
    dt = float(np.float32(cfg.timestep))

    def run(with_calls):
        seen = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            st.set_tracers(np.array([[10.0, 20.0], [300.0, -40.0]]))
            for s in range(4):
                if s:
                    st.step(1)
                if with_calls:
                    state = ec.widen(st.download())
                    got = st.encounters()                           # horizon=None: the context's own time step
                    assert got[1]["horizon"] == dt
                    ec.assert_same(got, ec.model_encounters(*state, dt), "n0 %d after %d steps" % (n, s))
                    ec.assert_same(st.encounters(5.0), ec.model_encounters(*state, 5.0), "n0 %d after %d steps, h 5" % (n, s))
                    seen.append(got[1])
            d = st.download()
            tr = st.tracers()
            end = (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                   np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes(), tr["pos"].tobytes(), tr["vel"].tobytes())
        return end, seen
    plain, _ = run(False)
    called, seen = run(True)
    assert plain == called                                          # state, count, pair counter, events, tracers
    assert seen[0]["n_bodies"] == n and seen[-1]["n_bodies"] == plain[0] < n
    assert all(i["now"] > 0 and i["pairs"] > i["now"] for i in seen[:1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. a ring-kernel context
# ---------------------------------------------------------------------------------------------------------------------
def test_ring_kernel_context(nb):
    n = 8269                                                        # ragged: 64 tiles and 77 bodies
    cfg = nb.stock_config(particleCount=n, fieldWidth=12000, fieldHeight=12000)
    b = nb.init_bodies(cfg)
    b.Velocities[:] = ec.standard_state(n, np.float32)[1]
    with nb.Stepper(cfg) as st:
        assert "ring" in st.force_kernel_name()
        st.upload(b)
        dt = float(np.float32(cfg.timestep))
        got = st.encounters()                                       # 65 tiles, 33 workgroups; the model's 34 M pairs in chunks: 2 s
        print("ring context at upload: %s" % (got[1],))
        ec.assert_same(got, ec.model_encounters(*ec.widen(b), dt), "ring kernel context at upload")
        assert got[1]["n_bodies"] == n and got[1]["pairs"] > n
        st.step(2)                                                  # the stock radii in this field: most bodies have merged by now
        state = ec.widen(st.download())
        got = st.encounters()
        print("ring context after 2 steps: %s" % (got[1],))
        ec.assert_same(got, ec.model_encounters(*state, dt), "ring kernel context after 2 steps")
        assert got[1]["n_bodies"] == len(state[2]) <= n and got[1]["pairs"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    state, (want, winfo) = standard(300, 0, ec.H)
    call, bcall = nb.lib.nbody_get_encounters, nb.lib.nbody_batch_get_encounters
    out = np.frombuffer(bytes([0x77]) * (24 * 512), dtype=ec.RECORD_DTYPE).copy()
    info = np.full(2, -7, dtype=ec.INFO_DTYPE)
    untouched = (out.tobytes(), info.tobytes())
    O, I = out.ctypes.data, info.ctypes.data

    def bad_arguments(fn, handle, systems):
        assert fn(None, ec.H, O, 512, I) == INVALID
        assert fn(handle, ec.H, O, 512, None) == INVALID
        for h in (float("nan"), -1.0, -0.5, -INF):
            assert fn(handle, h, O, 512, I) == INVALID and b"horizon" in nb.lib.nbody_last_error_string()
        assert fn(handle, ec.H, O, -1, I) == INVALID
        assert fn(handle, ec.H, None, 4, I) == INVALID
        assert fn(handle, ec.H, O, (1 << 31) // (24 * systems) + 1, I) == INVALID     # cap x 24 bytes (x systems) above 2^31
        assert (out.tobytes(), info.tobytes()) == untouched

    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, ec.H, O, 512, I) == STATE_ERR and b"before" in nb.lib.nbody_last_error_string()
        bad_arguments(call, st._ctx, 1)                             # refused before the state is looked at
        st.upload(bodies_of(nb, *state, 0))
        bad_arguments(call, st._ctx, 1)
        ec.assert_same(st.encounters(ec.H), (want, winfo), "after the refusals")
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 1000000, 1000000)] * 2) as batch:
        assert bcall(batch._b, ec.H, O, 256, I) == STATE_ERR
        batch.upload([bodies_of(nb, *state, 0), nb.BodiesData(0)])
        bad_arguments(bcall, batch._b, 2)
        got = batch.encounters(ec.H)
        ec.assert_same(got[0], (want, winfo), "batch after the refusals")
        assert len(got[1][0]) == 0 and [got[1][1][f] for f in ec.COUNTS] == [0] * 5
    grp = nb.StepperGroup(2, capacity=300, timestep=0.2, growthRate=0.1, fieldWidth=1000000, fieldHeight=1000000)
    grp.upload(bodies_of(nb, *state, 0))
    for r in grp.ranks:                                             # a rank holds only its own velocities
        assert call(r._ctx, ec.H, O, 512, I) == STATE_ERR and b"single-rank" in nb.lib.nbody_last_error_string()
    assert (out.tobytes(), info.tobytes()) == untouched
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_and_model(nb, semantics):
    cap, counts = 1024, (0, 1, 64, 129, 1024)
    S = len(counts)
    params = [(0.2, 0.1, 3000, 3000), (0.1, 0.0, 3000, 3000), (0.3, 0.2, 2000, 2500), (0.2, 0.1, 4000, 4000), (0.25, 0.1, 6000, 6000)]
    bodies = []
    for s, k in enumerate(counts):
        if not k:
            bodies.append(nb.BodiesData(0))
            continue
        if k == 1024:                                               # the stock generator's radii: nearly every swept pair overlaps now
            b = nb.init_bodies(nb.stock_config(particleCount=k, fieldWidth=params[s][2], fieldHeight=params[s][3]), seed=60 + s)
            b.Velocities[:] = ec.standard_state(k, np.float32, seed=100 + s)[1]
        else:                                                       # the standard state: every class
            b = bodies_of(nb, *ec.standard_state(k, np.float32, seed=100 + s), 0)
        bodies.append(b)
    h = 0.75
    with nb.StepperBatch(S, cap, params=params, semantics=semantics) as batch:
        batch.upload(bodies)
        for steps in (0, 3):
            if steps:
                batch.step(steps)
            got = batch.encounters(h)
            assert len(got) == S
            worst = 0
            for s in range(S):
                d = batch.download(s)
                what = "system %d (n %d) after %d steps" % (s, d.numBodies, steps)
                ec.assert_same(got[s], ec.model_encounters(*ec.widen(d), h), what + ": model")
                p = params[s]
                with nb.Stepper(capacity=cap, semantics=semantics, timestep=p[0], growthRate=p[1], fieldWidth=p[2], fieldHeight=p[3]) as one:
                    one.upload(d)
                    ec.assert_same(got[s], one.encounters(h), what + ": Stepper")
                worst = max(worst, got[s][1]["pairs"])
            assert got[0][1]["pairs"] == got[1][1]["pairs"] == 0 and got[4][1]["pairs"] > 0 and got[3][1]["n_bodies"] <= 129
            assert steps or min(ec.classes(got[3][0])) >= 1
            # the C call: the tails of out past each system's pairs stay untouched; one system over cap fails the whole call
            out = np.frombuffer(bytes([0x77]) * (24 * S * worst), dtype=ec.RECORD_DTYPE).copy().reshape(S, worst)
            info = np.full(S, -7, dtype=ec.INFO_DTYPE)
            assert nb.lib.nbody_batch_get_encounters(batch._b, h, out.ctypes.data, worst, info.ctypes.data) == 0
            for s in range(S):
                k = got[s][1]["pairs"]
                assert tuple(info[s])[:5] == tuple(got[s][1][f] for f in ec.COUNTS) and info["horizon"][s] == h
                assert np.array_equal(out["t"][s, :k].view(np.uint64), got[s][0]["t"].view(np.uint64)) and np.array_equal(out["j"][s, :k], got[s][0]["j"])
                assert out[s, k:].tobytes() == bytes([0x77]) * (24 * (worst - k))
            out[:] = np.frombuffer(bytes([0x77]) * 24, dtype=ec.RECORD_DTYPE)[0]
            info[:] = -7
            assert nb.lib.nbody_batch_get_encounters(batch._b, h, out.ctypes.data, worst - 1, info.ctypes.data) == CAPACITY_ERR
            assert out.tobytes() == bytes([0x77]) * (24 * S * worst)
            assert [tuple(info[s])[:5] for s in range(S)] == [tuple(got[s][1][f] for f in ec.COUNTS) for s in range(S)]


def test_batch_of_many_small_systems(nb):
    # 1024 systems of one wave's rows; then 64 systems on both sides of a wave (63, 65) and of a tile (127, 129) in one batch
    for S, sizes in ((1024, [64]), (64, [63, 65, 127, 129])):
        cfg = nb.stock_config(particleCount=max(sizes), fieldWidth=600, fieldHeight=600)
        bodies = [bodies_of(nb, *ec.standard_state(sizes[s % len(sizes)], np.float32, seed=5000 + s), 0) for s in range(S)]
        with nb.StepperBatch(S, max(sizes), cfg=cfg) as batch:
            batch.upload(bodies)
            got = batch.encounters(ec.H)
            total = [0, 0, 0]
            for s in range(S):
                ec.assert_same(got[s], ec.model_encounters(*ec.widen(bodies[s]), ec.H), "system %d of %d" % (s, S))
                total = [a + b for a, b in zip(total, ec.classes(got[s][0]))]
            print("%d x %s: now %d, end only %d, missed %d" % (S, sizes, *total))
            assert min(total) > S
