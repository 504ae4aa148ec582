"""Tracer particles (nbody_tracers_*, nbody_batch_tracers_*; Stepper.set_tracers / tracers, StepperBatch likewise) on the
MI355X.  All comparisons are bit for bit unless said otherwise: the field of an advance against the library's own
nbody_get_field on a twin without tracers, the update against the numpy restatement tracer_cases.advance, a batch against
one Stepper per system.  The accuracy of the field itself is field_cases.py's, with its derived bounds."""
import ctypes

import numpy as np
import pytest

import field_cases as fc
import tracer_cases as tc
from test_gpu_batch import params_of
from test_gpu_diagnostics import state_arrays

pytestmark = pytest.mark.gpu

INVALID, STATE_ERR = -1, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
SEMANTICS = [pytest.param(0, id="literal"), pytest.param(1, id="clean")]
M_SIZES = (1, 64, 65, 257, 600)


def setup_module(module):
    fc.require_long_double()


def assert_bits(got, want, what):
    assert np.shape(got) == np.shape(want), (what, np.shape(got), np.shape(want))
    bad = np.argwhere(tc.bits(got) != tc.bits(want))
    assert len(bad) == 0, (what, "%d values differ, first at %s" % (len(bad), bad[:4].tolist()))


def assert_same_bodies(a, b, what):
    da, db = a.download(), b.download()
    assert da.numBodies == db.numBodies, what
    assert np.array_equal(np.ascontiguousarray(da.block).view(np.uint8), np.ascontiguousarray(db.block).view(np.uint8)), what


def checked_step(nb, st, twin, cfg, precision, walls, want_steps, coin, what):
    """One step of `st` (with tracers) beside `twin` (without): the field of the advance is the twin's field at the tracers'
    positions, the update is the model's.  -> the coincident sources of the advance."""
    before = st.tracers()
    f = twin.field(before["pos"])
    st.step(1)
    twin.step(1)
    after = st.tracers()
    assert_bits(after["acc"], f["acc"], what + " acc")
    assert_bits(after["phi"], f["phi"], what + " phi")
    want = tc.advance(before, f["acc"], tc.dt_of(nb, cfg, precision), walls, (cfg.fieldWidth, cfg.fieldHeight))
    assert_bits(after["pos"], want["pos"], what + " pos")
    assert_bits(after["vel"], want["vel"], what + " vel")
    assert after["steps"] == want_steps and after["coincident"] == coin + f["coincident"], what
    return f["coincident"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. a chain of steps against the library's own field and the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [1, 127, 129, 300])
@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chain_against_field_and_model(nb, precision, semantics, n0):
    cfg, b = tc.dense_case(nb, n0, precision)
    kw = dict(precision=precision, semantics=semantics, record_events=True)
    shrank = False
    for m in M_SIZES:
        walls = m % 2 == 1
        pos, vel = tc.tracer_set(cfg, m, seed=m + n0)
        with nb.Stepper(cfg, **kw) as st, nb.Stepper(cfg, **kw) as twin:
            st.set_tracers(pos, vel, walls=walls)               # before the first upload
            st.upload(b)
            twin.upload(b)
            t0 = st.tracers()
            assert_bits(t0["pos"], pos, "set pos")
            assert_bits(t0["vel"], vel, "set vel")
            assert not tc.bits(t0["acc"]).any() and not tc.bits(t0["phi"]).any() and (t0["steps"], t0["coincident"]) == (0, 0)
            coin = 0
            for s in range(6):
                coin += checked_step(nb, st, twin, cfg, precision, walls, s + 1, coin,
                                     "n0 %d, m %d, step %d" % (n0, m, s))
            assert_same_bodies(st, twin, "n0 %d, m %d: the bodies" % (n0, m))   # the bodies never notice
            order = ("step", "i", "j", "kind")                  # the log's order is the atomics': the sets are compared
            assert np.array_equal(np.sort(st.events(), order=order), np.sort(twin.events(), order=order))
            shrank = shrank or st.body_count() < n0
    if n0 == 300:                                               # stock radii in the dense field: bodies have merged, so the
        assert shrank                                           # chain covers the count read from Meta


# ---------------------------------------------------------------------------------------------------------------------
# 2. step(5) once = 5 x step(1), over a count that changes inside those five steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bulk_enqueue_equals_single_steps(nb, precision):
    cfg, b = tc.dense_case(nb, 300, precision)
    pos, vel = tc.tracer_set(cfg, 257, seed=9)
    with nb.Stepper(cfg, precision=precision) as bulk, nb.Stepper(cfg, precision=precision) as single:
        counts = []
        for st in (bulk, single):
            st.upload(b)
            st.set_tracers(pos, vel, walls=True)
        bulk.step(5)
        for _ in range(5):
            single.step(1)
            counts.append(single.body_count())
        assert len(set(counts)) > 1 and counts[-1] < 300, counts  # the count changed inside the five steps
        tb, ts = bulk.tracers(), single.tracers()
        for k in ("pos", "vel", "acc", "phi"):
            assert_bits(tb[k], ts[k], k)
        assert tb["steps"] == ts["steps"] == 5 and tb["coincident"] == ts["coincident"]
        assert_same_bodies(bulk, single, "bodies")


# ---------------------------------------------------------------------------------------------------------------------
# 3. accuracy of "last" after one step: the long-double oracle and the derived bounds of field_cases.py
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_last_against_the_oracle(nb, precision):
    cfg, b = tc.dense_case(nb, 300, precision)
    pos, vel = tc.tracer_set(cfg, 257, seed=4)
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        st.step(2)
        P, _, M = state_arrays(st.download())                   # J_t of the advance to come
        st.set_tracers(pos, vel)
        st.step(1)
        t = st.tracers()
    acc, phi, mag, coin = fc.exact_field(P, M, points=pos)
    assert t["coincident"] == coin == 0 and t["steps"] == 1
    fc.check_field(t["acc"], t["phi"], acc, phi, mag, len(M), "last after one step, n %d" % len(M))


# ---------------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_edge_cases(nb, precision):
    cfg, b = tc.dense_case(nb, 129, precision)
    P, _, M = state_arrays(b)
    ordinary, ovel = tc.tracer_set(cfg, 70, seed=2)
    # 70: exactly on body 5 (the term is left out and counted); 71: so far out that d2 overflows (the general code);
    # 72, 73: NaN and infinite coordinates
    odd = np.array([P[5], [1e200, -3e199], [np.nan, 10.0], [np.inf, -np.inf]])
    pos, vel = np.concatenate([ordinary, odd]), np.concatenate([ovel, np.ones((4, 2))])
    kw = dict(precision=precision)
    with nb.Stepper(cfg, **kw) as st, nb.Stepper(cfg, **kw) as plain, nb.Stepper(cfg, **kw) as twin:
        for s in (st, plain, twin):
            s.upload(b)
        st.set_tracers(pos, vel)
        plain.set_tracers(ordinary, ovel)
        f = twin.field(pos[:72])
        assert f["coincident"] == 1
        acc, phi, mag, coin = fc.exact_field(P, M, points=pos[70:71])
        assert coin == 1
        fc.check_field(f["acc"][70:71], f["phi"][70:71], acc, phi, mag, len(M), "on a body")
        st.step(1)
        plain.step(1)
        t, tp = st.tracers(), plain.tracers()
        assert t["coincident"] == 1 and tp["coincident"] == 0
        assert_bits(t["acc"][:72], f["acc"], "acc")
        assert_bits(t["phi"][:72], f["phi"], "phi")
        assert np.isfinite(t["acc"][71]).all() and t["phi"][71] < 0   # the general code's sums: the chain's are NaN there
        want = tc.advance({"pos": pos[:72], "vel": vel[:72]}, f["acc"], tc.dt_of(nb, cfg, precision), False, (0, 0))
        assert_bits(t["pos"][:72], want["pos"], "pos")
        assert_bits(t["vel"][:72], want["vel"], "vel")
        st.step(3)
        plain.step(3)
        t, tp = st.tracers(), plain.tracers()
        for k in ("pos", "vel", "acc", "phi"):                  # the ordinary ones keep the bits they have without the others
            assert_bits(t[k][:70], tp[k], k)
            assert np.isfinite(tp[k]).all()
        assert np.isnan(t["pos"][72]).any() and not np.isfinite(t["pos"][73]).all()
        assert_same_bodies(st, plain, "bodies")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mirrored_tracers_stay_mirrored(nb, precision):
    body = nb.BodiesData.from_arrays([[0.0, 0.0]], [[0.0, 0.0]], [3.0e9], [0.0], precision)
    # no tracer on an axis through the source: a component that is exactly 0 is +0 on both sides (the sums start from +0)
    a = np.array([[3.25, -1.5], [0.7, 11.0], [40.0, 0.125]])
    v = np.array([[0.3, -0.2], [0.0, 1.0], [0.0, 0.05]])
    with nb.Stepper(capacity=4, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100) as st:
        st.upload(body)
        st.set_tracers(np.concatenate([a, -a]), np.concatenate([v, -v]), walls=True)
        for s in range(4):
            st.step(1)
            t = st.tracers()
            for k in ("pos", "vel", "acc"):
                assert_bits(t[k][:3], -t[k][3:], "%s after step %d" % (k, s))
            assert_bits(t["phi"][:3], t["phi"][3:], "phi after step %d" % s)
        assert (t["acc"][:3] != 0).any() and t["steps"] == 4 and t["coincident"] == 0
        assert st.body_count() == 1


# ---------------------------------------------------------------------------------------------------------------------
# 5. walls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_walls(nb, precision):
    W, dt = 1000, 0.25
    # one heavy body outside the +x wall pulls towards it: at the wall x + ax dt crosses fieldWidth, 100 inside it does not
    body = nb.BodiesData.from_arrays([[W + 10.0, 0.0]], [[0.0, 0.0]], [1.0e9], [0.0], precision)
    pos = np.array([[float(W), 0.0], [W - 100.0, 0.0], [W - 100.0, W + 1.0], [3.0, -5.0]])
    vel = np.array([[1.0, 2.0], [1.0, 2.0], [1.0, 2.0], [-1.0, 0.5]])
    out = {}
    for walls in (False, True):
        with nb.Stepper(capacity=4, precision=precision, timestep=dt, growthRate=0.1, fieldWidth=W, fieldHeight=W) as st:
            st.upload(body)
            f = st.field(pos)
            st.set_tracers(pos, vel, walls=walls)
            st.step(1)
            t = out[walls] = st.tracers()
            want = tc.advance({"pos": pos, "vel": vel}, f["acc"], dt, walls, (W, W))
            assert_bits(t["acc"], f["acc"], "acc")
            assert_bits(t["pos"], want["pos"], "pos, walls %s" % walls)
            assert_bits(t["vel"], want["vel"], "vel, walls %s" % walls)
    acc = out[True]["acc"]
    assert acc[0, 0] > 0 and W + acc[0, 0] * dt > W                                  # the model's test at the wall
    assert out[True]["vel"][0, 0] < 0 < out[False]["vel"][0, 0]                      # flipped with the flag only
    assert out[True]["vel"][2, 1] < 0 < out[False]["vel"][2, 1]                      # outside in y: flipped as well
    for k in (1, 3):                                                                 # inside: the flag changes nothing
        assert_bits(out[True]["vel"][k], out[False]["vel"][k], "tracer %d" % k)
    assert_bits(out[True]["vel"][[0, 2], [1, 0]], out[False]["vel"][[0, 2], [1, 0]], "the other component")


# ---------------------------------------------------------------------------------------------------------------------
# 6. a batch against one Stepper per system
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", SEMANTICS)
def test_batch_equals_steppers(nb, semantics):
    sizes, m, steps = [0, 1, 130, 300, 1024], 65, 4
    cases = [tc.dense_case(nb, n, seed=50 + n) for n in sizes]
    S, cap = len(sizes), 1024
    for s, (cfg, _) in enumerate(cases):
        cfg.timestep = 0.2 + 0.01 * s                           # parameters of its own per system
    pos = np.stack([tc.tracer_set(cfg, m, seed=n)[0] for n, (cfg, _) in zip(sizes, cases)])
    vel = tc.tracer_set(cases[0][0], m, seed=77)[1]             # (m, 2): given to every system
    with nb.StepperBatch(S, cap, params=[params_of(cfg) for cfg, _ in cases], semantics=semantics) as batch:
        batch.upload([b for _, b in cases])
        batch.set_tracers(pos, vel, walls=True)
        t0 = batch.tracers()
        assert t0["pos"].shape == (S, m, 2) and t0["phi"].shape == (S, m) and t0["steps"].tolist() == [0] * S
        for s in range(S):
            assert_bits(t0["pos"][s], pos[s], "set pos")
            assert_bits(t0["vel"][s], vel, "broadcast vel")
        batch.step(steps)
        got = batch.tracers()
        counts = batch.counts()
    assert got["steps"].tolist() == [steps] * S
    assert counts[0] == 0 and counts[3] < 300
    for s, (cfg, b) in enumerate(cases):
        if sizes[s] == 0:                                       # an empty system: the tracers drift only
            want = {"pos": pos[s], "vel": vel}
            for _ in range(steps):
                want = tc.advance(want, np.zeros((m, 2)), tc.dt_of(nb, cfg, nb.F32), True, (cfg.fieldWidth, cfg.fieldHeight))
            want.update(acc=np.zeros((m, 2)), phi=np.zeros(m), coincident=0)
        else:
            with nb.Stepper(cfg, capacity=cap, semantics=semantics) as st:
                st.upload(b)
                st.set_tracers(pos[s], vel, walls=True)
                st.step(steps)
                want = st.tracers()
                assert st.body_count() == counts[s]
        for k in ("pos", "vel", "acc", "phi"):
            assert_bits(got[k][s], want[k], "system %d (n0 %d) %s" % (s, sizes[s], k))
        assert got["coincident"][s] == want["coincident"]
    with nb.StepperBatch(2, 8, cfg=cases[1][0]) as small:       # (m, 2) for both: every system gets the same tracers
        small.set_tracers(pos[1])
        t = small.tracers()
        for s in range(2):
            assert_bits(t["pos"][s], pos[1], "broadcast pos")
        assert not t["vel"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. lifecycle and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_lifecycle(nb):
    cfg, b = tc.dense_case(nb, 300)
    pos, vel = tc.tracer_set(cfg, 65, seed=6)
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as twin:
        t = st.tracers()                                        # get before set
        assert t["pos"].shape == (0, 2) and t["phi"].shape == (0,) and (t["steps"], t["coincident"]) == (0, 0)
        st.upload(b)
        twin.upload(b)
        st.set_tracers(pos, vel)
        st.step(2)
        twin.step(2)
        st.clear_tracers()                                      # m = 0 removes
        assert st.tracers()["pos"].shape == (0, 2)
        st.step(2)
        twin.step(2)
        assert_same_bodies(st, twin, "after clear_tracers")
        st.set_tracers(pos, vel)
        st.step(3)
        t3 = st.tracers()
        assert t3["steps"] == 3
        st.upload(b)                                            # tracers survive an upload, with their counters
        t = st.tracers()
        for k in ("pos", "vel", "acc", "phi"):
            assert_bits(t[k], t3[k], k)
        assert t["steps"] == 3
        twin.upload(b)
        checked_step(nb, st, twin, cfg, nb.F32, False, 4, t3["coincident"], "after the upload")
        st.set_tracers(pos[:3])                                 # set again: replaced, counters and "last" zeroed
        t = st.tracers()
        assert t["pos"].shape == (3, 2) and t["steps"] == 0 and not t["vel"].any() and not tc.bits(t["acc"]).any()


def test_refusals(nb):
    cfg, b = tc.dense_case(nb, 300)
    pos, _ = tc.tracer_set(cfg, 5, seed=1)
    rec = np.zeros(5, dtype=nb.TRACER_DTYPE)
    info = np.zeros(1, dtype=nb.TRACER_INFO_DTYPE)
    grp = nb.StepperGroup(2, cfg=cfg)
    grp.upload(b)
    with pytest.raises(nb.NbodyError) as ei:
        grp.ranks[1].set_tracers(pos)
    assert ei.value.status == STATE_ERR and "single-rank" in str(ei.value)
    grp.step(2)                                                 # and the group still steps
    want = grp.download()
    grp.close()
    with nb.Stepper(cfg, comm_id=nb.comm_unique_id(), force_comm=True) as rc:
        rc.upload(b)
        with pytest.raises(nb.NbodyError) as ei:
            rc.set_tracers(pos)
        assert ei.value.status == STATE_ERR and "single-rank" in str(ei.value)
        rc.step(2)
        got = rc.download()
        assert got.numBodies == want.numBodies and np.array_equal(got.block.view(np.uint32), want.block.view(np.uint32))
    with nb.Stepper(cfg) as st, nb.StepperBatch(2, 300, cfg=cfg) as batch:
        st.upload(b)
        batch.upload([b, b])
        for call, h in ((nb.lib.nbody_tracers_set, st._ctx), (nb.lib.nbody_batch_tracers_set, batch._b)):
            assert call(h, rec.ctypes.data, -1, 0) == INVALID
            assert call(h, rec.ctypes.data, 5, 2) == INVALID and "flags" in nb.lib.nbody_last_error_string().decode()
            assert call(h, None, 5, 0) == INVALID
            assert call(h, rec.ctypes.data, (1 << 26) + 1, 0) == INVALID and "2^31" in nb.lib.nbody_last_error_string().decode()
        assert nb.lib.nbody_tracers_get(st._ctx, rec.ctypes.data, None, -1, info.ctypes.data) == INVALID
        assert nb.lib.nbody_tracers_get(st._ctx, None, None, 5, info.ctypes.data) == INVALID
        st.set_tracers(pos)                                     # both are still usable
        batch.set_tracers(pos)
        st.step(2)
        batch.step(2)
        t, tb = st.tracers(), batch.tracers()
        for s in range(2):
            assert_bits(tb["pos"][s], t["pos"], "system %d" % s)
        assert t["steps"] == 2 and st.body_count() == want.numBodies
