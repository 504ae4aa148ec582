"""Tidal tensor and jerk (nbody_get_tides, nbody_batch_get_tides; Stepper.tides, StepperGroup.tides, StepperBatch.tides) on
the MI355X: the field's derivatives at the bodies' own positions and at probe points.

Product against oracle: the long-double oracle and the derived bounds of tide_cases.py ((n + 26) u B_ab per tensor
component, (2 n + 28) u B_a per jerk component; nothing fitted to runs).  Product against product - the same state through
another route: with or without the jerk, other points beside it, another partition, a batch - zero tolerance, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_diagnostics as dg
import tide_cases as tc
from test_gpu_batch import FIELD_OF, params_of
from test_gpu_diagnostics import bodies_with_velocities, state_arrays
from test_gpu_field import probe_points
from tide_cases import G, U

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


def setup_module(module):
    tc.require_long_double()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def tide_bits(t):
    return (bits(t["tide"]).tobytes(), bits(t["jerk"]).tobytes() if "jerk" in t else None,
            np.asarray(t["coincident"]).tolist())


def point_velocities(m, seed):
    return np.random.default_rng(seed).uniform(-4, 4, size=(m, 2))


def check_state(nb, st, what, explicit=(), seed=5, cfg=None):
    """The resident state of `st` against the oracle: own rows with and without the jerk, then explicit point sets of the
    given sizes - moving, at rest, and the tensor alone; the tensor bits the same in all of them; the coincident count
    against field()'s."""
    P, V, M = state_arrays(st.download())
    n = len(M)
    own, ownj = st.tides(), st.tides(jerk=True)
    assert own["tide"].shape == (n, 3) and ownj["jerk"].shape == (n, 2) and "jerk" not in own
    assert same(own["tide"], ownj["tide"]), what
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, rows=np.arange(n))
    assert own["coincident"] == ownj["coincident"] == coin == st.field()["coincident"], what
    tc.check_tides(ownj["tide"], ownj["jerk"], tide, jerk, bt, bj, n, what + " own rows")
    for m in explicit:
        pts, pv = probe_points(cfg, m, seed + m), point_velocities(m, seed + m)
        alone, rest, moving = st.tides(pts), st.tides(pts, jerk=True), st.tides(pts, pv, jerk=True)
        assert alone["tide"].shape == (m, 3) and moving["jerk"].shape == (m, 2)
        assert same(alone["tide"], rest["tide"]) and same(alone["tide"], moving["tide"]), (what, m)
        tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
        assert alone["coincident"] == rest["coincident"] == moving["coincident"] == coin == 0, (what, m)
        tc.check_tides(moving["tide"], moving["jerk"], tide, jerk, bt, bj, n, "%s %d moving points" % (what, m))
        tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=pts)
        tc.check_tides(rest["tide"], rest["jerk"], tide, jerk, bt, bj, n, "%s %d points at rest" % (what, m))
    return ownj


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the oracle, 2. after collisions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 255, 256, 257, 300, 1000])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_oracle(nb, precision, n):
    cfg, b = bodies_with_velocities(nb, n, precision, seed=n)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    check_state(nb, st, "n %d" % n, explicit=(1, 255, 256, 257, 1000), cfg=cfg)
    st.close()


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_after_collisions(nb, precision, n):
    cfg, b = bodies_with_velocities(nb, n, precision, seed=n, field=FIELD_OF[n])
    st = nb.Stepper(cfg, precision=precision, record_events=True)
    st.upload(b)
    st.step(5)
    assert len(st.events()) > 0 and st.body_count() < n         # stock radii in a dense field: bodies have merged
    check_state(nb, st, "n %d after 5 steps" % n, explicit=(257,), cfg=cfg)
    st.close()


def test_sources_at_rest_give_T_v(nb):
    """adot = T v with every source at rest, here through the library: within the two bounds."""
    cfg, b = bodies_with_velocities(nb, 300, nb.F64, seed=2)
    b.Velocities[:] = 0
    with nb.Stepper(cfg, precision=nb.F64) as st:
        st.upload(b)
        pts, pv = probe_points(cfg, 129, 3), point_velocities(129, 3)
        t = st.tides(pts, pv, jerk=True)
        P, V, M = state_arrays(b)
        _, _, _, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
        T = t["tide"]
        want = np.stack([T[:, 0] * pv[:, 0] + T[:, 1] * pv[:, 1], T[:, 1] * pv[:, 0] + T[:, 2] * pv[:, 1]], axis=1)
        # T's error times |v|, the jerk's own, and the two roundings of the product formed here
        slack = (300 + tc.TIDE_C + 2) * U * (np.stack([bt[:, 0] + bt[:, 1], bt[:, 1] + bt[:, 2]], axis=1).astype(np.float64) * 4) \
            + (2 * 300 + tc.JERK_C) * U * bj.astype(np.float64)
        assert (np.abs(t["jerk"] - want) <= slack).all()
        assert (st.tides(pts, jerk=True)["jerk"] == 0).all()        # a point at rest among sources at rest


# ---------------------------------------------------------------------------------------------------------------------
# 3. awkward inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_coincident_bodies_probe_on_a_body_nan_mass_one_body(nb, precision):
    cfg, b = bodies_with_velocities(nb, 200, precision, seed=1)
    st = nb.Stepper(cfg, precision=precision)
    b.Positions[150] = b.Positions[20]                          # two coincident bodies among others
    b.Positions[199] = b.Positions[20]                          # and a third
    st.upload(b)
    P, V, M = state_arrays(b)
    own = check_state(nb, st, "coincident bodies", explicit=(129,), cfg=cfg)
    assert own["coincident"] == 6 and np.isfinite(own["tide"]).all() and np.isfinite(own["jerk"]).all()
    pts, pv = probe_points(cfg, 70, 2), point_velocities(70, 2)
    far = st.tides(pts, pv, jerk=True)                          # no probe on a body yet: the chain's bits
    on = pts.copy()
    on[3], on[64], on[69] = P[20], P[7], P[199]                 # probes on bodies: 3 sources, 1 source, 3 sources
    f = st.tides(on, pv, jerk=True)
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=on, point_vel=pv)
    assert f["coincident"] == coin == 7 == st.field(on)["coincident"]
    tc.check_tides(f["tide"], f["jerk"], tide, jerk, bt, bj, 200, "probes on bodies")
    assert np.isfinite(f["tide"]).all() and np.isfinite(f["jerk"]).all()
    keep = np.ones(70, dtype=bool)
    keep[[3, 64, 69]] = False                                   # the rows beside the flagged ones keep their chain bits
    assert same(f["tide"][keep], far["tide"][keep]) and same(f["jerk"][keep], far["jerk"][keep])
    assert same(f["tide"], st.tides(on)["tide"])
    # an infinite velocity: every jerk sum is flagged and stays non-finite, every tensor sum is finite and keeps its bits
    b1 = b.copy()
    b1.Velocities[10] = [np.inf, 0.0]
    st.upload(b1)
    t = st.tides(jerk=True)
    assert same(t["tide"], own["tide"]) and same(t["tide"], st.tides()["tide"]) and t["coincident"] == 6
    assert not np.isfinite(t["jerk"][:, 0]).any()
    # a NaN mass: a source like any other - every other body and every point sees NaN, the body itself does not
    b2 = b.copy()
    b2.Masses[33] = np.nan
    st.upload(b2)
    own = st.tides(jerk=True)
    assert own["coincident"] == 6 == st.field()["coincident"]
    others = np.arange(200) != 33
    assert np.isnan(own["tide"][others]).all() and np.isnan(own["jerk"][others]).all()
    assert np.isfinite(own["tide"][33]).all() and np.isfinite(own["jerk"][33]).all()
    P2, V2, M2 = state_arrays(b2)
    sub = np.concatenate([[33], np.arange(200)[others]])
    tide, jerk, _, bt, bj = tc.exact_tides(P2[sub], V2[sub], np.concatenate([[0.0], M2[sub[1:]]]), rows=[0])
    tc.check_tides(own["tide"][33:34], own["jerk"][33:34], tide, jerk, bt, bj, 200, "the NaN body's own row")
    assert np.isnan(st.tides(pts[:5])["tide"]).all()
    # one body: nothing acts on it; a point beside it sees it
    one = nb.BodiesData.from_arrays([[10.0, 20.0]], [[2.0, -1.0]], [4.0], [1.0], precision)
    st.upload(one)
    own = st.tides(jerk=True)
    assert own["coincident"] == 0 and own["tide"].shape == (1, 3) and own["jerk"].shape == (1, 2)
    assert not bits(own["tide"]).any() and not bits(own["jerk"]).any()
    f = st.tides([[13.0, 24.0], [10.0, 20.0]], jerk=True)
    assert f["coincident"] == 1 and not bits(f["tide"][1]).any() and not bits(f["jerk"][1]).any()
    tide, jerk, _, bt, bj = tc.exact_tides(np.array([[10.0, 20.0]]), np.array([[2.0, -1.0]]), np.array([4.0]),
                                           points=[[13.0, 24.0]])
    tc.check_tides(f["tide"][:1], f["jerk"][:1], tide, jerk, bt, bj, 1, "a point beside the one body")
    q = G * 4.0 / 125.0                                         # d = (-3, -4), r = 5: u = (-0.6, -0.8)
    assert abs(f["tide"][0, 0] - q * (3 * 0.36 - 1)) <= 27 * U * q * 2.08 and abs(f["tide"][0, 1] - q * 1.44) <= 27 * U * q * 1.44
    st.close()


@pytest.mark.parametrize("e,me,ve", tc.FAR_CASES)
def test_fp64_bodies_far_outside_the_usual_range(nb, e, me, ve):
    """Three fp64 bodies 2^e apart with masses 2^me and velocities 2^ve (tide_cases.far_state; test_tide_cases_cpu.py checks
    that every exact term is a normal double): where the chain leaves its range the general code takes over; the result
    is finite and inside the bound."""
    P, V, M, pts, pv = tc.far_state(e, me, ve)
    st = nb.Stepper(capacity=4, precision=nb.F64, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    st.upload(nb.BodiesData.from_arrays(P, V, M, np.zeros(3), nb.F64))
    own = st.tides(jerk=True)
    assert own["coincident"] == 0 and np.isfinite(own["tide"]).all() and np.isfinite(own["jerk"]).all()
    assert same(own["tide"], st.tides()["tide"])
    tide, jerk, _, bt, bj = tc.exact_tides(P, V, M, rows=[0, 1, 2])
    tc.check_tides(own["tide"], own["jerk"], tide, jerk, bt, bj, 3, "2^%d apart" % e)
    f = st.tides(pts, pv, jerk=True)
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
    assert f["coincident"] == coin == 0 and np.isfinite(f["tide"]).all() and np.isfinite(f["jerk"]).all()
    tc.check_tides(f["tide"], f["jerk"], tide, jerk, bt, bj, 3, "2^%d apart, points" % e)
    assert same(f["tide"], st.tides(pts)["tide"])
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. point independence, 5. partition independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_point_independence(nb, precision):
    cfg, b = bodies_with_velocities(nb, 777, precision, seed=9)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    pts, pv = probe_points(cfg, 600, 4), point_velocities(600, 4)
    pts[17] = np.asarray(b.Positions[5], dtype=np.float64)       # one of them on a body
    f = st.tides(pts, pv, jerk=True)
    perm = np.random.default_rng(1).permutation(600)
    g = st.tides(pts[perm], pv[perm], jerk=True)
    assert same(g["tide"], f["tide"][perm]) and same(g["jerk"], f["jerk"][perm])
    assert g["coincident"] == f["coincident"] == 1
    assert same(st.tides(pts)["tide"], f["tide"])
    for p in (0, 17, 255, 256, 599):
        h = st.tides(pts[p:p + 1], pv[p:p + 1], jerk=True)
        assert same(h["tide"][0], f["tide"][p]) and same(h["jerk"][0], f["jerk"][p]), p
        assert h["coincident"] == (1 if p == 17 else 0)
        assert same(st.tides(pts[p:p + 1])["tide"][0], f["tide"][p]), p
    # a body's own position and velocity as an explicit point: the body itself is then a source at distance 0, counted
    # and left out; the rest is the same sum by the general code
    own = st.tides(jerk=True)
    P, V, M = state_arrays(b)
    h = st.tides(P[300:301], V[300:301], jerk=True)
    assert h["coincident"] == 1
    tide, jerk, _, bt, bj = tc.exact_tides(P, V, M, rows=[300])
    tc.check_tides(h["tide"], h["jerk"], tide, jerk, bt, bj, 777, "body 300 as a point")
    tc.check_tides(own["tide"][300:301], own["jerk"][300:301], tide, jerk, bt, bj, 777, "body 300 as a row")
    st.close()


@pytest.mark.parametrize("n", [300, 1000])
def test_partition_independence(nb, n):
    """Worlds 1, 2 and 3 on one device (every rank on its own), the single-rank RCCL path and a plain context: the tensor
    has the same bits, at upload and after two steps; the jerk there is NBODY_ERR_STATE."""
    cfg, b = bodies_with_velocities(nb, n, nb.F32, seed=n, field=FIELD_OF[n])
    pts = probe_points(cfg, 300, 8)
    plain = nb.Stepper(cfg)
    plain.upload(b)
    ref = []
    for steps in (0, 2):
        plain.step(steps)
        ref.append((tide_bits(plain.tides()), tide_bits(plain.tides(pts))))
        assert same(plain.tides(jerk=True)["tide"], plain.tides()["tide"])
    plain.close()
    for world in (1, 2, 3):
        grp = nb.StepperGroup(world, cfg=cfg)
        grp.upload(b)
        for k, steps in enumerate((0, 2)):
            grp.step(steps)
            for rank in range(world):
                assert tide_bits(grp.tides(rank=rank)) == ref[k][0], (world, rank, steps)
                assert tide_bits(grp.tides(pts, rank=rank)) == ref[k][1], (world, rank, steps)
                if world == 1:                                   # a group of one is a plain context: it holds every velocity
                    assert bits(grp.ranks[0].tides(jerk=True)["tide"]).tobytes() == ref[k][0][0]
                    continue
                with pytest.raises(nb.NbodyError) as err:
                    grp.ranks[rank].tides(jerk=True)
                assert err.value.status == STATE_ERR
        grp.close()
    rc = nb.Stepper(cfg, comm_id=nb.comm_unique_id(), force_comm=True)
    rc.upload(b)
    for k, steps in enumerate((0, 2)):
        rc.step(steps)
        assert tide_bits(rc.tides()) == ref[k][0] and tide_bits(rc.tides(pts)) == ref[k][1], steps
    with pytest.raises(nb.NbodyError) as err:
        rc.tides(pts, jerk=True)
    assert err.value.status == STATE_ERR
    rc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,variant", [(0, 52), (1, 0)], ids=["f32-ring", "f64"])
def test_no_effect_on_stepping(nb, precision, variant):
    cfg = nb.stock_config(particleCount=3000, fieldWidth=5000, fieldHeight=5000)
    b = nb.init_bodies(cfg, precision)
    pts, pv = probe_points(cfg, 100, 3), point_velocities(100, 3)

    def run(with_calls):
        st = nb.Stepper(cfg, precision=precision, record_events=True, kernel_variant=variant)
        st.upload(b)
        for k in range(5):
            st.step(2)
            if with_calls:
                st.tides()
                st.tides(jerk=True)
                st.tides(pts)
                st.tides(pts, pv, jerk=True)
        d = st.download()
        ev = np.sort(st.events(), order=["step", "i", "j", "kind"])
        out = (d.numBodies, d.block.view(np.uint32).tobytes(), ev.tobytes(), st.stats().pairs, st.stats().steps,
               st.force_kernel_name())
        st.close()
        return out

    a, c = run(False), run(True)
    assert a == c
    assert a[0] < 3000 and len(a[2]) > 0                        # collisions happened
    if precision == nb.F32:
        assert "ring" in a[5], a[5]


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [0, 1, 127, 128, 129, 256, 257, 1000, 1500]


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper(nb, semantics, lanes):
    cap = 1500
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        field = FIELD_OF.get(n, 3000)
        cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field)
        bd = nb.init_bodies(cfg, seed=40 + s) if n else nb.BodiesData(0)
        if n:
            bd.Velocities[:] = np.random.default_rng(40 + s).uniform(-3, 3, size=(n, 2)).astype(np.float32)
        cfgs.append(cfg)
        bodies.append(bd)
    S = len(BATCH_SIZES)
    batch = nb.StepperBatch(S, cap, params=[params_of(c) for c in cfgs], semantics=semantics, kernel_variant=lanes)
    batch.upload(bodies)
    one = nb.Stepper(cfgs[-1], capacity=cap, semantics=semantics)
    pts, pv = probe_points(cfgs[-1], 300, 6), point_velocities(300, 6)
    for steps in (0, 3):
        batch.step(steps)
        own, exp, counts = batch.tides(jerk=True), batch.tides(pts, pv, jerk=True), batch.counts()
        fld = batch.field()
        assert own["tide"].shape == (S, cap, 3) and own["jerk"].shape == (S, cap, 2) and own["coincident"].shape == (S,)
        assert exp["tide"].shape == (S, 300, 3) and exp["jerk"].shape == (S, 300, 2) and own["coincident"].dtype == np.int64
        assert same(batch.tides()["tide"], own["tide"]) and same(batch.tides(pts)["tide"], exp["tide"])
        assert np.array_equal(own["coincident"], fld["coincident"])
        for s in range(S):
            n = int(counts[s])
            assert not bits(own["tide"][s, n:]).any() and not bits(own["jerk"][s, n:]).any(), s   # zero-filled past the count
            if n == 0:                                          # an empty system: +0 everywhere, nothing coincident
                assert not bits(exp["tide"][s]).any() and not bits(exp["jerk"][s]).any() and exp["coincident"][s] == 0
                continue
            one.upload(batch.download(s))
            f, g = one.tides(jerk=True), one.tides(pts, pv, jerk=True)
            assert same(f["tide"], own["tide"][s, :n]) and same(f["jerk"], own["jerk"][s, :n]), (s, steps)
            assert same(g["tide"], exp["tide"][s]) and same(g["jerk"], exp["jerk"][s]), (s, steps)
            assert f["coincident"] == own["coincident"][s] and g["coincident"] == exp["coincident"][s] == 0
        if steps:
            assert int(counts[7]) < 1000                        # the dense systems have merged bodies by now
    one.close()
    batch.close()


def test_batch_of_1024_systems_of_64(nb):
    S, n = 1024, 64
    cfg = nb.stock_config(particleCount=n, fieldWidth=500, fieldHeight=500)
    bodies = [nb.init_bodies(cfg, seed=900 + s) for s in range(S)]
    batch = nb.StepperBatch(S, n, cfg=cfg)
    batch.upload(bodies)
    batch.step(2)
    pts, pv = probe_points(cfg, 16, 12), point_velocities(16, 12)
    exp, own, counts = batch.tides(pts, pv, jerk=True), batch.tides(jerk=True), batch.counts()
    assert exp["tide"].shape == (S, 16, 3) and not exp["coincident"].any()
    assert same(batch.tides(pts)["tide"], exp["tide"]) and same(batch.tides()["tide"], own["tide"])
    one = nb.Stepper(cfg, capacity=n)
    for s in (0, 1, 63, 64, 511, 1023):
        d = batch.download(s)
        one.upload(d)
        f, g = one.tides(jerk=True), one.tides(pts, pv, jerk=True)
        k = int(counts[s])
        assert same(g["tide"], exp["tide"][s]) and same(g["jerk"], exp["jerk"][s]), s
        assert same(f["tide"], own["tide"][s, :k]) and same(f["jerk"], own["jerk"][s, :k]), s
        P, V, M = state_arrays(d)
        tide, jerk, _, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
        tc.check_tides(exp["tide"][s], exp["jerk"][s], tide, jerk, bt, bj, k, "system %d" % s)
    one.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    cfg, b = bodies_with_velocities(nb, 300, nb.F32)
    st = nb.Stepper(cfg)
    tide = np.full((300, 3), 7.0)
    jerk = np.full((300, 2), 7.0)
    pts, pv = probe_points(cfg, 4, 1), point_velocities(4, 1)
    n, coin = ctypes.c_int(-5), ctypes.c_int64(-5)
    args = (ctypes.byref(n), ctypes.byref(coin))
    call = nb.lib.nbody_get_tides
    assert call(st._ctx, None, None, 300, tide.ctypes.data, jerk.ctypes.data, *args) == STATE_ERR       # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    assert call(st._ctx, pts.ctypes.data, None, -1, tide.ctypes.data, None, *args) == INVALID
    assert call(st._ctx, pts.ctypes.data, None, 4, None, None, *args) == INVALID
    assert call(st._ctx, None, pv.ctypes.data, 300, tide.ctypes.data, jerk.ctypes.data, *args) == INVALID
    assert call(st._ctx, pts.ctypes.data, pv.ctypes.data, 4, tide.ctypes.data, None, *args) == INVALID
    assert call(st._ctx, pts.ctypes.data, None, (1 << 31) // 24 + 1, tide.ctypes.data, None, *args) == INVALID
    assert call(st._ctx, None, None, 299, tide.ctypes.data, jerk.ctypes.data, *args) == CAPACITY_ERR
    assert (tide == 7.0).all() and (jerk == 7.0).all() and n.value == -5 and coin.value == -5
    assert call(st._ctx, pts.ctypes.data, None, 0, tide.ctypes.data, jerk.ctypes.data, *args) == 0 and n.value == 0 and coin.value == 0
    assert (tide == 7.0).all() and (jerk == 7.0).all()
    assert call(st._ctx, None, None, 300, tide.ctypes.data, None, *args) == 0 and n.value == 300
    assert same(tide, st.tides()["tide"]) and (jerk == 7.0).all()          # jerk == NULL: nothing but the tensor is written
    assert call(st._ctx, None, None, 300, tide.ctypes.data, jerk.ctypes.data, *args) == 0
    assert same(jerk, st.tides(jerk=True)["jerk"])
    assert st.tides(np.zeros((0, 2)), jerk=True)["jerk"].shape == (0, 2)
    st.close()
    batch = nb.StepperBatch(2, 300, cfg=cfg)
    bcall = nb.lib.nbody_batch_get_tides
    c2 = (ctypes.c_int64 * 2)(-5, -5)
    btide = np.full((600, 3), 7.0)
    assert bcall(batch._b, None, None, 300, btide.ctypes.data, None, c2) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, pts.ctypes.data, None, -1, btide.ctypes.data, None, c2) == INVALID
    assert bcall(batch._b, pts.ctypes.data, None, 4, None, None, c2) == INVALID
    assert bcall(batch._b, pts.ctypes.data, None, 4, btide.ctypes.data, None, None) == INVALID
    assert bcall(batch._b, pts.ctypes.data, None, (1 << 31) // 48 + 1, btide.ctypes.data, None, c2) == INVALID   # two systems
    assert (btide == 7.0).all()
    assert bcall(batch._b, pts.ctypes.data, None, 0, btide.ctypes.data, None, c2) == 0 and list(c2) == [0, 0]
    assert bcall(batch._b, None, None, 300, btide.ctypes.data, None, c2) == 0
    assert same(btide[:300], tide) and (btide[300:] == 7.0).all()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the bits, pinned.  The bounds above leave room for a changed chain and the routes compared bit for bit all go through
# one kernel pair; tests/golden/tide_pins.npz holds what the library gave for the states of diag_pins.npz at the points of
# field_pins.npz (both read, not copied) when the fixture was recorded (tests/golden/make_tide_pins.py): the bits may not
# move.  The fixture's own input is the points' velocities, one set per precision.  Point 100 lies on body 5 of the
# n = 300 state: its chains are NaN, the general code answers.
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIDE_PINS = os.path.join(GOLDEN, "tide_pins.npz")
FIELD_PINS = os.path.join(GOLDEN, "field_pins.npz")
TIDE_PIN_POINTS = 257


def pin_tide_velocities(nb, precision):
    """The fixture's point velocities of one precision, made once by the generator."""
    return {"vel_" + dg.pin_tag(nb, precision): dg.pin_bits(point_velocities(TIDE_PIN_POINTS, 71 + precision))}


def pin_tide_result(tag, t):
    return {tag + "_tide": dg.pin_bits(t["tide"]), tag + "_jerk": dg.pin_bits(t["jerk"]),
            tag + "_coincident": np.asarray(t["coincident"], dtype=np.int64).reshape(-1)}


def pin_tide_stepper(nb, states, points, pins, precision, n):
    """-> {key: bits} of tides(jerk=True) and tides(points, point_vel, jerk=True) straight after the upload."""
    tag = "ctx_%s_n%d" % (dg.pin_tag(nb, precision), n)
    pts = points["points_" + dg.pin_tag(nb, precision)].view(np.float64)
    pv = pins["vel_" + dg.pin_tag(nb, precision)].view(np.float64)
    with nb.Stepper(nb.stock_config(particleCount=n), precision=precision) as st:
        st.upload(dg.pin_bodies(nb, states, precision, n))
        return {**pin_tide_result(tag + "_own", st.tides(jerk=True)),
                **pin_tide_result(tag + "_points", st.tides(pts, pv, jerk=True))}


def pin_tide_batch(nb, states, points, pins):
    """One fp32 batch of the systems n = 0, 1, 129, 256, 300 at capacity 300."""
    pts, pv = points["points_f32"].view(np.float64), pins["vel_f32"].view(np.float64)
    cfg = nb.stock_config(particleCount=300)
    with nb.StepperBatch(len(dg.PIN_BATCH_SIZES), 300, cfg=cfg) as b:
        b.upload([dg.pin_bodies(nb, states, nb.F32, n) for n in dg.PIN_BATCH_SIZES])
        return {**pin_tide_result("batch_own", b.tides(jerk=True)), **pin_tide_result("batch_points", b.tides(pts, pv, jerk=True))}


def pin_inputs():
    with np.load(dg.PINS) as z:
        states = {k: z[k] for k in z.files if k.startswith("in_")}
    with np.load(FIELD_PINS) as z:
        points = {k: z[k] for k in z.files if k.startswith("points_")}
    return states, points


def test_pinned_bits(nb):
    with np.load(TIDE_PINS) as z:
        pins = {k: z[k] for k in z.files}
    states, points = pin_inputs()
    got = {}
    for precision in (nb.F32, nb.F64):
        for n in dg.PIN_SIZES:
            got.update(pin_tide_stepper(nb, states, points, pins, precision, n))
    got.update(pin_tide_batch(nb, states, points, pins))
    assert set(got) | {"vel_f32", "vel_f64"} == set(pins)
    dg.check_pins(pins, got)
    for precision in (nb.F32, nb.F64):
        tag = "ctx_%s_n300" % dg.pin_tag(nb, precision)
        assert got[tag + "_own_coincident"].tolist() == [2] and got[tag + "_points_coincident"].tolist() == [2], tag
        assert np.isfinite(got[tag + "_points_tide"].view(np.float64)[100]).all(), tag
    assert got["batch_own_coincident"].tolist() == [0, 0, 0, 0, 2]
    # the batch's n = 300 system is the fp32 context's state: the same bits through the other count policy
    assert np.array_equal(got["batch_points_tide"][4], got["ctx_f32_n300_points_tide"])
    assert np.array_equal(got["batch_own_jerk"][4], got["ctx_f32_n300_own_jerk"])
