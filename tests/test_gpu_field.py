"""Field evaluation (nbody_get_field, nbody_batch_get_field; Stepper.field, StepperGroup.field, StepperBatch.field) on the
MI355X: acceleration and potential at the bodies' own positions and at probe points.

Product against oracle: the long-double oracle and the derived bounds of field_cases.py ((n + 14) u sum |term| per
acceleration component, (n + 4) u |phi|; nothing fitted to runs).  Product against product - the same state through
another route: other points beside it, another partition, a batch - zero tolerance, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import field_cases as fc
import test_gpu_diagnostics as dg
from field_cases import G, LD, U
from test_gpu_batch import FIELD_OF, params_of
from test_gpu_diagnostics import bodies_with_velocities, state_arrays

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


def setup_module(module):
    fc.require_long_double()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def field_bits(f):
    return (bits(f["acc"]).tobytes(), bits(f["phi"]).tobytes(), np.asarray(f["coincident"]).tolist())


def probe_points(cfg, m, seed):
    """m points: uniform over the field, the last one far outside it."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, size=(m, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
    pts[-1] = [-7.5 * cfg.fieldWidth, 11.25 * cfg.fieldHeight]
    return pts


def check_state(nb, st, what, explicit=(), seed=5, cfg=None, sample=None):
    """The resident state of `st` against the oracle: points=None (all rows, or `sample` of them), then explicit point
    sets of the given sizes; phi and the coincident count against the diagnostics, bit for bit."""
    P, _, M = state_arrays(st.download())
    n = len(M)
    own = st.field()
    dg = st.diagnostics(potential=True)
    assert own["acc"].shape == (n, 2) and own["phi"].shape == (n,)
    assert np.array_equal(bits(own["phi"]), bits(dg["phi"])), what
    assert own["coincident"] == dg["coincident_pairs"], what
    rows = np.arange(n) if sample is None else sample
    acc, phi, mag, coin = fc.exact_field(P, M, rows=rows)
    if sample is None:
        assert own["coincident"] == coin, what
    fc.check_field(own["acc"][rows], own["phi"][rows], acc, phi, mag, n, what + " own positions")
    for m in explicit:
        pts = probe_points(cfg, m, seed + m)
        f = st.field(pts)
        assert f["acc"].shape == (m, 2) and f["phi"].shape == (m,)
        acc, phi, mag, coin = fc.exact_field(P, M, points=pts)
        assert f["coincident"] == coin == 0, (what, m)
        fc.check_field(f["acc"], f["phi"], acc, phi, mag, n, "%s %d points" % (what, m))
    return own


# ---------------------------------------------------------------------------------------------------------------------
# 1. closed forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_closed_forms(nb, precision):
    st = nb.Stepper(capacity=8, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    for e in (-20, -3, 0, 1, 7, 30):                            # two bodies a power of two apart: everything but G is exact
        d, m0, m1 = 2.0 ** e, 3.0, 5.0
        st.upload(nb.BodiesData.from_arrays([[0.0, 2.0], [d, 2.0]], [[0, 0], [0, 0]], [m0, m1], [0, 0], precision))
        f = st.field()
        want_a = np.array([[G * m1 / d / d, 0.0], [-G * m0 / d / d, 0.0]])
        want_p = np.array([-G * m1 / d, -G * m0 / d])
        assert f["coincident"] == 0
        assert (np.abs(f["acc"] - want_a) <= (2 + fc.ACC_C) * U * np.abs(want_a)).all(), (e, f["acc"], want_a)
        assert (np.abs(f["phi"] - want_p) <= (2 + fc.PHI_C) * U * np.abs(want_p)).all(), (e, f["phi"], want_p)
        g = st.field([[-d, 2.0]])                               # on the axis: d from body 0, 2 d from body 1
        wa, wp = G * (m0 / d / d + m1 / (4 * d * d)), -G * (m0 / d + m1 / (2 * d))
        assert abs(g["acc"][0, 0] - wa) <= (2 + fc.ACC_C) * U * wa and g["acc"][0, 1] == 0
        assert abs(g["phi"][0] - wp) <= (2 + fc.PHI_C) * U * -wp
    # the centre of a square of equal masses (vertices exact in both precisions): the terms cancel, phi = -G n m / R
    R, m = 1024.0, 7.0
    sq = [[R, 0.0], [0.0, R], [-R, 0.0], [0.0, -R]]
    st.upload(nb.BodiesData.from_arrays(sq, [[0, 0]] * 4, [m] * 4, [0] * 4, precision))
    f = st.field([[0.0, 0.0]])
    term = G * m / R / R
    assert (np.abs(f["acc"][0]) <= (4 + fc.ACC_C) * U * 2 * term).all(), f["acc"]
    assert abs(f["phi"][0] + G * 4 * m / R) <= (4 + fc.PHI_C) * U * G * 4 * m / R
    # a heptagon, vertices rounded to the precision: against the oracle of the rounded vertices
    k = np.arange(7)
    hep = nb.BodiesData.from_arrays(np.stack([R * np.cos(2 * np.pi * k / 7), R * np.sin(2 * np.pi * k / 7)], axis=1),
                                    np.zeros((7, 2)), [m] * 7, [0] * 7, precision)
    st.upload(hep)
    P, _, M = state_arrays(hep)
    f = st.field([[0.0, 0.0]])
    acc, phi, mag, coin = fc.exact_field(P, M, points=[[0.0, 0.0]])
    fc.check_field(f["acc"], f["phi"], acc, phi, mag, 7, "heptagon")
    # a vertex within eps R of its place moves its term by at most 3 eps of its size; on top, the bound of the sum itself
    eps = 2.0 ** -23 if precision == nb.F32 else 2.0 ** -52
    assert (np.abs(f["acc"][0]) <= (7 * 3 * eps + (7 + fc.ACC_C) * U * 7) * term).all()
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle, 3. after collisions, 4. a sampled large state; 5. phi bits in every one of them
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


def test_sampled_large_state(nb):
    n = 65536
    cfg, b = bodies_with_velocities(nb, n, nb.F32, seed=3, field=20000)
    st = nb.Stepper(cfg)
    st.upload(b)
    rows = np.sort(np.random.default_rng(11).choice(n, 64, replace=False))
    rows[0], rows[-1] = 0, n - 1
    check_state(nb, st, "n 65536", sample=rows)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. awkward inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_coincident_bodies_probe_on_a_body_nan_mass_one_body(nb, precision):
    cfg, b = bodies_with_velocities(nb, 200, precision, seed=1)
    b.Positions[150] = b.Positions[20]                          # two coincident bodies among others
    b.Positions[199] = b.Positions[20]                          # and a third
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    P, _, M = state_arrays(b)
    own = check_state(nb, st, "coincident bodies", explicit=(129,), cfg=cfg)
    assert own["coincident"] == 6 and np.isfinite(own["acc"]).all() and np.isfinite(own["phi"]).all()
    pts = probe_points(cfg, 70, 2)
    pts[3], pts[64], pts[69] = P[20], P[7], P[199]              # probes on bodies: 3 sources, 1 source, 3 sources
    f = st.field(pts)
    acc, phi, mag, coin = fc.exact_field(P, M, points=pts)
    assert f["coincident"] == coin == 7
    fc.check_field(f["acc"], f["phi"], acc, phi, mag, 200, "probes on bodies")
    assert np.isfinite(f["acc"]).all() and np.isfinite(f["phi"]).all()
    # a NaN mass: a source like any other - every other body and every point sees NaN, the body itself does not
    b2 = b.copy()
    b2.Masses[33] = np.nan
    st.upload(b2)
    own = st.field()
    dg = st.diagnostics(potential=True)
    assert np.array_equal(bits(own["phi"]), bits(dg["phi"])) and own["coincident"] == dg["coincident_pairs"] == 6
    others = np.arange(200) != 33
    assert np.isnan(own["phi"][others]).all() and np.isnan(own["acc"][others]).all()
    assert np.isfinite(own["phi"][33]) and np.isfinite(own["acc"][33]).all()
    P2, _, M2 = state_arrays(b2)
    keep = np.arange(200) != 33                                 # body 33 sees the finite rest
    acc, phi, mag, _ = fc.exact_field(np.concatenate([P2[33:34], P2[keep]]), np.concatenate([[0.0], M2[keep]]), rows=[0])
    fc.check_field(own["acc"][33:34], own["phi"][33:34], acc, phi, mag, 200, "the NaN body's own row")
    assert np.isnan(st.field(pts[:5])["phi"]).all()
    # one body: nothing acts on it; a point beside it sees it
    one = nb.BodiesData.from_arrays([[10.0, 20.0]], [[0, 0]], [4.0], [1.0], precision)
    st.upload(one)
    own = st.field()
    assert own["coincident"] == 0 and own["acc"].shape == (1, 2)
    assert np.array_equal(bits(own["phi"]), bits(st.diagnostics(potential=True)["phi"]))
    assert (own["acc"] == 0).all() and own["phi"][0] == 0
    f = st.field([[13.0, 24.0], [10.0, 20.0]])
    assert f["coincident"] == 1 and (f["acc"][1] == 0).all() and f["phi"][1] == 0
    assert abs(f["phi"][0] + G * 4.0 / 5.0) <= 5 * U * G and abs(f["acc"][0, 0] + G * 4.0 * 3.0 / 125.0) <= 15 * U * G
    st.close()


@pytest.mark.parametrize("e,me", [(-300, 0), (300, 0), (-520, -100), (520, 200), (-345, 0)])
def test_fp64_bodies_far_outside_the_usual_range(nb, e, me):
    """Two (three) fp64 bodies 2^e apart with masses 2^me: where the fast chain leaves its range (y^3 or a product
    overflowing, d2 outside the normal range) the general code takes over; the result is finite - m / r^2 is, in every
    case here - and inside the bound."""
    d, m = 2.0 ** e, 2.0 ** me
    P = np.array([[0.0, 0.0], [d, 0.0], [0.0, -d]])
    M = np.array([m, 3 * m, 5 * m])
    st = nb.Stepper(capacity=4, precision=nb.F64, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    st.upload(nb.BodiesData.from_arrays(P, np.zeros((3, 2)), M, np.zeros(3), nb.F64))
    own = st.field()
    dg = st.diagnostics(potential=True)
    assert np.array_equal(bits(own["phi"]), bits(dg["phi"])) and own["coincident"] == dg["coincident_pairs"] == 0
    assert np.isfinite(own["acc"]).all() and np.isfinite(own["phi"]).all()
    acc, phi, mag, _ = fc.exact_field(P, M, rows=[0, 1, 2])
    assert float(mag.min()) > 2.0 ** -1000                      # the oracle's terms are normal numbers
    fc.check_field(own["acc"], own["phi"], acc, phi, mag, 3, "2^%d apart" % e)
    pts = np.array([[-d, 0.0], [d, d]])
    f = st.field(pts)
    acc, phi, mag, coin = fc.exact_field(P, M, points=pts)
    assert f["coincident"] == coin == 0 and np.isfinite(f["acc"]).all()
    fc.check_field(f["acc"], f["phi"], acc, phi, mag, 3, "2^%d apart, points" % e)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. point independence, 8. partition independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_point_independence(nb, precision):
    cfg, b = bodies_with_velocities(nb, 777, precision, seed=9)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    pts = probe_points(cfg, 600, 4)
    pts[17] = np.asarray(b.Positions[5], dtype=np.float64)       # one of them on a body
    f = st.field(pts)
    perm = np.random.default_rng(1).permutation(600)
    g = st.field(pts[perm])
    assert np.array_equal(bits(g["acc"]), bits(f["acc"][perm])) and np.array_equal(bits(g["phi"]), bits(f["phi"][perm]))
    assert g["coincident"] == f["coincident"] == 1
    for p in (0, 17, 255, 256, 599):
        h = st.field(pts[p:p + 1])
        assert np.array_equal(bits(h["acc"][0]), bits(f["acc"][p])) and bits(h["phi"])[0] == bits(f["phi"])[p], p
        assert h["coincident"] == (1 if p == 17 else 0)
    # a body's own position as an explicit point: the body itself is then a source at distance 0, the rest is the same sum
    own = st.field()
    h = st.field(np.asarray(b.Positions[300:301], dtype=np.float64))
    assert h["coincident"] == 1
    assert abs(h["phi"][0] - own["phi"][300]) <= (777 + 4) * U * abs(own["phi"][300])
    st.close()


@pytest.mark.parametrize("n", [300, 1000])
def test_partition_independence(nb, n):
    """Worlds 1, 2 and 3 on one device (every rank on its own), the single-rank RCCL path and a plain context: the same
    bits, at upload and after two steps."""
    cfg, b = bodies_with_velocities(nb, n, nb.F32, seed=n, field=FIELD_OF[n])
    pts = probe_points(cfg, 300, 8)
    plain = nb.Stepper(cfg)
    plain.upload(b)
    ref = []
    for steps in (0, 2):
        plain.step(steps)
        ref.append((field_bits(plain.field()), field_bits(plain.field(pts))))
    plain.close()
    for world in (1, 2, 3):
        grp = nb.StepperGroup(world, cfg=cfg)
        grp.upload(b)
        for k, steps in enumerate((0, 2)):
            grp.step(steps)
            for rank in range(world):
                assert field_bits(grp.field(rank=rank)) == ref[k][0], (world, rank, steps)
                assert field_bits(grp.field(pts, rank=rank)) == ref[k][1], (world, rank, steps)
        grp.close()
    rc = nb.Stepper(cfg, comm_id=nb.comm_unique_id(), force_comm=True)
    rc.upload(b)
    for k, steps in enumerate((0, 2)):
        rc.step(steps)
        assert field_bits(rc.field()) == ref[k][0] and field_bits(rc.field(pts)) == ref[k][1], steps
    rc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,variant", [(0, 52), (1, 0)], ids=["f32-ring", "f64"])
def test_no_effect_on_stepping(nb, precision, variant):
    cfg = nb.stock_config(particleCount=3000, fieldWidth=5000, fieldHeight=5000)
    b = nb.init_bodies(cfg, precision)
    pts = probe_points(cfg, 100, 3)

    def run(with_calls):
        st = nb.Stepper(cfg, precision=precision, record_events=True, kernel_variant=variant)
        st.upload(b)
        for k in range(5):
            st.step(2)
            if with_calls:
                st.field()
                st.field(pts)
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
# 10. batch
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
    pts = probe_points(cfgs[-1], 300, 6)
    for steps in (0, 3):
        batch.step(steps)
        own, exp, counts = batch.field(), batch.field(pts), batch.counts()
        dg = batch.diagnostics(potential=True)
        assert own["acc"].shape == (S, cap, 2) and own["phi"].shape == (S, cap) and own["coincident"].shape == (S,)
        assert exp["acc"].shape == (S, 300, 2) and exp["phi"].shape == (S, 300) and own["coincident"].dtype == np.int64
        for s in range(S):
            n = int(counts[s])
            assert (own["acc"][s, n:] == 0).all() and (own["phi"][s, n:] == 0).all(), s   # zero-filled past the count
            assert np.array_equal(bits(own["phi"][s, :n]), bits(dg[s]["phi"])), (s, steps)
            assert own["coincident"][s] == dg[s]["coincident_pairs"], (s, steps)
            if n == 0:                                          # an empty system: +0 everywhere, nothing coincident
                assert not bits(exp["acc"][s]).any() and not bits(exp["phi"][s]).any() and exp["coincident"][s] == 0
                continue
            one.upload(batch.download(s))
            f, g = one.field(), one.field(pts)
            assert np.array_equal(bits(f["acc"]), bits(own["acc"][s, :n])), (s, steps)
            assert np.array_equal(bits(f["phi"]), bits(own["phi"][s, :n])), (s, steps)
            assert np.array_equal(bits(g["acc"]), bits(exp["acc"][s])) and np.array_equal(bits(g["phi"]), bits(exp["phi"][s]))
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
    pts = probe_points(cfg, 16, 12)
    exp, own, counts = batch.field(pts), batch.field(), batch.counts()
    assert exp["acc"].shape == (S, 16, 2) and not exp["coincident"].any()
    one = nb.Stepper(cfg, capacity=n)
    for s in (0, 1, 63, 64, 511, 1023):
        d = batch.download(s)
        one.upload(d)
        f, g = one.field(), one.field(pts)
        k = int(counts[s])
        assert np.array_equal(bits(g["acc"]), bits(exp["acc"][s])) and np.array_equal(bits(g["phi"]), bits(exp["phi"][s])), s
        assert np.array_equal(bits(f["acc"]), bits(own["acc"][s, :k])) and np.array_equal(bits(f["phi"]), bits(own["phi"][s, :k]))
        P, _, M = state_arrays(d)
        acc, phi, mag, _ = fc.exact_field(P, M, points=pts)
        fc.check_field(exp["acc"][s], exp["phi"][s], acc, phi, mag, k, "system %d" % s)
    one.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    cfg, b = bodies_with_velocities(nb, 300, nb.F32)
    st = nb.Stepper(cfg)
    out = np.full(300, 7.0, dtype=nb.FIELD_DTYPE)
    pts = probe_points(cfg, 4, 1)
    n, coin = ctypes.c_int(-5), ctypes.c_int64(-5)
    args = (ctypes.byref(n), ctypes.byref(coin))
    call = nb.lib.nbody_get_field
    assert call(st._ctx, None, 300, out.ctypes.data, *args) == STATE_ERR       # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    assert call(st._ctx, pts.ctypes.data, -1, out.ctypes.data, *args) == INVALID
    assert call(st._ctx, pts.ctypes.data, 4, None, *args) == INVALID
    assert call(st._ctx, pts.ctypes.data, 4, out.ctypes.data, None, ctypes.byref(coin)) == INVALID
    assert call(st._ctx, pts.ctypes.data, 4, out.ctypes.data, ctypes.byref(n), None) == INVALID
    assert call(st._ctx, pts.ctypes.data, (1 << 31) // 24 + 1, out.ctypes.data, *args) == INVALID
    assert call(st._ctx, None, 299, out.ctypes.data, *args) == CAPACITY_ERR     # room for fewer than the 300 bodies
    assert (out["acc"] == 7.0).all() and (out["phi"] == 7.0).all() and n.value == -5 and coin.value == -5
    assert call(st._ctx, pts.ctypes.data, 0, out.ctypes.data, *args) == 0 and n.value == 0 and coin.value == 0
    assert (out["phi"] == 7.0).all()
    assert call(st._ctx, None, 300, out.ctypes.data, *args) == 0 and n.value == 300
    assert np.array_equal(bits(out["phi"]), bits(st.field()["phi"]))
    assert st.field(np.zeros((0, 2)))["phi"].shape == (0,)
    st.close()
    batch = nb.StepperBatch(2, 300, cfg=cfg)
    bcall = nb.lib.nbody_batch_get_field
    c2 = (ctypes.c_int64 * 2)(-5, -5)
    bout = np.full(600, 7.0, dtype=nb.FIELD_DTYPE)
    assert bcall(batch._b, None, 300, bout.ctypes.data, c2) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, pts.ctypes.data, -1, bout.ctypes.data, c2) == INVALID
    assert bcall(batch._b, pts.ctypes.data, 4, None, c2) == INVALID
    assert bcall(batch._b, pts.ctypes.data, 4, bout.ctypes.data, None) == INVALID
    assert (bout["phi"] == 7.0).all()
    assert bcall(batch._b, pts.ctypes.data, 0, bout.ctypes.data, c2) == 0 and list(c2) == [0, 0]
    assert bcall(batch._b, None, 300, bout.ctypes.data, c2) == 0
    assert np.array_equal(bits(bout["phi"][:300]), bits(out["phi"])) and (bout["phi"][300:] == 7.0).all()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 12. the bits, pinned.  The bounds above leave room for a changed summation order and the routes compared bit for bit all
# go through one kernel; tests/golden/field_pins.npz holds what the library gave for the states of diag_pins.npz when the
# fixture was recorded (tests/golden/make_field_pins.py): the bits may not move.  The states: n = 1, 129, 256, 300, bodies 5
# and 200 of the last at one position.  The 257 points (two workgroups, the second ragged) are part of the fixture, one
# set per precision, point 100 exactly on body 5 of that precision's n = 300 state: its chains are NaN, the general code
# answers and counts both bodies.
# ---------------------------------------------------------------------------------------------------------------------
FIELD_PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_pins.npz")
FIELD_PIN_POINTS = 257
FIELD_PIN_ON_BODY = (100, 5)                                    # (point, body of the n = 300 state)
FIELD_PIN_BATCH_CAPACITY = 300


def pin_field_points(nb, states, precision):
    """The fixture's point set of one precision, made once by the generator."""
    pts = probe_points(nb.stock_config(particleCount=dg.PIN_SIZES[-1]), FIELD_PIN_POINTS, 31 + precision)
    point, body = FIELD_PIN_ON_BODY
    pts[point] = dg.pin_bodies(nb, states, precision, dg.PIN_SIZES[-1]).Positions[body].astype(np.float64)
    return {"points_" + dg.pin_tag(nb, precision): dg.pin_bits(pts)}


def pin_field_result(tag, f):
    return {tag + "_acc": dg.pin_bits(f["acc"]), tag + "_phi": dg.pin_bits(f["phi"]),
            tag + "_coincident": np.asarray(f["coincident"], dtype=np.int64).reshape(-1)}


def pin_field_stepper(nb, states, pins, precision, n):
    """-> {key: bits} of field() and field(points) straight after the upload."""
    tag = "ctx_%s_n%d" % (dg.pin_tag(nb, precision), n)
    pts = pins["points_" + dg.pin_tag(nb, precision)].view(np.float64)
    with nb.Stepper(nb.stock_config(particleCount=n), precision=precision) as st:
        st.upload(dg.pin_bodies(nb, states, precision, n))
        return {**pin_field_result(tag + "_own", st.field()), **pin_field_result(tag + "_points", st.field(pts))}


def pin_field_batch(nb, states, pins):
    """One fp32 batch of the systems n = 0, 1, 129, 256, 300 at capacity 300."""
    pts = pins["points_f32"].view(np.float64)
    cfg = nb.stock_config(particleCount=FIELD_PIN_BATCH_CAPACITY)
    with nb.StepperBatch(len(dg.PIN_BATCH_SIZES), FIELD_PIN_BATCH_CAPACITY, cfg=cfg) as b:
        b.upload([dg.pin_bodies(nb, states, nb.F32, n) for n in dg.PIN_BATCH_SIZES])
        return {**pin_field_result("batch_own", b.field()), **pin_field_result("batch_points", b.field(pts))}


@pytest.fixture(scope="module")
def field_pins():
    with np.load(FIELD_PINS) as z:
        return {k: z[k] for k in z.files}


def test_pinned_bits(nb, field_pins):
    with np.load(dg.PINS) as z:
        states = {k: z[k] for k in z.files if k.startswith("in_")}
    got = {}
    for precision in (nb.F32, nb.F64):
        for n in dg.PIN_SIZES:
            got.update(pin_field_stepper(nb, states, field_pins, precision, n))
    got.update(pin_field_batch(nb, states, field_pins))
    assert set(got) | {"points_f32", "points_f64"} == set(field_pins)
    dg.check_pins(field_pins, got)
    # what the inputs were built to reach: the shared position counted from both sides, and the point placed on it counting
    # every body that lies there (the states share their first bodies, so it meets body 5 of the smaller ones too)
    def bodies_at_the_point(precision, n):
        at = field_pins["points_" + dg.pin_tag(nb, precision)].view(np.float64)[FIELD_PIN_ON_BODY[0]]
        return int((dg.pin_bodies(nb, states, precision, n).Positions.astype(np.float64) == at).all(axis=1).sum()) if n else 0

    for precision in (nb.F32, nb.F64):
        tag = "ctx_%s_n300" % dg.pin_tag(nb, precision)
        assert bodies_at_the_point(precision, 300) == 2
        assert got[tag + "_own_coincident"].tolist() == [2], tag
        assert np.isfinite(got[tag + "_points_phi"].view(np.float64)[FIELD_PIN_ON_BODY[0]]), tag
        for n in dg.PIN_SIZES:
            tag = "ctx_%s_n%d" % (dg.pin_tag(nb, precision), n)
            assert got[tag + "_points_coincident"].tolist() == [bodies_at_the_point(precision, n)], tag
    assert got["batch_own_coincident"].tolist() == [0, 0, 0, 0, 2]
    assert got["batch_points_coincident"].tolist() == [bodies_at_the_point(nb.F32, n) for n in dg.PIN_BATCH_SIZES]
    # the batch's n = 300 system is the fp32 context's state: the same bits through the other count policy
    assert np.array_equal(got["batch_points_acc"][4], got["ctx_f32_n300_points_acc"])
    assert np.array_equal(got["batch_own_phi"][4], got["ctx_f32_n300_own_phi"])
