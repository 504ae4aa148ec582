"""Per-system diagnostics of a batch (StepperBatch.diagnostics / nbody_batch_diagnostics) and the recorded series
(nbody_batch_diag_*) on the GPU.  System s of a batch reports, bit for bit, what a Stepper holding the same state reports:
zero tolerance wherever product is compared with product; the long-double oracle and the derived bounds of
test_gpu_diagnostics.py where it is not."""
import ctypes

import numpy as np
import pytest

from test_gpu_batch import FIELD_OF, params_of
from test_gpu_diagnostics import bodies_with_velocities, check_phi, check_totals, diag_bits, exact_phi, state_arrays

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 77, 127, 128, 129, 130, 255, 256, 257, 300, 1000, 1024, 1025, 1500, 4096]
CAPACITY_ERR, STATE_ERR = -7, -9


def ensemble(nb, sizes, seed0=100):
    """Per system: the dense field of FIELD_OF where it has the size (collisions in every step), seeded random velocities,
    a time step and a growth rate of its own."""
    cfgs, bodies = [], []
    for s, n in enumerate(sizes):
        field = FIELD_OF.get(n, 3000 if n <= 300 else 8000)
        cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field,
                              timestep=float(np.float32(0.2 + 0.01 * (s % 3))),
                              growthRate=float(np.float32(0.1 + 0.05 * (s % 2))))
        b = nb.init_bodies(cfg, seed=seed0 + s)
        b.Velocities[:] = np.random.default_rng(seed0 + s).uniform(-3, 3, size=(n, 2)).astype(np.float32)
        cfgs.append(cfg)
        bodies.append(b)
    return cfgs, bodies


def state_bits(b):
    """Everything a batch holds that a read must not change: states, counts, pair counters, events."""
    out = [tuple(int(c) for c in b.counts())]
    for s in range(b.systems):
        d = b.download(s)
        out.append((d.numBodies, d.block.view(np.uint32).tobytes(), b.stats(s).pairs, b.stats(s).steps))
    return out


def log_row_bits(row):
    """A row of the recorded series (S records) in the form of diag_bits without phi."""
    out = []
    for r in row:
        vals = [int(r["step"]), int(r["n_bodies"]), int(r["coincident_pairs"])]
        for k in ("mass", "momentum", "center_of_mass", "angular_momentum", "kinetic", "potential"):
            vals += [int(e) for e in np.atleast_1d(r[k]).view(np.uint64)]
        out.append(tuple(vals))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. equals Stepper, 2. and the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_every_system_equals_its_stepper(nb, semantics):
    """Sixteen sizes around the tile and workgroup edges in one batch, at upload and after each of four steps: the counts
    shrink through collisions, so the grid sized at upload is larger than the live systems.  N = 1000 and N = 1500 are
    also held against the long-double oracle on the downloaded state."""
    cfgs, bodies = ensemble(nb, SIZES)
    singles = [nb.Stepper(cfg, semantics=semantics) for cfg in cfgs]
    for st, bd in zip(singles, bodies):
        st.upload(bd)
    with nb.StepperBatch(len(SIZES), max(SIZES), params=[params_of(c) for c in cfgs], semantics=semantics) as b:
        b.upload(bodies)
        shrunk = 0
        for k in range(5):
            if k:
                b.step(1)
                for st in singles:
                    st.step(1)
            got = b.diagnostics(potential=True)
            plain = b.diagnostics()
            assert len(got) == len(SIZES)
            for s, st in enumerate(singles):
                what = "N0 = %d, step %d" % (SIZES[s], k)
                want = st.diagnostics(potential=True)
                assert got[s]["step"] == k and got[s]["n_bodies"] == want["n_bodies"], what
                assert len(got[s]["phi"]) == want["n_bodies"], what
                assert diag_bits(got[s]) == diag_bits(want), what
                assert diag_bits(plain[s]) == diag_bits(want)[:-1], what          # without phi: the same totals
            for s in (SIZES.index(1000), SIZES.index(1500)):                        # not only product against product
                state = b.download(s)
                n = state.numBodies
                P, V, M = state_arrays(state)
                want_phi, coincident = exact_phi(P, M, np.arange(n))
                what = "oracle, N0 = %d, step %d" % (SIZES[s], k)
                check_phi(got[s]["phi"], want_phi, n, what)
                assert got[s]["coincident_pairs"] == coincident, what
                check_totals(got[s], P, V, M, want_phi, what)
            shrunk = sum(g["n_bodies"] < n0 for g, n0 in zip(got, SIZES))
        assert shrunk >= 4, shrunk                               # the fields are dense: systems did lose bodies
    for st in singles:
        st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. isolation
# ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_systems_side_by_side(nb):
    """Coincident bodies at zero radii, a NaN mass, a single body, an empty system and an ordinary one in one batch: the
    general path, the NaN and the empty grid rows stay inside their system."""
    n = 2048
    r0 = dict(particleCount=n, minRadius=0.0, maxRadius=0.0)
    cfg0 = nb.stock_config(**r0)
    _, twins = bodies_with_velocities(nb, n, nb.F32, seed=21)
    twins.Radii[:] = 0
    P = twins.Positions
    P[70] = P[5]                      # same tile, same wave
    P[200] = P[130]                   # same tile, other half
    P[1000] = P[300]                  # across tiles
    P[2040] = P[3]
    P[1500] = P[1501] = P[1502]       # three on one point
    P[129] = P[128]
    _, nanm = bodies_with_velocities(nb, n, nb.F32, seed=22)
    nanm.Masses[1300] = np.nan
    one = nb.BodiesData.from_arrays([[1.5, -2.0]], [[0.5, 0.25]], [3.0], [1.0], nb.F32)
    empty = nb.BodiesData(0)
    plain_cfg, plain = bodies_with_velocities(nb, 1500, nb.F32, seed=23, field=6000)
    bodies = [twins, nanm, one, empty, plain]
    cfgs = [cfg0, cfg0, cfg0, cfg0, plain_cfg]
    with nb.StepperBatch(5, n, params=[params_of(c) for c in cfgs]) as b:
        phi_all = np.full(5 * n, -777.0)                       # the C call: slices past a system's count stay as they are
        out = (nb.Diag * 5)()
        b.upload(bodies)
        for k in range(3):
            if k:
                b.step(1)
            got = b.diagnostics(potential=True)
            for s in (0, 1, 2, 4):
                with nb.Stepper(cfgs[s], capacity=n) as st:    # the twin holds the batch's own state of this step
                    state = b.download(s)
                    st.upload(state)
                    want = st.diagnostics(potential=True)
                want["step"] = k                               # a fresh upload counts from 0; the batch from its own upload
                g, w = diag_bits(got[s]), diag_bits(want)
                if s == 1:                                     # NaN payloads: equal where neither is NaN, NaN where one is
                    assert got[s]["n_bodies"] == want["n_bodies"] and got[s]["coincident_pairs"] == want["coincident_pairs"]
                    for key in ("mass", "angular_momentum", "kinetic", "potential"):
                        assert np.isnan(got[s][key]) == np.isnan(want[key]), (key, k)
                        assert np.isnan(want[key]) or got[s][key] == want[key], (key, k)
                    both = np.isnan(got[s]["phi"]) & np.isnan(want["phi"])
                    assert np.array_equal(got[s]["phi"][~both].view(np.uint64), want["phi"][~both].view(np.uint64)), k
                    assert np.isnan(got[s]["mass"]) and both.sum() >= state.numBodies - 1
                else:
                    assert g == w, "system %d step %d" % (s, k)
            if k == 0:
                Pd, V, M = state_arrays(twins)
                want_phi, coincident = exact_phi(Pd, M, np.arange(n))
                assert coincident == 2 * 5 + 6 and got[0]["coincident_pairs"] == coincident
                check_phi(got[0]["phi"], want_phi, n, "coincident system")
                check_totals(got[0], Pd, V, M, want_phi, "coincident system")
                assert got[2]["phi"][0] == 0 and got[2]["mass"] == 3.0 and got[2]["center_of_mass"] == (1.5, -2.0)
            e = got[3]                                         # the empty system: the header's rule for mass == 0
            assert (e["step"], e["n_bodies"], e["coincident_pairs"]) == (k, 0, 0) and len(e["phi"]) == 0
            for key in ("mass", "angular_momentum", "kinetic", "potential"):
                assert e[key] == 0.0 and not np.signbit(e[key]), key
            assert all(v == 0.0 and not np.signbit(v) for v in e["momentum"])
            assert all(np.isnan(v) for v in e["center_of_mass"])
            phi_all[:] = -777.0
            assert nb.lib.nbody_batch_diagnostics(b._b, out, phi_all.ctypes.data) == 0
            for s in range(5):
                cur = out[s].n_bodies
                assert np.array_equal(phi_all[s * n:s * n + cur].view(np.uint64), got[s]["phi"].view(np.uint64)), s
                assert np.all(phi_all[s * n + cur:(s + 1) * n] == -777.0), s


# ---------------------------------------------------------------------------------------------------------------------
# 4. reads only
# ---------------------------------------------------------------------------------------------------------------------
def test_diagnostics_and_records_change_nothing(nb):
    sizes = [300, 1000, 1500, 130, 1024, 77]
    cfgs, bodies = ensemble(nb, sizes, seed0=300)
    kw = dict(params=[params_of(c) for c in cfgs], record_events=True)
    with nb.StepperBatch(len(sizes), max(sizes), **kw) as a, nb.StepperBatch(len(sizes), max(sizes), **kw) as c:
        a.upload(bodies)
        c.upload(bodies)
        c.reserve_diagnostics(8)
        c.diagnostics(potential=True)
        for k in range(6):
            a.step(1)
            c.step(1)
            c.record_diagnostics()
            if k % 2:
                c.diagnostics(potential=bool(k & 2))
        assert state_bits(a) == state_bits(c)
        for s in range(len(sizes)):
            ea, ec = a.events(s, cap=1 << 16), c.events(s, cap=1 << 16)
            assert sorted(map(tuple, ea.tolist())) == sorted(map(tuple, ec.tolist())), s
        assert sum(len(a.events(s, cap=1 << 16)) for s in range(len(sizes))) > 0
        assert len(c.diagnostics_log()) == 6


# ---------------------------------------------------------------------------------------------------------------------
# 5. the recorded series
# ---------------------------------------------------------------------------------------------------------------------
def test_recorded_series_equals_diagnostics_at_the_same_steps(nb):
    sizes = [1000, 1500, 300, 1024, 130, 257, 1, 4096]
    cfgs, bodies = ensemble(nb, sizes, seed0=500)
    S, nsteps, every = len(sizes), 11, 3
    kw = dict(params=[params_of(c) for c in cfgs])
    with nb.StepperBatch(S, max(sizes), **kw) as b, nb.StepperBatch(S, max(sizes), **kw) as twin:
        b.upload(bodies)
        twin.upload(bodies)
        with pytest.raises(nb.NbodyError) as ei:               # no reservation yet
            b.record_diagnostics()
        assert ei.value.status == STATE_ERR
        b.reserve_diagnostics(4)
        assert b.diagnostics_log().shape == (0, S)
        b.record_diagnostics()                                 # row 0: the uploaded state
        b.step(nsteps, record_every=every)                     # rows 1..3: after steps 3, 6, 9; then two more steps
        want_rows = [twin.diagnostics()]
        for i in range(1, nsteps + 1):
            twin.step(1)
            if i % every == 0:
                want_rows.append(twin.diagnostics())
        log = b.diagnostics_log()
        assert log.dtype == nb.DIAG_DTYPE and log.shape == (4, S)
        for k, want in enumerate(want_rows):
            assert log_row_bits(log[k]) == [diag_bits(w) for w in want], "row %d" % k
            assert [int(x) for x in log[k]["step"]] == [every * k] * S
        counts = b.counts()
        assert [int(x) for x in log[3]["n_bodies"]] != [int(x) for x in log[0]["n_bodies"]]   # systems lost bodies
        assert [int(x) for x in log[0]["n_bodies"]] == sizes
        assert all(int(c) <= int(m) for c, m in zip(counts, log[3]["n_bodies"]))
        # the log is full: the host says so, nothing is enqueued, rows and state stay
        before = state_bits(b)
        with pytest.raises(nb.NbodyError) as ei:
            b.record_diagnostics()
        assert ei.value.status == CAPACITY_ERR
        assert state_bits(b) == before and b.diagnostics_log().tobytes() == log.tobytes()
        with pytest.raises(nb.NbodyError) as ei:
            b.step(3, record_every=3)
        assert ei.value.status == CAPACITY_ERR
        twin.step(3)                                           # (that call did enqueue its three steps before the record)
        assert state_bits(b) == state_bits(twin) and before != state_bits(b)
        again = b.diagnostics_log()
        assert again.tobytes() == log.tobytes()
        # the C call: fewer rows than recorded are asked for
        part = np.zeros((2, S), dtype=nb.DIAG_DTYPE)
        n_rec = ctypes.c_int(0)
        assert nb.lib.nbody_batch_diag_read(b._b, part.ctypes.data, 2, ctypes.byref(n_rec)) == 0
        assert n_rec.value == 4 and part.tobytes() == log[:2].tobytes()
        # an upload restarts the log and keeps the reservation
        b.upload(bodies)
        assert b.diagnostics_log().shape == (0, S)
        b.step(2, record_every=1)
        log2 = b.diagnostics_log()
        assert log2.shape == (2, S) and [int(x) for x in log2[1]["step"]] == [2] * S
        twin.upload(bodies)
        twin.step(2)
        assert log_row_bits(log2[1]) == [diag_bits(w) for w in twin.diagnostics()]
        # reserve(0) frees the log; a larger reservation starts empty
        b.reserve_diagnostics(0)
        with pytest.raises(nb.NbodyError) as ei:
            b.record_diagnostics()
        assert ei.value.status == STATE_ERR
        assert b.diagnostics_log().shape == (0, S)
        b.reserve_diagnostics(16)
        assert b.diagnostics_log().shape == (0, S)
        b.record_diagnostics()
        assert log_row_bits(b.diagnostics_log()[0]) == [diag_bits(w) for w in twin.diagnostics()]
        for bad in (-1, 1 << 30):                              # negative, and far above 2^31 bytes
            with pytest.raises(nb.NbodyError) as ei:
                b.reserve_diagnostics(bad)
            assert ei.value.status == -1
    with nb.StepperBatch(2, 64, cfg=nb.stock_config(particleCount=64)) as fresh:   # before the first upload
        fresh.reserve_diagnostics(2)
        with pytest.raises(nb.NbodyError) as ei:
            fresh.record_diagnostics()
        assert ei.value.status == STATE_ERR
        with pytest.raises(nb.NbodyError) as ei:
            fresh.diagnostics()
        assert ei.value.status == STATE_ERR


# ---------------------------------------------------------------------------------------------------------------------
# 6. extremes of S, and the force kernel does not matter
# ---------------------------------------------------------------------------------------------------------------------
def test_four_thousand_systems_of_64(nb):
    S, n = 4096, 64
    cfg = nb.stock_config(particleCount=n, fieldWidth=1000, fieldHeight=1000)
    bodies = []
    for s in range(S):
        b = nb.init_bodies(cfg, seed=9000 + s)
        b.Velocities[:] = np.random.default_rng(s).uniform(-3, 3, size=(n, 2)).astype(np.float32)
        bodies.append(b)
    with nb.StepperBatch(S, n, cfg=cfg) as b:
        b.upload(bodies)
        b.reserve_diagnostics(2)
        b.step(3, record_every=3)
        got = b.diagnostics(potential=True)
        log = b.diagnostics_log()
        assert log_row_bits(log[0]) == [diag_bits(g)[:-1] for g in got]
        assert sum(g["n_bodies"] < n for g in got) > 0
        for s in (0, 1, 63, 64, 2047, 4095):
            with nb.Stepper(cfg) as st:
                st.upload(bodies[s])
                st.step(3)
                assert diag_bits(st.diagnostics(potential=True)) == diag_bits(got[s]), s


@pytest.mark.parametrize("lanes", [1, 4])
def test_one_system_of_4096_whatever_the_force_kernel(nb, lanes):
    cfg, bodies = bodies_with_velocities(nb, 4096, nb.F32, seed=31, field=8000)
    with nb.StepperBatch(1, 4096, cfg=cfg, kernel_variant=lanes) as b, nb.Stepper(cfg) as st:
        assert "%d lane" % lanes in b.kernel_name()
        b.upload([bodies])
        st.upload(bodies)
        for k in range(3):
            if k:
                b.step(2)
                st.step(2)
            want = st.diagnostics(potential=True)
            assert diag_bits(b.diagnostics(potential=True)[0]) == diag_bits(want), k
        assert want["n_bodies"] < 4096
