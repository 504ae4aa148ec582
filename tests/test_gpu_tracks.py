"""The track log on the GPU (Stepper / StepperBatch .reserve_tracks, .record_tracks, .tracks, step(track_every=)) against
the numpy model on the CPU oracle (tests/track_cases.py), and its potential column against the existing diagnostics.
Every comparison is bitwise.  Reads the CPU oracle only."""
import ctypes

import numpy as np
import pytest

import lineage_cases as lc
import oracle_lib as ol
import track_cases as tc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -7, -9
SPARE = 16                                                       # capacity above n0: room for an identity nobody has


def params_of(cfg):
    return (cfg.timestep, cfg.growthRate, cfg.fieldWidth, cfg.fieldHeight)


def event_sets(ev):
    return sorted((int(e["step"]), int(e["kind"]), int(e["i"]), int(e["j"])) for e in ev)


def record_run(st, steps=lc.STEPS):
    """A row before the first step and one after each step."""
    st.record_tracks()
    for _ in range(steps):
        st.step(1)
        st.record_tracks()


def status_of(call, *a, **kw):
    with pytest.raises(RuntimeError) as ei:                     # NbodyError
        call(*a, **kw)
    return ei.value.status


# ---------------------------------------------------------------------------------------------------------
# 1. Stepper against the model
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
@pytest.mark.parametrize("n0", lc.DENSE_N0)
def test_stepper_against_model(nb, n0, semantics, precision):
    cfg, bodies, tab = tc.dense_tables(nb, n0, precision, semantics)
    with nb.Stepper(cfg, precision=precision, semantics=semantics, track_ids=True) as st:
        st.reserve_tracks(lc.STEPS + 1)                         # before the first upload
        st.upload(bodies)
        record_run(st)
        got = st.tracks()
        tc.assert_tables_equal(got, tab, "N0 %d" % n0)
        assert "phi" not in got
        # the last row against the two synchronising calls it replaces
        out, ids = st.download(), st.ids()
        assert np.array_equal(got["index"][-1][ids], np.arange(out.numBodies))
        assert np.array_equal(tc.bits(got["m"][-1][ids]), tc.bits(out.Masses))
        assert np.array_equal(tc.bits(got["vx"][-1][ids]), tc.bits(out.Velocities[:, 0]))
        assert out.numBodies == lc.SURVIVORS[(n0, semantics)]


# ---------------------------------------------------------------------------------------------------------
# 2. selection
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("n0", lc.DENSE_N0)
def test_selection_equals_columns_of_the_full_table(nb, n0, precision):
    cfg, bodies, tab = tc.dense_tables(nb, n0, precision, ol.LITERAL)
    sel = tc.selection_of(tab, n0)
    assert sel[-1] >= n0
    one = sel[2:3]                                              # k = 1
    with nb.Stepper(cfg, capacity=n0 + SPARE, precision=precision, track_ids=True) as a, \
            nb.Stepper(cfg, capacity=n0 + SPARE, precision=precision, track_ids=True) as b, \
            nb.Stepper(cfg, capacity=n0 + SPARE, precision=precision, track_ids=True) as full:
        a.reserve_tracks(lc.STEPS + 1, ids=sel)
        b.reserve_tracks(lc.STEPS + 1, ids=one)
        full.reserve_tracks(lc.STEPS + 1)
        for st in (a, b, full):
            st.upload(bodies)
            record_run(st)
        tc.assert_tables_equal(a.tracks(), tab.columns(sel), "selection %s" % sel)
        tc.assert_tables_equal(b.tracks(), tab.columns(one), "k = 1: %s" % one)
        got = full.tracks()                                     # capacity n0 + SPARE columns, trimmed to the upload
        tc.assert_tables_equal(got, tab, "all columns of a larger capacity")
        ga = a.tracks()
        for c, k in enumerate(sel[:-1]):
            assert np.array_equal(ga["index"][:, c], got["index"][:, k])
            assert np.array_equal(tc.bits(ga["x"][:, c]), tc.bits(got["x"][:, k]))
        assert np.all(ga["index"][:, -1] == -1)


# ---------------------------------------------------------------------------------------------------------
# 3. potential
# ---------------------------------------------------------------------------------------------------------
def check_phi(got, phis, what):
    """Row s of the log against the diagnostics taken at the same moment; absent columns hold +0."""
    assert got["phi"].dtype == np.float64 and len(got["phi"]) == len(phis), what
    checked = 0
    for s, ref in enumerate(phis):
        idx = got["index"][s]
        here = idx >= 0
        assert got["n_bodies"][s] == len(ref), (what, s)
        assert np.array_equal(tc.bits(got["phi"][s][here]), tc.bits(ref[idx[here]])), (what, s)
        assert not tc.bits(got["phi"][s][~here]).any(), (what, s)
        checked += int(here.sum())
    return checked


def phi_run(st, moments):
    """Records a row, and takes the diagnostics of the same moment, after each of the step counts in `moments`."""
    phis, done = [], 0
    for t in moments:
        st.step(t - done)
        done = t
        st.record_tracks()
        phis.append(st.diagnostics(potential=True)["phi"])
    return phis


PHI_CASES = {
    # one wave, three different self tiles
    "n257-three-tiles": (257, [0, 128, 256], (0, 1)),
    # two workgroups, ragged last tile; after two steps the count is ragged again and the ids are sparse
    "n300-all": (300, None, (0, 2)),
    "n1-all": (1, None, (0, 1)),
    # after merges: the dense N = 1500 run at step 8
    "n1500-step8-all": (1500, None, (8,)),
    "n1500-step8-selection": (1500, "model", (0, 8)),
}


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", sorted(PHI_CASES))
def test_potential_equals_diagnostics(nb, case, precision):
    n0, sel, moments = PHI_CASES[case]
    if n0 in lc.FIELD_OF:
        cfg, bodies = lc.dense_bodies(nb, n0, precision)
    else:
        cfg = nb.stock_config(particleCount=n0, fieldWidth=2000, fieldHeight=2000)
        bodies = nb.init_bodies(cfg, precision, seed=lc.SEED)
    if isinstance(sel, str):
        sel = tc.selection_of(tc.dense_tables(nb, n0, precision, ol.LITERAL)[2], n0)
    with nb.Stepper(cfg, capacity=n0 + SPARE, precision=precision, track_ids=True) as st:
        st.reserve_tracks(len(moments), ids=sel, potential=True)
        st.upload(bodies)
        phis = phi_run(st, moments)
        got = st.tracks()
        checked = check_phi(got, phis, case)
        assert checked > 0
        if sel is None:
            assert checked == sum(len(p) for p in phis)         # every current body was a present column
        if n0 == 1500:
            assert got["n_bodies"][-1] == lc.SURVIVORS[(1500, ol.LITERAL)]
            assert (got["index"][-1] < 0).any() and (got["index"][-1] >= 0).any()
        if n0 == 257:
            assert np.array_equal(got["index"][0], [0, 128, 256])


def test_potential_of_coincident_bodies_takes_the_general_rows(nb):
    """N = 130, fp32, radii 0, growth 0, bodies 3 and 129 at one position: their rows are not finite in the fast chain and
    are redone by the general code, coincident pairs left out; row 64 stays on the fast chain."""
    cfg = nb.stock_config(particleCount=130, radiusGrowthRate=0.0)
    bodies = nb.init_bodies(cfg, seed=lc.SEED)
    bodies.Radii[:] = 0.0
    bodies.Positions[129] = bodies.Positions[3]
    with nb.Stepper(cfg, track_ids=True) as st, nb.Stepper(cfg, track_ids=True) as full:
        st.reserve_tracks(1, ids=[3, 64, 129], potential=True)
        full.reserve_tracks(1, potential=True)
        for s in (st, full):
            s.upload(bodies)
            s.record_tracks()
        d = st.diagnostics(potential=True)
        assert d["coincident_pairs"] == 2 and np.all(np.isfinite(d["phi"]))
        got, gf = st.tracks(), full.tracks()
        assert np.array_equal(got["index"][0], [3, 64, 129])
        assert np.array_equal(tc.bits(got["phi"][0]), tc.bits(d["phi"][[3, 64, 129]]))
        assert np.array_equal(tc.bits(gf["phi"][0]), tc.bits(d["phi"]))
        assert np.array_equal(tc.bits(got["x"][0][[0]]), tc.bits(got["x"][0][[2]]))


# ---------------------------------------------------------------------------------------------------------
# 4. protocol
# ---------------------------------------------------------------------------------------------------------
def test_track_every_equals_the_stepwise_run(nb):
    cfg, bodies, tab = tc.dense_tables(nb, 1000, 0, ol.LITERAL)
    with nb.Stepper(cfg, track_ids=True) as st:
        st.reserve_tracks(8)
        st.upload(bodies)
        st.record_tracks()
        st.step(8, track_every=2)
        tc.assert_tables_equal(st.tracks(), tab.every(2), "track_every=2")
        st.upload(bodies)
        st.step(8, track_every=3)                               # rows after steps 3 and 6, none at 8, none before the first
        got = st.tracks()
        assert np.array_equal(got["step"], [3, 6]) and np.array_equal(got["index"], tab.index[[3, 6]])
        with pytest.raises(ValueError):
            st.step(1, track_every=-1)
    sizes = [300, 1000]
    cfgs = [lc.dense_cfg(nb, n) for n in sizes]
    bds = [nb.init_bodies(c, seed=lc.SEED) for c in cfgs]
    with nb.StepperBatch(2, 1000, params=[params_of(c) for c in cfgs], track_ids=True) as b:
        b.reserve_tracks(8)
        b.reserve_diagnostics(8)
        b.upload(bds)
        b.record_tracks()
        b.step(8, record_every=4, track_every=2)                # both series in one loop
        got = b.tracks()
        assert len(b.diagnostics_log()) == 2 and np.array_equal(b.diagnostics_log()["step"][:, 0], [4, 8])
        for s, n0 in enumerate(sizes):
            want = tc.dense_tables(nb, n0, 0, ol.LITERAL)[2].every(2)
            sys_s = {k: v[:, s] for k, v in got.items()}
            assert np.array_equal(sys_s["step"], want.step) and np.array_equal(sys_s["n_bodies"], want.n_bodies)
            assert np.array_equal(sys_s["index"][:, :n0], want.index) and np.all(sys_s["index"][:, n0:] == -1)
            for f in tc.FIELDS:
                assert np.array_equal(tc.bits(sys_s[f][:, :n0]), tc.bits(want.rec[f])), (s, f)


def test_full_log_upload_and_release(nb):
    cfg, bodies, tab = tc.dense_tables(nb, 300, 0, ol.LITERAL)
    with nb.Stepper(cfg, track_ids=True) as st:
        st.reserve_tracks(2, potential=True)
        st.upload(bodies)
        st.record_tracks()
        st.step(1)
        st.record_tracks()
        before = st.tracks()
        st.step(1)
        assert status_of(st.record_tracks) == CAPACITY         # found on the host: nothing enqueued
        after = st.tracks()
        assert sorted(before) == sorted(after) and len(after["step"]) == 2
        for k in before:
            assert np.array_equal(tc.bits(before[k]) if before[k].dtype.kind == "f" else before[k],
                                  tc.bits(after[k]) if after[k].dtype.kind == "f" else after[k]), k
        assert np.array_equal(after["index"], tab.index[:2])
        # an upload restarts at row 0 and keeps the reservation
        st.upload(bodies)
        assert len(st.tracks()["step"]) == 0
        st.record_tracks()
        got = st.tracks()
        assert np.array_equal(got["step"], [0]) and np.array_equal(got["index"][0], np.arange(300)) and "phi" in got
        # a smaller read than the log
        st.record_tracks()
        rows = np.zeros(1, dtype=nb.TRACK_ROW_DTYPE)
        n, cols = ctypes.c_int(0), ctypes.c_int(0)
        assert nb.lib.nbody_track_read(st._ctx, rows.ctypes.data, None, None, None, 1, ctypes.byref(n), ctypes.byref(cols)) == 0
        assert (n.value, cols.value) == (2, 300) and rows["n_bodies"][0] == 300
        # a re-reservation empties the log; without the potential, asking for it is a state error
        st.reserve_tracks(3)
        assert len(st.tracks()["step"]) == 0
        phi = np.zeros(900)
        assert nb.lib.nbody_track_read(st._ctx, None, None, None, phi.ctypes.data, 3, ctypes.byref(n), ctypes.byref(cols)) == STATE
        # reserve(0) frees the log
        st.reserve_tracks(0)
        assert status_of(st.record_tracks) == STATE
        assert len(st.tracks()["step"]) == 0
        st.step(1)                                              # and the context steps on
        assert st.body_count() == tab.n_bodies[1]


def test_errors(nb):
    cfg, bodies = lc.dense_bodies(nb, 300)
    with nb.Stepper(cfg, record_events=True) as plain, nb.Stepper(cfg, track_ids=True) as st:
        plain.upload(bodies)
        assert status_of(plain.reserve_tracks, 4) == STATE     # without track_ids
        assert status_of(plain.record_tracks) == STATE
        assert status_of(plain.tracks) == STATE
        assert status_of(st.record_tracks) == STATE            # no reservation, no upload
        st.reserve_tracks(4)
        assert status_of(st.record_tracks) == STATE            # before an upload
        st.upload(bodies)
        st.record_tracks()
        for ids in ([5, 3], [3, 3], [-1, 3], [3, 300], [0, 1, 2, 1], []):
            assert status_of(st.reserve_tracks, 4, ids=ids) == INVALID, ids
        assert status_of(st.reserve_tracks, -1) == INVALID
        assert nb.lib.nbody_track_reserve(st._ctx, 4, None, 0, 2) == INVALID           # unknown fields
        assert nb.lib.nbody_track_reserve(st._ctx, 1 << 30, None, 0, 0) == INVALID      # above 2^31 bytes
        got = st.tracks()                                       # a refused reservation leaves the log as it was
        assert np.array_equal(got["step"], [0]) and got["index"].shape == (1, 300)
    with nb.StepperBatch(2, 300, cfg=cfg) as plain, nb.StepperBatch(2, 300, cfg=cfg, track_ids=True) as b:
        assert status_of(plain.reserve_tracks, 4) == STATE
        assert status_of(b.record_tracks) == STATE
        b.reserve_tracks(1, ids=[0, 299])
        assert status_of(b.record_tracks) == STATE             # before an upload
        for ids in ([5, 3], [3, 3], [-1], [300], []):
            assert status_of(b.reserve_tracks, 4, ids=ids) == INVALID, ids
        assert status_of(b.reserve_tracks, -1) == INVALID
        assert nb.lib.nbody_batch_track_reserve(b._b, 4, None, 0, 2) == INVALID
        b.upload([bodies, bodies])
        b.record_tracks()
        assert status_of(b.record_tracks) == CAPACITY
        got = b.tracks()
        assert got["index"].shape == (1, 2, 2) and np.array_equal(got["index"][0], [[0, 299], [0, 299]])
        b.reserve_tracks(0)
        assert status_of(b.record_tracks) == STATE


# ---------------------------------------------------------------------------------------------------------
# 5. recording never changes stepping
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,variant", [(0, 0), (0, 31), (0, 50), (0, 1), (1, 0), (1, 1)])
def test_recording_does_not_change_the_step(nb, precision, variant):
    cfg, bodies = lc.dense_bodies(nb, 1500, precision)
    kw = dict(precision=precision, kernel_variant=variant, record_events=True, track_ids=True)
    with nb.Stepper(cfg, **kw) as a, nb.Stepper(cfg, **kw) as b:
        a.reserve_tracks(lc.STEPS + 1, potential=True)
        a.upload(bodies)
        b.upload(bodies)
        a.record_tracks()
        a.step(lc.STEPS, track_every=1)
        b.step(lc.STEPS)
        ga, gb = a.download(), b.download()
        assert ga.numBodies == gb.numBodies == lc.SURVIVORS[(1500, ol.LITERAL)]
        assert np.array_equal(tc.bits(ga.block), tc.bits(gb.block))
        assert np.array_equal(a.ids(), b.ids())
        assert event_sets(a.events()) == event_sets(b.events()) and len(a.events()) > 0
        assert a.stats().pairs == b.stats().pairs
        assert len(a.tracks()["step"]) == lc.STEPS + 1


# ---------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_tables(nb, semantics):
    """32 mixed dense systems (sizes of lineage_cases.FIELD_OF), an empty one and one of 1500 bodies (the three-launch
    step) among them: all columns and a selection, phi against StepperBatch.diagnostics."""
    rng = np.random.RandomState(40 + semantics)
    sizes = [0, 77, 130, 300, 1000, 1024, 1500] + [int(x) for x in rng.choice(sorted(lc.FIELD_OF), 25)]
    S, cap = len(sizes), 1500 + SPARE
    assert S == 32
    cfgs = [nb.stock_config(particleCount=max(n, 1), fieldWidth=lc.FIELD_OF.get(n, 1000), fieldHeight=lc.FIELD_OF.get(n, 1000),
                            timestep=float(np.float32(0.2 + 0.01 * (s % 3))),
                            growthRate=float(np.float32(0.1 + 0.05 * (s % 2))))
            for s, n in enumerate(sizes)]
    bodies = [nb.init_bodies(cfg, seed=7100 + s) if n else nb.BodiesData(0) for s, (n, cfg) in enumerate(zip(sizes, cfgs))]
    sel = np.array([0, 5, 76, 77, 129, 299, 1023, 1499, 1500 + 5], dtype=np.int32)
    rows = lc.STEPS + 1
    singles = {s: nb.Stepper(cfgs[s], capacity=cap, semantics=semantics, track_ids=True) for s in range(S) if sizes[s]}
    try:
        for s, st in singles.items():
            st.reserve_tracks(rows)
            st.upload(bodies[s])
        kw = dict(params=[params_of(c) for c in cfgs], semantics=semantics, track_ids=True)
        with nb.StepperBatch(S, cap, **kw) as ball, nb.StepperBatch(S, cap, **kw) as bsel:
            ball.reserve_tracks(rows, potential=True)
            bsel.reserve_tracks(rows, ids=sel, potential=True)
            ball.upload(bodies)
            bsel.upload(bodies)
            diags = []
            for t in range(rows):
                if t:
                    for x in list(singles.values()) + [ball, bsel]:
                        x.step(1)
                for x in list(singles.values()) + [ball, bsel]:
                    x.record_tracks()
                diags.append(ball.diagnostics(potential=True))
            ga, gs = ball.tracks(), bsel.tracks()
            assert ga["index"].shape == (rows, S, cap) and gs["index"].shape == (rows, S, len(sel))
            assert ga["step"].shape == (rows, S)
            deleted = 0
            for s, n0 in enumerate(sizes):
                what = "system %d (N0 = %d)" % (s, n0)
                mine = {k: v[:, s] for k, v in ga.items()}
                assert np.all(mine["index"][:, n0:] == -1), what
                for f in tc.FIELDS + ("phi",):
                    assert not tc.bits(mine[f][:, n0:]).any(), (what, f)
                assert np.array_equal(mine["step"], np.arange(rows)), what
                if n0 == 0:
                    assert not mine["n_bodies"].any(), what
                    continue
                want = singles[s].tracks()
                assert want["index"].shape == (rows, n0)
                assert np.array_equal(mine["n_bodies"], want["n_bodies"]) and np.array_equal(mine["step"], want["step"]), what
                assert np.array_equal(mine["index"][:, :n0], want["index"]), what
                for f in tc.FIELDS:
                    assert np.array_equal(tc.bits(mine[f][:, :n0]), tc.bits(want[f])), (what, f)
                check_phi({k: mine[k] for k in ("index", "phi", "n_bodies")}, [d[s]["phi"] for d in diags], what)
                deleted += n0 - int(mine["n_bodies"][-1])
                # the selection: those columns of the all-columns table
                picked = {k: v[:, s] for k, v in gs.items()}
                assert np.array_equal(picked["n_bodies"], mine["n_bodies"]), what
                for k in ("index", "phi") + tc.FIELDS:
                    col = mine[k][:, sel]
                    assert np.array_equal(tc.bits(picked[k]) if col.dtype.kind == "f" else picked[k],
                                          tc.bits(col) if col.dtype.kind == "f" else col), (what, k)
            assert deleted > sum(sizes) / 3                     # the systems did merge meanwhile
            assert singles[6].body_count() == int(ga["n_bodies"][-1, 6]) < 1500
    finally:
        for st in singles.values():
            st.close()
