"""Shell moments (nbody_get_shell_moments, nbody_batch_get_shell_moments; Stepper.shell_moments, StepperBatch.shell_moments) on
the MI355X: nine fp64 sums and a count over the bodies in each bin of distance around every body or moving probe point.

The definition has no fma, no divide and no square root, rounds every operation on its own and fixes the order of every sum,
so the numpy model of shell_moment_cases.py restates it bit for bit: zero tolerance throughout - the nine sums by their bits,
count and pad exactly - against the model, and product against product (nbody_get_shells, nbody_get_pair_counts, a batch
against a Stepper holding the same state) the same way.  The masses of moment_state span 1e4 .. 1e17 and the velocities are
signed: test_shell_moment_cases_cpu.py asserts that each of the nine sums changes with the order, so a kernel that adds in
another order, or re-associates, or contracts a multiply and an add, fails the comparisons here."""
import ctypes

import numpy as np
import pytest

import shell_moment_cases as smc
from test_gpu_batch import params_of
from test_gpu_neighbors import dense_bodies, dense_field

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
DTYPE_OF = {0: np.float32, 1: np.float64}
INF = np.inf
WHOLE = np.array([0.0, INF])


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=capacity, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, V, M, precision):
    n = len(P)
    return nb.BodiesData.from_arrays(P, V, M, np.full(n, 0.25), precision) if n else nb.BodiesData(0, precision)


def check(st, P, V, M, edges2, what, points=None, point_vel=None):
    """shell_moments on the resident state, squared edges, against the model of (P, V, M); -> the moments."""
    got = st.shell_moments(edges2, points=points, point_vel=point_vel, squared=True)
    rows = len(P) if points is None else len(points)
    assert got["moments"].shape == (rows, len(edges2) - 1), what
    smc.assert_same(got, smc.model_shell_moments(P, V, M, edges2, points, point_vel), what)
    return got["moments"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
# 63 .. 65: the self tile's checked loop ends inside tile 0; 191 .. 193: the third wave, self tile 1; 385: a second workgroup
# whose first wave has self tile 2
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 385])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    P, V, M = smc.moment_state(n, DTYPE_OF[precision])
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        got = check(st, P, V, M, smc.tenth_edges(smc.tenth_field(n)), "n %d, a tenth of the field" % n)
        if n >= 127:
            inside = got["count"].sum(axis=1)
            assert (got["count"].sum(axis=0) > 0).any() and (inside < n - 1).any()     # a bin in use, a source outside
        got = check(st, P, V, M, WHOLE, "n %d, one bin for everything" % n)
        assert (got["count"] == n - 1).all()
        got = check(st, P, V, M, np.array([4.0, 9.0]), "n %d, [4, 9]" % n)
        assert n < 127 or got["count"].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. every tier boundary, and the wrapper's split
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_tier_boundary(nb, precision):
    n, m = 130, 37
    P, V, M = smc.moment_state(n, DTYPE_OF[precision], field=30.0)
    pts = smc.probe_points(P, m, seed=5, field=30.0)
    vel = smc.point_velocities(m, seed=5)
    nout = ctypes.c_int(0)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        seen = {}
        for bins in (1, 2, 4, 5, 8, 9, 17, 32):
            e2 = np.geomspace(0.05, 2500.0, bins + 1)
            own = check(st, P, V, M, e2, "%d geometric bins" % bins)
            exp = check(st, P, V, M, e2, "%d geometric bins, 37 moving points" % bins, points=pts, point_vel=vel)
            assert (own["count"].sum(axis=1) > 0).all() and np.count_nonzero(own["count"].sum(axis=0)) >= min(bins, 4)
            assert (exp["count"][-1] == 0).all() and not smc.bits(exp["ke"][-1]).any()     # a point far outside the field
            seen[bins] = own
            if bins <= smc.SHELL_MOMENTS_MAX:                     # one C call, no wrapper in between
                raw = np.zeros((m, bins), dtype=smc.DTYPE)
                assert nb.lib.nbody_get_shell_moments(st._ctx, pts.ctypes.data, vel.ctypes.data, m, e2.ctypes.data, bins,
                                                      raw.ctypes.data, ctypes.byref(nout)) == 0 and nout.value == m
                smc.assert_same(raw, exp, "%d bins through the C call" % bins)
        # the tier plays no part and bins are independent: the last bin of each set against a call with that one bin alone
        for bins in (4, 5, 8, 9, 17, 32):
            e2 = np.geomspace(0.05, 2500.0, bins + 1)
            k = bins - 1
            alone = st.shell_moments(e2[k:k + 2], squared=True)["moments"]
            smc.assert_same(alone, seen[bins][:, k:k + 1], "the last of %d bins alone" % bins)
        with pytest.raises(ValueError):
            st.shell_moments(np.arange(34.0), squared=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. points form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_points_form(nb, precision):
    n = 300
    field = smc.tenth_field(n)
    P, V, M = smc.moment_state(n, DTYPE_OF[precision])
    e2 = smc.tenth_edges(field)
    allpts = smc.probe_points(P, 257, seed=4, field=field)       # the first 64 ON bodies; points 1 and 255 the same point
    allvel = smc.point_velocities(257, seed=4)
    allvel[255] = allvel[1]
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        for m in (0, 1, 63, 64, 65, 257):                         # 63, 65, 257: a wave past the last row only loads tiles
            moving = check(st, P, V, M, e2, "m %d, moving" % m, points=allpts[:m], point_vel=allvel[:m])
            rest = check(st, P, V, M, e2, "m %d, at rest" % m, points=allpts[:m])
            zeros = st.shell_moments(e2, allpts[:m], np.zeros((m, 2)), squared=True)["moments"]
            smc.assert_same(zeros, rest, "m %d: a point_vel of zeros has the bits of None" % m)
            check(st, P, V, M, WHOLE, "m %d, one bin" % m, points=allpts[:m], point_vel=allvel[:m])
        assert moving["count"].sum() > 0 and smc.differing(moving, rest, "ke") > 0      # moving, rest: m = 257
        assert smc.same(moving[1:2], moving[255:256])             # one point at two places
        one = st.shell_moments(e2, allpts[200:201], allvel[200:201], squared=True)["moments"]
        assert smc.same(one, moving[200:201])                     # alone or among 257: the same bits
        st.upload(nb.BodiesData(0, precision))                    # no bodies left: every record zeroed
        none = (np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0))
        got = check(st, *none, e2, "points over no bodies", points=allpts[:200], point_vel=allvel[:200])
        assert not got.view(np.uint8).any()
        assert check(st, *none, e2, "no bodies").shape == (0, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 4. awkward values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_awkward_values(nb, precision):
    n = 130
    P, V, M = smc.moment_state(n, DTYPE_OF[precision], seed=2, field=30.0)
    wide = np.array([0.0, 25.0, 400.0, INF])
    pts = np.array([[np.nan, 1.0], [3.0, 4.0], [INF, 0.0]])
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        clean = check(st, P, V, M, wide, "finite state, top +inf")
        assert (clean["count"].sum(axis=1) == n - 1).all()
        Pn = P.copy()
        Pn[7, 0] = np.nan                                         # counted nowhere; its own row is empty
        st.upload(bodies_of(nb, Pn, V, M, precision))
        got = check(st, Pn, V, M, wide, "NaN coordinate, top +inf")
        assert (got["count"][7] == 0).all() and (np.delete(got["count"], 7, 0).sum(axis=1) == n - 2).all()
        check(st, Pn, V, M, np.array([1.0, 100.0]), "NaN coordinate, finite top")
        check(st, Pn, V, M, wide, "NaN coordinate, points", points=pts, point_vel=np.array([[1.0, 2.0], [np.nan, 0.0], [0.0, 0.0]]))
        Vn = V.copy()
        Vn[9, 1] = np.nan                                         # a NaN velocity: its bin's sums NaN, the count intact
        st.upload(bodies_of(nb, P, Vn, M, precision))
        got = check(st, P, Vn, M, wide, "a NaN velocity")
        assert np.array_equal(got["count"], clean["count"])
        others = np.arange(n) != 9
        assert (np.isnan(got["ke"][others]).sum(axis=1) == 1).all() and (np.isnan(got["py"][others]).sum(axis=1) == 1).all()
        assert np.array_equal(smc.bits(got["mass"]), smc.bits(clean["mass"])) and np.array_equal(smc.bits(got["mr2"]), smc.bits(clean["mr2"]))
        C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])     # two bodies at one place: d2 = +0
        Vc = np.array([[1.0, 2.0], [0.0, 0.0], [-1.0, 0.5]])
        Mc = np.array([5.0, 7.0, 11.0])
        st.upload(bodies_of(nb, C, Vc, Mc, precision))
        got = check(st, C, Vc, Mc, np.array([0.0, 1.0]), "coincident, first edge 0")
        assert got["count"].tolist() == [[1], [0], [1]] and got["px"].tolist() == [[-22.0], [0.0], [10.0]]
        got = check(st, C, Vc, Mc, np.array([1e-300, 1.0]), "coincident, first edge 1e-300")
        assert not got.view(np.uint8).any()
        Mz = M.copy()
        Mz[9] = 0.0                                               # a body of mass 0 counts and adds zeros
        st.upload(bodies_of(nb, P, V, Mz, precision))
        got = check(st, P, V, Mz, wide, "a body of mass 0")
        assert np.array_equal(got["count"], clean["count"])
        Vz = np.zeros_like(V)                                     # every velocity zero: all velocity sums +0.0, sign bit clear
        st.upload(bodies_of(nb, P, Vz, M, precision))
        for points in (None, P[:40] + 0.25):
            got = check(st, P, Vz, M, wide, "every velocity zero", points=points)
            for f in smc.VELOCITY_FIELDS:
                assert not smc.bits(got[f]).any(), f
            assert got["count"].sum() > 0 and (got["mr2"] > 0).any()
        st.upload(bodies_of(nb, P, np.full_like(V, -0.0), M, precision))               # -0.0 against points at rest
        got = check(st, P, np.full_like(V, -0.0), M, wide, "every velocity -0.0", points=P[:40] + 0.25)
        for f in smc.VELOCITY_FIELDS:
            assert not smc.bits(got[f]).any(), f


# ---------------------------------------------------------------------------------------------------------------------
# 5. products against each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_shells_and_pair_counts(nb, precision):
    n = 300
    field = smc.tenth_field(n)
    P, V, M = smc.moment_state(n, DTYPE_OF[precision])
    pts = smc.probe_points(P, 100, seed=9, field=field)
    vel = smc.point_velocities(100, seed=9)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, V, M, precision))
        for e2 in (smc.tenth_edges(field), np.geomspace(0.5, 4 * field * field, 33), np.array([4.0, 9.0])):
            own = st.shell_moments(e2, squared=True)["moments"]
            exp = st.shell_moments(e2, pts, vel, squared=True)["moments"]
            for mom, sums in ((own, st.shells(e2, squared=True)), (exp, st.shells(e2, pts, squared=True))):
                assert np.array_equal(smc.bits(mom["mass"]), smc.bits(sums["mass"])) and np.array_equal(mom["count"], sums["count"])
            dd, dr = st.pair_counts(e2, squared=True), st.pair_counts(e2, points=pts, squared=True)
            assert own["count"].sum(axis=0, dtype=np.int64).tolist() == (2 * dd["counts"].astype(np.int64)).tolist()
            assert exp["count"].sum(axis=0, dtype=np.int64).tolist() == dr["counts"].astype(np.int64).tolist()
            assert dd["counts"].sum() > 0 and dr["counts"].sum() > 0


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics):
    """n = 1000 dense: the model on the download after each of 3 steps (literal semantics: the frozen tail stays a source
    like any other body).  And a run with calls between the steps downloads the bytes of one without."""
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=7003)
    field = dense_field(n)
    e2 = np.geomspace(4.0, float(field) ** 2 / 4.0, 9)
    pts = smc.probe_points(smc.widen_state(b)[0], 100, seed=4, field=field)
    vel = smc.point_velocities(100, seed=3)

    def run(with_calls):
        counts = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            for s in range(4):
                if s:
                    st.step(1)
                if with_calls:
                    P, V, M = smc.widen_state(st.download())
                    counts.append(len(P))
                    got = check(st, P, V, M, e2, "after %d steps" % s)
                    check(st, P, V, M, e2, "points after %d steps" % s, points=pts, point_vel=vel)
                    assert got["count"][0].sum() > 0 and (s == 0 or np.abs(got["rad"]).max() > 0)   # moving after a step
            d = st.download()
            end = (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                   np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes())
        return end, counts

    plain, _ = run(False)
    called, counts = run(True)
    assert plain == called                                        # state, count, pair counter, events
    assert counts[0] == n and counts[-1] == plain[0] < n and counts == sorted(counts, reverse=True)


# ---------------------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [0, 1, 64, 129, 1024]


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_and_model(nb, semantics):
    cap = 1024
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        cfg, bd = dense_bodies(nb, max(n, 1), seed=40 + s)
        cfgs.append(cfg)
        bodies.append(bd if n else nb.BodiesData(0))
    S = len(BATCH_SIZES)
    batch = nb.StepperBatch(S, cap, params=[params_of(c) for c in cfgs], semantics=semantics)
    batch.upload(bodies)
    one = nb.Stepper(cfgs[-1], capacity=cap, semantics=semantics)
    field = dense_field(cap)
    pts = smc.probe_points(smc.widen_state(bodies[-1])[0], 100, seed=6, field=field)
    vel = smc.point_velocities(100, seed=6)
    for steps, bins in ((0, 5), (3, 8)):
        batch.step(steps)
        e2 = np.geomspace(4.0, float(field) ** 2, bins + 1)
        own, exp, counts = batch.shell_moments(e2, squared=True), batch.shell_moments(e2, pts, vel, squared=True), batch.counts()
        assert len(own) == S and exp["moments"].shape == (S, 100, bins)
        if steps == 0:
            assert counts.tolist() == BATCH_SIZES
        raw = np.full((S, cap, bins * 10), -3.0)                  # the C call into a prefilled buffer: the tails stay
        assert nb.lib.nbody_batch_get_shell_moments(batch._b, None, None, cap, e2.ctypes.data, bins, raw.ctypes.data) == 0
        rec = raw.view(smc.DTYPE).reshape(S, cap, bins)
        for s in range(S):
            n = int(counts[s])
            what = "system %d (n %d), %d bins" % (s, n, bins)
            assert own[s]["moments"].shape == (n, bins), what
            assert smc.same(rec[s, :n], own[s]["moments"]), what
            assert (raw[s, n:] == -3.0).all(), what
            if n == 0:                                            # the empty system: zeroed records
                assert not exp["moments"][s].view(np.uint8).any()
                continue
            d = batch.download(s)
            P, V, M = smc.widen_state(d)
            one.upload(d)
            smc.assert_same(own[s], one.shell_moments(e2, squared=True), what + ": Stepper, own")
            smc.assert_same(exp["moments"][s], one.shell_moments(e2, pts, vel, squared=True), what + ": Stepper, points")
            smc.assert_same(own[s], smc.model_shell_moments(P, V, M, e2), what + ": model, own")
            smc.assert_same(exp["moments"][s], smc.model_shell_moments(P, V, M, e2, pts, vel), what + ": model, points")
        assert own[-1]["moments"]["count"].sum() > 0
        if steps:
            assert int(counts[4]) < cap                           # the dense system has merged bodies by now
    wide = batch.shell_moments(np.geomspace(4.0, float(field) ** 2, 10), pts, squared=True)["moments"]     # 9 bins: two calls
    smc.assert_same(wide[4], one.shell_moments(np.geomspace(4.0, float(field) ** 2, 10), pts, squared=True), "9 bins, split")
    one.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. raw C calls on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_raw_calls(nb):
    n, bins = 300, 4
    P, V, M = smc.moment_state(n, np.float32)
    e2 = np.array([0.0, 9.0, 25.0, 100.0, 400.0])
    b = bodies_of(nb, P, V, M, 0)
    out = np.full((n, bins * 10), 7.0)
    pts = smc.probe_points(P, 4, seed=1, field=smc.tenth_field(n))
    vel = smc.point_velocities(4, seed=1)
    nout = ctypes.c_int(-5)
    call = nb.lib.nbody_get_shell_moments
    E, O, N, PT, PV = e2.ctypes.data, out.ctypes.data, ctypes.byref(nout), pts.ctypes.data, vel.ctypes.data

    def untouched():
        return (out == 7.0).all()

    st = small_stepper(nb, 0, n)
    assert call(st._ctx, None, None, n, E, bins, O, N) == STATE_ERR       # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    bad = np.array([0.0, 9.0, 9.0, 100.0, 400.0])
    assert call(st._ctx, PT, PV, 4, E, 0, O, N) == INVALID
    assert call(st._ctx, PT, PV, 4, np.arange(10.0).ctypes.data, 9, O, N) == INVALID
    assert call(st._ctx, PT, PV, 4, bad.ctypes.data, bins, O, N) == INVALID and b"edges2[2]" in nb.lib.nbody_last_error_string()
    assert call(st._ctx, PT, PV, -1, E, bins, O, N) == INVALID
    assert call(st._ctx, PT, PV, 4, None, bins, O, N) == INVALID
    assert call(st._ctx, PT, PV, 4, E, bins, None, N) == INVALID
    assert call(st._ctx, PT, PV, 4, E, bins, O, None) == INVALID
    assert call(st._ctx, None, PV, n, E, bins, O, N) == INVALID and b"point_vel without points" in nb.lib.nbody_last_error_string()
    assert call(st._ctx, PT, PV, (1 << 31) // (80 * bins) + 1, E, bins, O, N) == INVALID   # m x bins x 80 bytes above 2^31
    assert call(st._ctx, None, None, (1 << 31) // (80 * bins) + 1, E, bins, O, N) == INVALID     # the own form: m as given
    assert call(st._ctx, None, None, n - 1, E, bins, O, N) == CAPACITY_ERR                 # room for fewer than the bodies
    assert untouched() and nout.value == -5
    assert call(st._ctx, PT, PV, 0, E, bins, O, N) == 0 and nout.value == 0                # m == 0 is legal
    assert untouched()
    assert call(st._ctx, None, None, n, E, bins, O, N) == 0 and nout.value == n
    want = smc.model_shell_moments(P, V, M, e2)
    smc.assert_same(out.view(smc.DTYPE).reshape(n, bins), want, "through the C call")
    smc.assert_same(st.shell_moments([0.0, 3.0, 5.0, 10.0, 20.0]), want, "lengths")          # squared=False
    assert st.shell_moments(e2, np.zeros((0, 2)), squared=True)["moments"].shape == (0, bins)
    st.close()
    grp = nb.StepperGroup(2, capacity=n, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    grp.upload(b)
    out[:] = 7.0
    for rank in range(2):                                         # each rank of a group: not built
        assert call(grp.ranks[rank]._ctx, None, None, n, E, bins, O, N) == STATE_ERR
        assert b"single-rank" in nb.lib.nbody_last_error_string()
    assert untouched()
    grp.close()
    batch = nb.StepperBatch(2, n, params=[(0.2, 0.1, 100, 100)] * 2)
    bcall = nb.lib.nbody_batch_get_shell_moments
    out = np.full((2, n, bins * 10), 7.0)
    O = out.ctypes.data
    assert bcall(batch._b, None, None, n, E, bins, O) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, PT, PV, 4, E, 0, O) == INVALID
    assert bcall(batch._b, PT, PV, 4, E, 9, O) == INVALID
    assert bcall(batch._b, PT, PV, 4, bad.ctypes.data, bins, O) == INVALID
    assert bcall(batch._b, PT, PV, -1, E, bins, O) == INVALID
    assert bcall(batch._b, PT, PV, 4, None, bins, O) == INVALID
    assert bcall(batch._b, PT, PV, 4, E, bins, None) == INVALID
    assert bcall(batch._b, None, PV, n, E, bins, O) == INVALID
    assert bcall(batch._b, PT, PV, (1 << 31) // (2 * 80 * bins) + 1, E, bins, O) == INVALID  # 2 systems x m x bins x 80 bytes
    assert bcall(batch._b, PT, PV, 0, E, bins, O) == 0
    assert untouched()
    assert bcall(batch._b, None, None, n, E, bins, O) == 0
    smc.assert_same(out[0].view(smc.DTYPE).reshape(n, bins), want, "batch through the C call")
    assert (out[1] == 7.0).all()                                  # the empty system writes nothing in the own form
    batch.close()
