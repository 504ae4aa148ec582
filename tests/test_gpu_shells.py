"""Shell sums (nbody_get_shells, nbody_batch_get_shells; Stepper.shells, StepperGroup.shells, StepperBatch.shells) on the
MI355X: the mass and the number of the bodies in each bin of distance around every body or probe point.

The definition has no fma, rounds every operation on its own and fixes the order of the mass sum, so the numpy model of
shell_cases.py restates it bit for bit: zero tolerance throughout - count exactly, mass by its bits - against the model, and
product against product (nbody_get_pair_counts, nbody_get_knn, another rank, a batch against a Stepper holding the same
state) the same way.  The masses of order_sensitive_state span 1e4 .. 1e17: test_shell_cases_cpu.py asserts that their sums
change with the order, so a kernel that adds in another order, or re-associates, fails the comparisons of masses here."""
import ctypes

import numpy as np
import pytest

import sharded_cases as sc
import shell_cases as shc
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


def bodies_of(nb, P, M, precision):
    n = len(P)
    return nb.BodiesData.from_arrays(P, np.zeros((n, 2)), M, np.full(n, 0.25), precision) if n else nb.BodiesData(0, precision)


def check(st, P, M, edges2, what, points=None):
    """shells on the resident state, squared edges, against the model of (P, M); -> the result."""
    got = st.shells(edges2, points=points, squared=True)
    rows = len(P) if points is None else len(points)
    assert got["mass"].shape == (rows, len(edges2) - 1) == got["count"].shape, what
    shc.assert_same(got, shc.model_shells(P, M, edges2, points), what)
    return got


def check_download(st, edges2, what, points=None):
    P, M = shc.widen_mass(st.download())
    return check(st, P, M, edges2, what, points), P, M


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
# 63 .. 65: the self tile's checked loop ends inside tile 0; 191 .. 193: the third wave, self tile 1; 385: a second workgroup
# whose first wave has self tile 2
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 385])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    P, M = shc.order_sensitive_state(n, DTYPE_OF[precision])
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, M, precision))
        got = check(st, P, M, shc.tenth_edges(shc.tenth_field(n)), "n %d, a tenth of the field" % n)
        if n >= 127:
            inside = got["count"].sum(axis=1)
            assert (got["count"].sum(axis=0) > 0).any() and (inside < n - 1).any()     # a bin in use, a source outside
        got = check(st, P, M, WHOLE, "n %d, one bin for everything" % n)
        assert (got["count"] == n - 1).all()
        got = check(st, P, M, np.array([4.0, 9.0]), "n %d, [4, 9]" % n)
        assert n < 127 or got["count"].sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. every tier boundary
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_tier_boundary(nb, precision):
    n = 130
    P, M = shc.order_sensitive_state(n, DTYPE_OF[precision], field=30.0)
    pts = shc.probe_points(P, 37, seed=5, field=30.0)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, M, precision))
        seen = {}
        for bins in (1, 2, 4, 5, 8, 9, 16, 17, 31, 32):
            e2 = np.geomspace(0.05, 2500.0, bins + 1)
            own = check(st, P, M, e2, "%d geometric bins" % bins)
            exp = check(st, P, M, e2, "%d geometric bins, 37 points" % bins, points=pts)
            assert (own["count"].sum(axis=1) > 0).all() and np.count_nonzero(own["count"].sum(axis=0)) >= min(bins, 4)
            assert (exp["count"][-1] == 0).all() and (exp["mass"][-1] == 0).all()      # a point far outside the field
            seen[bins] = own
        # the tier plays no part and bins are independent: the last bin of each set against a call with that one bin alone
        for bins in (4, 5, 8, 9, 16, 17, 32):
            e2 = np.geomspace(0.05, 2500.0, bins + 1)
            k = bins - 1
            alone = st.shells(e2[k:k + 2], squared=True)
            assert np.array_equal(shc.bits(alone["mass"][:, 0]), shc.bits(seen[bins]["mass"][:, k]))
            assert np.array_equal(alone["count"][:, 0], seen[bins]["count"][:, k])


# ---------------------------------------------------------------------------------------------------------------------
# 3. equality at the edges and awkward values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_equality_at_the_edges(nb, precision):
    """lattice(8) has integer d2: 112 unordered pairs at 1, 98 at 2, 96 at 4 and 168 at 5 (test_shell_cases_cpu.py); the rows
    see each twice.  Edges one ulp DOWN leave every integer d2 in its bin; one ulp UP moves every count one bin down and
    brings d2 == 5 in."""
    P, _ = shc.lattice(8)
    M = np.ones(64)
    e2 = np.array([0.0, 1.0, 2.0, 4.0, 5.0])
    with small_stepper(nb, precision, 64) as st:
        st.upload(bodies_of(nb, P, M, precision))
        got = check(st, P, M, e2, "lattice")
        assert got["count"].sum(axis=0).tolist() == [0, 224, 196, 192] and got["count"][3 * 8 + 3].tolist() == [0, 4, 4, 4]
        down = np.concatenate([[0.0], np.nextafter(e2[1:], -INF)])
        assert check(st, P, M, down, "lattice, edges one ulp down")["count"].sum(axis=0).tolist() == [0, 224, 196, 192]
        up = np.concatenate([[0.0], np.nextafter(e2[1:], INF)])
        got = check(st, P, M, up, "lattice, edges one ulp up")
        assert got["count"].sum(axis=0).tolist() == [224, 196, 192, 336]
        assert np.array_equal(shc.bits(got["mass"]), shc.bits(got["count"].astype(np.float64)))     # unit masses
        lengths = st.shells([0.0, 1.0, 3.0])                      # lengths: squared once by the wrapper
        assert np.array_equal(lengths["edges2"], [0.0, 1.0, 9.0])
        assert lengths["count"].sum(axis=0).tolist() == [0, 2 * (112 + 98 + 96 + 168 + 72)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_awkward_values(nb, precision):
    n = 130
    P, M = shc.order_sensitive_state(n, DTYPE_OF[precision], seed=2, field=30.0)
    wide = np.array([0.0, 25.0, 400.0, INF])
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, M, precision))
        clean = check(st, P, M, wide, "finite state, top +inf")
        assert (clean["count"].sum(axis=1) == n - 1).all()
        Pn = P.copy()
        Pn[7, 0] = np.nan                                         # counted nowhere; its own row is empty
        st.upload(bodies_of(nb, Pn, M, precision))
        got = check(st, Pn, M, wide, "NaN coordinate, top +inf")
        assert (got["count"][7] == 0).all() and (np.delete(got["count"], 7, 0).sum(axis=1) == n - 2).all()
        check(st, Pn, M, np.array([1.0, 100.0]), "NaN coordinate, finite top")
        check(st, Pn, M, wide, "NaN coordinate, points", points=np.array([[np.nan, 1.0], [3.0, 4.0], [INF, 0.0]]))
        if precision == 1:                                        # fp32 cannot hold it
            Pi = P.copy()
            Pi[129] = [1e200, 3.0]                                # d2 = +inf fails d2 < +inf
            st.upload(bodies_of(nb, Pi, M, precision))
            got = check(st, Pi, M, wide, "a body at 1e200, top +inf")
            assert (got["count"][129] == 0).all() and (got["count"][:129].sum(axis=1) == n - 2).all()
        C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])     # two bodies at one place: d2 = +0
        Mc = np.array([5.0, 7.0, 11.0])
        st.upload(bodies_of(nb, C, Mc, precision))
        got = check(st, C, Mc, np.array([0.0, 1.0]), "coincident, first edge 0")
        assert got["count"].tolist() == [[1], [0], [1]] and got["mass"].tolist() == [[11.0], [0.0], [5.0]]
        got = check(st, C, Mc, np.array([1e-300, 1.0]), "coincident, first edge 1e-300")
        assert got["count"].tolist() == [[0], [0], [0]] and not got["mass"].any()
        Mz = M.copy()
        Mz[9] = 0.0                                               # a body of mass 0 counts and adds +0
        st.upload(bodies_of(nb, P, Mz, precision))
        got = check(st, P, Mz, wide, "a body of mass 0")
        assert np.array_equal(got["count"], clean["count"]) and not np.signbit(got["mass"]).any()
        Mn = M.copy()
        Mn[9] = np.nan                                            # a NaN mass: its bin is NaN, and it still counts
        st.upload(bodies_of(nb, P, Mn, precision))
        got = check(st, P, Mn, wide, "a NaN mass")
        assert np.array_equal(got["count"], clean["count"])
        assert (np.isnan(got["mass"]).sum(axis=1) == (np.arange(n) != 9)).all() and not np.isnan(got["mass"][9]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. points form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_points_form(nb, precision):
    n = 300
    field = shc.tenth_field(n)
    P, M = shc.order_sensitive_state(n, DTYPE_OF[precision])
    e2 = shc.tenth_edges(field)
    allpts = shc.probe_points(P, 257, seed=4, field=field)       # the first 64 ON bodies; points 1 and 255 the same point
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, M, precision))
        for m in (0, 1, 63, 64, 65, 257):                         # 63, 65, 257: a wave past the last row only loads tiles
            got = check(st, P, M, e2, "m %d" % m, points=allpts[:m])
            check(st, P, M, WHOLE, "m %d, one bin" % m, points=allpts[:m])
        on = np.arange(64) * 7 % n                                # got: m = 257.  A point on a body: d2 = +0 is counted
        first = st.shells([0.0, 1e-300], allpts[:64], squared=True)
        assert (first["count"] == 1).all() and np.array_equal(shc.bits(first["mass"][:, 0]), shc.bits(M[on]))
        assert shc.same(shc.sliced(got, slice(1, 2)), shc.sliced(got, slice(255, 256)))    # one point at two places
        one = st.shells(e2, allpts[200:201], squared=True)
        assert shc.same(one, shc.sliced(got, slice(200, 201)))   # alone or among 257: the same bits
        st.upload(nb.BodiesData(0, precision))                    # no bodies left: every bin {+0.0, 0}
        got = check(st, np.zeros((0, 2)), np.zeros(0), e2, "points over no bodies", points=allpts[:200])
        assert not got["count"].any() and not got["mass"].any() and not np.signbit(got["mass"]).any()
        assert check(st, np.zeros((0, 2)), np.zeros(0), e2, "no bodies")["mass"].shape == (0, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 5. products against each other
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_pair_counts_and_knn(nb, precision):
    n = 300
    field = shc.tenth_field(n)
    P, M = shc.order_sensitive_state(n, DTYPE_OF[precision])
    pts = shc.probe_points(P, 100, seed=9, field=field)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, M, precision))
        for e2 in (shc.tenth_edges(field), np.geomspace(0.5, 4 * field * field, 33), np.array([4.0, 9.0])):
            own, exp = st.shells(e2, squared=True), st.shells(e2, pts, squared=True)
            dd, dr = st.pair_counts(e2, squared=True), st.pair_counts(e2, points=pts, squared=True)
            assert own["count"].sum(axis=0, dtype=np.int64).tolist() == (2 * dd["counts"].astype(np.int64)).tolist()
            assert exp["count"].sum(axis=0, dtype=np.int64).tolist() == dr["counts"].astype(np.int64).tolist()
            assert dd["counts"].sum() > 0 and dr["counts"].sum() > 0
        near = st.knn(32)["d2"]
        near_pts = st.knn(32, pts)["d2"]
        for top in (1.0, 9.0, 40.0):                              # one bin [0, e2): the sources knn lists below e2
            for got, d2 in ((st.shells([0.0, top], squared=True), near), (st.shells([0.0, top], pts, squared=True), near_pts)):
                listed = (d2 < top).sum(axis=1)
                assert (listed < 32).any() and (listed > 0).any()
                assert np.array_equal(got["count"][:, 0][listed < 32], listed[listed < 32])


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics):
    """Literal semantics at n = 1000: the bodies from 896 on are frozen and stay sources like any other body - the model is
    taken over the whole download.  And a run with calls between the steps downloads the bytes of one without."""
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=7003)
    field = dense_field(n)
    e2 = np.geomspace(4.0, float(field) ** 2 / 4.0, 9)
    pts = shc.probe_points(shc.widen_mass(b)[0], 100, seed=4, field=field)

    def run(with_calls):
        counts = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            for s in range(4):
                if s:
                    st.step(1)
                if with_calls:
                    got, P, M = check_download(st, e2, "after %d steps" % s)
                    counts.append(len(P))
                    check(st, P, M, e2, "points after %d steps" % s, points=pts)
                    whole = st.shells(WHOLE, squared=True)
                    assert (whole["count"] == len(P) - 1).all()  # every other body of the download, the tail included
                    assert got["count"][0].sum() > 0
            d = st.download()
            end = (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                   np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes())
        return end, counts

    plain, _ = run(False)
    called, counts = run(True)
    assert plain == called                                        # state, count, pair counter, events
    assert counts[0] == n and counts[-1] == plain[0] < n and counts == sorted(counts, reverse=True)


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_of_a_group(nb, world):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    field = dense_field(n)
    e2 = np.geomspace(4.0, float(field) ** 2 / 4.0, 13)
    pts = shc.probe_points(shc.widen_mass(b)[0], 100, seed=8, field=field)
    grp = nb.StepperGroup(world, cfg=cfg)                         # NBODY_FLAG_GROUP_EXCHANGE, every rank on the one GPU
    grp.upload(b)
    steps = sc.LAG + 2                                            # past the exchange lag
    grp.step(steps)
    d = grp.download()
    P, M = shc.widen_mass(d)
    assert len(P) < n                                             # the count has shrunk
    with nb.Stepper(cfg) as one:                                  # a single-rank context on the group's download
        one.upload(d)
        want, want_pts = check(one, P, M, e2, "single rank"), check(one, P, M, e2, "single rank, points", points=pts)
    assert want["count"].sum() > 0
    for rank in reversed(range(world)):                           # each on its own
        shc.assert_same(grp.shells(e2, squared=True, rank=rank), want, "rank %d" % rank)
        shc.assert_same(grp.shells(e2, pts, squared=True, rank=rank), want_pts, "rank %d, points" % rank)
    grp.close()


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
    pts = shc.probe_points(shc.widen_mass(bodies[-1])[0], 100, seed=6, field=field)
    for steps, bins in ((0, 5), (3, 9), (0, 32)):
        batch.step(steps)
        e2 = np.geomspace(4.0, float(field) ** 2, bins + 1)
        own, exp, counts = batch.shells(e2, squared=True), batch.shells(e2, pts, squared=True), batch.counts()
        assert len(own) == S and exp["mass"].shape == (S, 100, bins) == exp["count"].shape
        if steps == 0 and bins == 5:
            assert counts.tolist() == BATCH_SIZES
        raw_mass = np.full((S, cap, bins), -3.0)                  # the C call into prefilled buffers: the tails stay
        raw_count = np.full((S, cap, bins), -77, dtype=np.int32)
        assert nb.lib.nbody_batch_get_shells(batch._b, None, cap, e2.ctypes.data, bins, raw_mass.ctypes.data,
                                             raw_count.ctypes.data) == 0
        for s in range(S):
            n = int(counts[s])
            what = "system %d (n %d), %d bins" % (s, n, bins)
            assert own[s]["mass"].shape == (n, bins), what
            assert shc.same({"mass": raw_mass[s, :n], "count": raw_count[s, :n]}, own[s]), what
            assert (raw_mass[s, n:] == -3.0).all() and (raw_count[s, n:] == -77).all(), what
            exp_s = {"mass": exp["mass"][s], "count": exp["count"][s]}
            if n == 0:                                            # the empty system: {+0.0, 0} everywhere
                assert not exp_s["count"].any() and not shc.bits(exp_s["mass"]).any()
                continue
            d = batch.download(s)
            P, M = shc.widen_mass(d)
            one.upload(d)
            shc.assert_same(own[s], one.shells(e2, squared=True), what + ": Stepper, own")
            shc.assert_same(exp_s, one.shells(e2, pts, squared=True), what + ": Stepper, points")
            shc.assert_same(own[s], shc.model_shells(P, M, e2), what + ": model, own")
            shc.assert_same(exp_s, shc.model_shells(P, M, e2, pts), what + ": model, points")
        assert own[-1]["count"].sum() > 0
        if steps:
            assert int(counts[4]) < cap                           # the dense system has merged bodies by now
    one.close()
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. raw C calls on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_raw_calls(nb):
    n, bins = 300, 4
    P, M = shc.order_sensitive_state(n, np.float32)
    e2 = np.array([0.0, 9.0, 25.0, 100.0, 400.0])
    b = bodies_of(nb, P, M, 0)
    mass = np.full((n, bins), 7.0)
    count = np.full((n, bins), 7, dtype=np.int32)
    pts = shc.probe_points(P, 4, seed=1, field=shc.tenth_field(n))
    nout = ctypes.c_int(-5)
    call = nb.lib.nbody_get_shells
    E, D, I, N, PT = e2.ctypes.data, mass.ctypes.data, count.ctypes.data, ctypes.byref(nout), pts.ctypes.data

    def untouched():
        return (mass == 7.0).all() and (count == 7).all()

    st = small_stepper(nb, 0, n)
    assert call(st._ctx, None, n, E, bins, D, I, N) == STATE_ERR  # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    bad = np.array([0.0, 9.0, 9.0, 100.0, 400.0])
    assert call(st._ctx, PT, 4, E, 0, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, np.arange(34.0).ctypes.data, 33, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, bad.ctypes.data, bins, D, I, N) == INVALID and b"edges2[2]" in nb.lib.nbody_last_error_string()
    assert call(st._ctx, PT, -1, E, bins, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, None, bins, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, E, bins, None, I, N) == INVALID
    assert call(st._ctx, PT, 4, E, bins, D, None, N) == INVALID
    assert call(st._ctx, PT, 4, E, bins, D, I, None) == INVALID
    assert call(st._ctx, PT, (1 << 31) // (12 * bins) + 1, E, bins, D, I, N) == INVALID    # m x bins x 12 bytes above 2^31
    assert call(st._ctx, None, (1 << 31) // (12 * bins) + 1, E, bins, D, I, N) == INVALID  # the own form: m as given
    assert call(st._ctx, None, n - 1, E, bins, D, I, N) == CAPACITY_ERR                    # room for fewer than the bodies
    assert untouched() and nout.value == -5
    assert call(st._ctx, PT, 0, E, bins, D, I, N) == 0 and nout.value == 0                 # m == 0 is legal
    assert untouched()
    assert call(st._ctx, None, n, E, bins, D, I, N) == 0 and nout.value == n
    want = shc.model_shells(P, M, e2)
    shc.assert_same({"mass": mass, "count": count}, want, "through the C call")
    lengths = st.shells([0.0, 3.0, 5.0, 10.0, 20.0])              # squared=False: the same edges as lengths
    shc.assert_same(lengths, want, "lengths")
    assert st.shells(e2, np.zeros((0, 2)), squared=True)["mass"].shape == (0, bins)
    with pytest.raises(nb.NbodyError):
        st.shells(np.arange(34.0), squared=True)
    st.close()
    batch = nb.StepperBatch(2, n, params=[(0.2, 0.1, 100, 100)] * 2)
    bcall = nb.lib.nbody_batch_get_shells
    mass = np.full((2, n, bins), 7.0)
    count = np.full((2, n, bins), 7, dtype=np.int32)
    D, I = mass.ctypes.data, count.ctypes.data
    assert bcall(batch._b, None, n, E, bins, D, I) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, PT, 4, E, 0, D, I) == INVALID
    assert bcall(batch._b, PT, 4, bad.ctypes.data, bins, D, I) == INVALID
    assert bcall(batch._b, PT, -1, E, bins, D, I) == INVALID
    assert bcall(batch._b, PT, 4, E, bins, None, I) == INVALID
    assert bcall(batch._b, PT, 4, E, bins, D, None) == INVALID
    assert bcall(batch._b, PT, (1 << 31) // (2 * 12 * bins) + 1, E, bins, D, I) == INVALID  # 2 systems x m x bins x 12 bytes
    assert bcall(batch._b, PT, 0, E, bins, D, I) == 0
    assert untouched()
    assert bcall(batch._b, None, n, E, bins, D, I) == 0
    shc.assert_same({"mass": mass[0], "count": count[0]}, want, "batch through the C call")
    assert (mass[1] == 7.0).all() and (count[1] == 7).all()      # the empty system writes nothing in the own form
    batch.close()
