"""Pair-separation counts (nbody_get_pair_counts, nbody_batch_get_pair_counts; Stepper.pair_counts, StepperGroup.pair_counts,
StepperBatch.pair_counts) on the MI355X: the binned pair histogram of the resident state.

The definition has no fma and rounds every operation on its own, so the numpy model of pair_cases.py restates every d2 bit
for bit, and the results are integers: zero tolerance throughout - every count against the model, and product against
product (another rank, a batch against a Stepper holding the same state).  Every result is also checked for
below + sum(counts) + rest == pairs with the pairs the form implies."""
import numpy as np
import pytest

import lineage_cases as lc
import pair_cases as pc
import sharded_cases as sc

pytestmark = pytest.mark.gpu

INVALID, STATE_ERR = -1, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
DTYPE_OF = {0: np.float32, 1: np.float64}


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=capacity, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, precision):
    n = len(P)
    return nb.BodiesData.from_arrays(P, np.zeros((n, 2)), np.ones(n), np.full(n, 0.25), precision) if n else nb.BodiesData(0, precision)


def check(st, P, edges2, what, points=None):
    """pair_counts on the resident state, squared edges, against the model of P; -> the result."""
    got = st.pair_counts(edges2, points=points, squared=True)
    want = pc.model_pair_counts(P, edges2, points)
    n = len(P)
    print("%s: n %d, %d bins -> below %d, inside %d, rest %d of %d pairs" % (what, n, len(edges2) - 1, got["below"],
                                                                             int(got["counts"].sum()), got["rest"], got["pairs"]))
    pc.assert_same(got, want, what)
    pc.check_sum(got, n * (n - 1) // 2 if points is None else len(points) * n, what)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
# 63 .. 65: the cut at the wave's last row inside tile 0; 191 .. 193: the third wave, cut at 64 entries of tile 1; 385: a second
# workgroup whose first wave has self tile 2
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 385])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    field = 5.0 * np.sqrt(n)
    P, _ = pc.random_state(n, DTYPE_OF[precision], seed=n, field=field)
    # pi t^2 = 0.1 with t = r / field; with the borders of the square the expected share is pi t^2 - (8/3) t^3 + t^4 / 2 = 0.085
    tenth = 0.1 * field * field / np.pi
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, precision))
        got = check(st, P, np.linspace(0.0, tenth, 9), "n %d, a tenth of the pairs" % n)
        if n >= 127:
            assert 0.04 * got["pairs"] < int(got["counts"].sum()) < 0.12 * got["pairs"] and (got["counts"] > 0).all()
        got = check(st, P, np.array([0.0, np.inf]), "n %d, one bin for everything" % n)
        assert (got["counts"][0], got["below"], got["rest"]) == (n * (n - 1) // 2, 0, 0)
        got = check(st, P, np.array([4.0, 9.0]), "n %d, [4, 9]" % n)
        assert n < 127 or (got["below"] > 0 and got["counts"][0] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. equality at the edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_equality_at_the_edges(nb, precision):
    """lattice(8) has integer d2: 112 pairs at 1, 98 at 2, 96 at 4 and 168 at 5 (4 * 7 * 6; tests/test_pair_cases_cpu.py
    counts them with the model).  Moving the edges one ulp DOWN leaves every integer d2 in its bin (the first edge stays 0,
    a negative edge is refused); one ulp UP moves every count one bin down and brings d2 == 5 in from rest."""
    P, _ = pc.lattice(8)
    e2 = np.array([0.0, 1.0, 2.0, 4.0, 5.0])
    with small_stepper(nb, precision, 64) as st:
        st.upload(bodies_of(nb, P, precision))
        got = check(st, P, e2, "lattice")
        assert (got["counts"].tolist(), got["below"], got["rest"]) == ([0, 112, 98, 96], 0, 2016 - 306)
        down = np.concatenate([[0.0], np.nextafter(e2[1:], -np.inf)])
        got = check(st, P, down, "lattice, edges one ulp down")
        assert (got["counts"].tolist(), got["rest"]) == ([0, 112, 98, 96], 2016 - 306)
        up = np.concatenate([[0.0], np.nextafter(e2[1:], np.inf)])
        got = check(st, P, up, "lattice, edges one ulp up")
        assert (got["counts"].tolist(), got["rest"]) == ([112, 98, 96, 168], 2016 - 474)
        lengths = st.pair_counts([0.0, 1.0, 3.0])                 # lengths: squared once by the wrapper
        assert np.array_equal(lengths["edges2"], [0.0, 1.0, 9.0]) and lengths["counts"].tolist() == [0, 112 + 98 + 96 + 168 + 72]


# ---------------------------------------------------------------------------------------------------------------------
# 3. awkward values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_awkward_values(nb, precision):
    n = 130
    P, _ = pc.random_state(n, DTYPE_OF[precision], seed=2, field=30.0)
    wide = np.array([0.0, 25.0, 400.0, np.inf])
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, precision))
        assert check(st, P, wide, "finite state, top +inf")["rest"] == 0
        Pn = P.copy()
        Pn[7, 0] = np.nan                                         # its n - 1 pairs are in rest
        st.upload(bodies_of(nb, Pn, precision))
        assert check(st, Pn, wide, "NaN coordinate, top +inf")["rest"] == n - 1
        check(st, Pn, np.array([1.0, 100.0]), "NaN coordinate, finite top")
        if precision == 1:                                        # fp32 cannot hold it
            Pi = P.copy()
            Pi[129] = [1e200, 3.0]                                # d2 = +inf fails d2 < +inf
            st.upload(bodies_of(nb, Pi, precision))
            assert check(st, Pi, wide, "a body at 1e200, top +inf")["rest"] == n - 1
        C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])     # two bodies at one place: d2 = +0
        st.upload(bodies_of(nb, C, precision))
        got = check(st, C, np.array([0.0, 1.0]), "coincident, first edge 0")
        assert (got["counts"].tolist(), got["below"], got["rest"]) == ([1], 0, 2)
        got = check(st, C, np.array([1e-300, 1.0]), "coincident, first edge 1e-300")
        assert (got["counts"].tolist(), got["below"], got["rest"]) == ([0], 1, 2)
        st.upload(bodies_of(nb, P, precision))
        for bins in (1, 2, 3, 4, 255, 256):                      # every trip count of the edge search, both ends of its range
            check(st, P, np.geomspace(0.05, 2500.0, bins + 1), "%d geometric bins" % bins)
        got = check(st, P, np.geomspace(0.05, 2500.0, 257), "256 geometric bins")
        assert got["rest"] == 0 and np.count_nonzero(got["counts"]) > 100      # no d2 reaches 2 * 30^2; the bins are in use


# ---------------------------------------------------------------------------------------------------------------------
# 4. points form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_points_form(nb, precision):
    n, field = 300, 5.0 * np.sqrt(300)
    P, _ = pc.random_state(n, DTYPE_OF[precision], seed=300, field=field)
    e2 = np.linspace(0.0, 0.1 * field * field / np.pi, 9)
    allpts = np.random.default_rng(4).uniform(-5.0, field + 5.0, size=(300, 2))
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, precision))
        for m in (0, 1, 63, 65, 255, 256, 257, 300):               # 63, 65, 257: a wave past the last row only loads tiles
            got = check(st, P, e2, "m %d" % m, points=allpts[:m])
            assert m == 0 or got["counts"].sum() > 0
            check(st, P, np.array([0.0, np.inf]), "m %d, one bin" % m, points=allpts[:m])
        own = check(st, P, e2, "own form")
        on = check(st, P, e2, "the bodies' own positions as points", points=P)
        want = 2 * own["counts"].astype(np.int64)
        want[0] += n                                              # every body against itself at d2 = 0
        assert on["counts"].tolist() == want.tolist() and on["rest"] == 2 * own["rest"]
        st.upload(nb.BodiesData(0, precision))                    # no bodies left: nothing to count, in either form
        got = check(st, np.zeros((0, 2)), e2, "points over no bodies", points=allpts[:200])
        assert (got["counts"].sum(), got["below"], got["rest"], got["pairs"], got["n_bodies"]) == (0, 0, 0, 0, 0)
        check(st, np.zeros((0, 2)), e2, "no bodies")


# ---------------------------------------------------------------------------------------------------------------------
# 5. after stepping, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_after_stepping_and_no_effect_on_stepping(nb, precision):
    cfg = nb.stock_config(particleCount=2048)
    b = nb.init_bodies(cfg, precision)
    lengths = np.geomspace(1.0, cfg.fieldWidth / 8.0, 17)
    with nb.Stepper(cfg, precision=precision) as st, nb.Stepper(cfg, precision=precision) as plain:
        st.upload(b)
        plain.upload(b)
        st.step(5)
        P, _ = pc.widen(st.download())
        first = st.pair_counts(lengths)
        want = pc.model_pair_counts(P, first["edges2"])
        print("N 2048 after 5 steps: n %d, inside %d of %d pairs" % (len(P), int(first["counts"].sum()), first["pairs"]))
        pc.assert_same(first, want, "after 5 steps")
        pc.check_sum(first, len(P) * (len(P) - 1) // 2)
        assert np.array_equal(first["edges2"].view(np.uint64), (lengths * lengths).view(np.uint64)) and first["counts"].sum() > 0
        pc.assert_same(st.pair_counts(lengths), first, "called again")
        st.step(3)
        plain.step(8)
        a, c = st.download(), plain.download()
        assert a.numBodies == c.numBodies and a.block.view(np.uint8).tobytes() == c.block.view(np.uint8).tobytes()
        assert int(st.stats().pairs) == int(plain.stats().pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 6. batch
# ---------------------------------------------------------------------------------------------------------------------
def test_batch_equals_stepper_and_model(nb):
    cap, counts = 512, (512, 130, 0, 63, 64, 65, 193)
    S = len(counts)
    cfg = nb.stock_config(particleCount=cap, fieldWidth=3000, fieldHeight=3000)
    bodies = [nb.init_bodies(nb.stock_config(particleCount=k, fieldWidth=3000, fieldHeight=3000), seed=40 + s) if k else nb.BodiesData(0)
              for s, k in enumerate(counts)]
    e2 = np.geomspace(4.0, 600.0 ** 2, 13)
    pts = np.random.default_rng(6).uniform(0.0, 3000.0, size=(200, 2))
    with nb.StepperBatch(S, cap, cfg=cfg) as batch, nb.Stepper(cfg) as one:
        batch.upload(bodies)
        for steps in (0, 2):                                      # as uploaded: systems of exactly 63, 64, 65 and 193 bodies
            if steps:
                batch.step(steps)
            assert steps or [batch.download(s).numBodies for s in range(S)] == list(counts)
            for points in (None, pts):
                got = batch.pair_counts(e2, points=points, squared=True)
                assert len(got) == S
                for s in range(S):
                    d = batch.download(s)
                    P, _ = pc.widen(d)
                    n = d.numBodies
                    what = "system %d (n %d), %s form" % (s, n, "own" if points is None else "points")
                    pc.assert_same(got[s], pc.model_pair_counts(P[:n], e2, points), what + ": model")
                    pc.check_sum(got[s], n * (n - 1) // 2 if points is None else 200 * n, what)
                    one.upload(d)
                    pc.assert_same(got[s], one.pair_counts(e2, points=points, squared=True), what + ": Stepper")
                assert 0 < batch.download(1).numBodies <= 130 and got[0]["counts"].sum() > 0 and got[1]["counts"].sum() > 0
                empty = got[2]
                assert (empty["counts"].sum(), empty["below"], empty["rest"], empty["pairs"], empty["n_bodies"]) == (0, 0, 0, 0, 0)
        raw = np.full((S, 12), 77, dtype=np.uint64)               # the C call: every count and record is written
        infos = np.full(S, -7, dtype=pc.INFO_DTYPE)
        assert nb.lib.nbody_batch_get_pair_counts(batch._b, pts.ctypes.data, 200, e2.ctypes.data, 12, raw.ctypes.data, infos.ctypes.data) == 0
        assert np.array_equal(raw, np.stack([g["counts"] for g in got])) and infos["rows"].tolist() == [200] * S
        assert infos["n_bodies"].tolist() == [g["n_bodies"] for g in got] and infos["pairs"].tolist() == [g["pairs"] for g in got]


# ---------------------------------------------------------------------------------------------------------------------
# 7. not collective
# ---------------------------------------------------------------------------------------------------------------------
def test_every_rank_of_a_group(nb):
    n0, semantics = sc.RUNS[1]
    steps = 6                                                     # past the exchange lag
    assert steps > sc.LAG
    cfg, bodies = lc.dense_bodies(nb, n0)
    e2 = np.geomspace(1.0, float(lc.FIELD_OF[n0]) ** 2 / 16.0, 11)
    pts = np.random.default_rng(8).uniform(0.0, float(lc.FIELD_OF[n0]), size=(sc.POINTS, 2))
    grp = nb.StepperGroup(3, cfg=cfg, semantics=semantics)
    with nb.Stepper(cfg, semantics=semantics) as plain:
        grp.upload(bodies)
        plain.upload(bodies)
        grp.step(steps)
        plain.step(steps)
        d = grp.download()
        assert d.numBodies == sc.COUNTS[sc.RUNS[1]][steps - 1] == plain.download().numBodies
        P, _ = pc.widen(d)
        for points in (None, pts):
            want = plain.pair_counts(e2, points=points, squared=True)
            pc.assert_same(want, pc.model_pair_counts(P, e2, points), "the plain context")
            assert want["counts"].sum() > 0
            for rank in (2, 0, 1):                                # each on its own
                pc.assert_same(grp.pair_counts(e2, points=points, squared=True, rank=rank), want, "rank %d" % rank)
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors on a live context
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    P, _ = pc.random_state(300, np.float32, seed=11, field=100)
    call, bcall = nb.lib.nbody_get_pair_counts, nb.lib.nbody_batch_get_pair_counts
    counts = np.full(256, 77, dtype=np.uint64)
    info = np.full(1, -7, dtype=pc.INFO_DTYPE)
    untouched = (counts.tobytes(), info.tobytes())
    good = np.array([0.0, 4.0, 25.0])
    pts = np.zeros((4, 2))
    long = np.arange(258, dtype=np.float64)

    def bad_arguments(fn, handle):
        for e2, bins in ((good, 0), (long, 257), (good, -1)):
            assert fn(handle, None, 0, e2.ctypes.data, bins, counts.ctypes.data, info.ctypes.data) == INVALID
            assert b"bins" in nb.lib.nbody_last_error_string()
        for edges in ([0.0, 25.0, 4.0], [0.0, 4.0, 4.0], [-1.0, 4.0, 25.0], [0.0, np.nan, 25.0], [np.nan, 4.0, 25.0], [0.0, 4.0, np.nan],
                      [-0.0, 0.0, 1.0], [0.0, np.inf, np.inf]):
            e2 = np.array(edges)
            assert fn(handle, None, 0, e2.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == INVALID, edges
            assert b"edges2" in nb.lib.nbody_last_error_string()
        assert fn(handle, None, 0, None, 2, counts.ctypes.data, info.ctypes.data) == INVALID
        assert fn(handle, None, 0, good.ctypes.data, 2, None, info.ctypes.data) == INVALID
        assert fn(handle, None, 0, good.ctypes.data, 2, counts.ctypes.data, None) == INVALID
        assert fn(None, None, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == INVALID
        assert fn(handle, pts.ctypes.data, -1, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == INVALID
        assert fn(handle, pts.ctypes.data, (1 << 27) + 1, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == INVALID
        assert (counts.tobytes(), info.tobytes()) == untouched

    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, None, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == STATE_ERR      # before an upload
        assert b"before" in nb.lib.nbody_last_error_string()
        bad_arguments(call, st._ctx)                              # refused before the state is looked at
        st.upload(bodies_of(nb, P, 0))
        bad_arguments(call, st._ctx)
        st.step(1)                                                # a context that has never made the call works as ever
        P1, _ = pc.widen(st.download())
        assert call(st._ctx, None, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == 0
        want = pc.model_pair_counts(P1, good)
        n = len(P1)
        assert counts[:2].tolist() == want["counts"].tolist() and (counts[2:] == 77).all()
        assert tuple(info[0]) == (n, n, n * (n - 1) // 2, want["below"], want["rest"])
        assert call(st._ctx, pts.ctypes.data, 4, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == 0
        want = pc.model_pair_counts(P1, good, pts)
        assert counts[:2].tolist() == want["counts"].tolist() and tuple(info[0]) == (n, 4, 4 * n, want["below"], want["rest"])
        assert call(st._ctx, pts.ctypes.data, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == 0   # m == 0 is legal
        assert counts[:2].tolist() == [0, 0] and tuple(info[0]) == (n, 0, 0, 0, 0)
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 100, 100)] * 2) as batch:
        counts = np.full(256, 77, dtype=np.uint64)
        info = np.full(2, -7, dtype=pc.INFO_DTYPE)
        untouched = (counts.tobytes(), info.tobytes())
        assert bcall(batch._b, None, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == STATE_ERR
        batch.upload([bodies_of(nb, P, 0), nb.BodiesData(0)])
        bad_arguments(bcall, batch._b)
        assert bcall(batch._b, None, 0, good.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == 0
        want = pc.model_pair_counts(P, good)
        assert counts[:4].tolist() == want["counts"].tolist() + [0, 0] and (counts[4:] == 77).all()
        assert tuple(info[0]) == (300, 300, 44850, want["below"], want["rest"]) and tuple(info[1]) == (0, 0, 0, 0, 0)
