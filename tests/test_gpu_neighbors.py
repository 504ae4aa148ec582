"""Neighbour queries (nbody_get_neighbors, nbody_batch_get_neighbors; Stepper.neighbors, StepperGroup.neighbors,
StepperBatch.neighbors) on the MI355X: the nearest body, its squared distance and the overlap count at the bodies' own
positions and at probe points.

The definition has no fma and rounds every operation on its own, so the numpy model of neighbor_cases.py restates it bit for
bit: zero tolerance throughout - d2 by bits, index and overlaps exactly - against the model, and product against product
(another rank, a batch against a Stepper holding the same state) the same way."""
import ctypes

import numpy as np
import pytest

import neighbor_cases as nc
from test_gpu_batch import FIELD_OF, params_of

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
INF = np.inf


def dense_field(n):
    """FIELD_OF's fields where it has one, its density (about 75 bodies per 1000 x 1000) elsewhere: stock radii overlap."""
    return FIELD_OF.get(n, max(200, int(115 * np.sqrt(n))))


def dense_bodies(nb, n, precision=0, seed=1024, zero_radii=False):
    kw = {"minRadius": 0.0, "maxRadius": 0.0} if zero_radii else {}
    cfg = nb.stock_config(particleCount=n, fieldWidth=dense_field(n), fieldHeight=dense_field(n), **kw)
    return cfg, nb.init_bodies(cfg, precision, seed=seed)


def check_own(st, what):
    """points=None on the resident state of `st` against the model of its download."""
    d = st.download()
    P, R = nc.widen(d)
    got = st.neighbors()
    assert got.dtype == nc.DTYPE and got.shape == (d.numBodies,), what
    want = nc.model_neighbors(P, R)
    print("%s: n %d, %d overlapping ordered pairs, closest pair d2 %.6g" % (what, d.numBodies, int(want["overlaps"].sum()),
                                                                            want["d2"].min() if len(want) else INF))
    nc.assert_same(got, want, what)
    return got, P, R


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 255, 256, 257, 300, 1000, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_and_workgroup_edges(nb, precision, n):
    for zero_radii in (False, True):
        cfg, b = dense_bodies(nb, n, precision, seed=n, zero_radii=zero_radii)
        with nb.Stepper(cfg, precision=precision) as st:
            st.upload(b)
            got, P, R = check_own(st, "n %d radii %s" % (n, "0" if zero_radii else "stock"))
        total = int(got["overlaps"].sum())
        assert total % 2 == 0                                     # symmetric
        if zero_radii:
            assert total == 0                                     # no two stock bodies coincide
        elif n >= 127:
            assert total > 0                                      # the dense field: the predicate holds somewhere
        if n == 1:
            assert tuple(got[0]) == nc.EMPTY
        else:
            nc.exact_check(P, R, got, sample=sorted({0, n // 2, n - 1}))


# ---------------------------------------------------------------------------------------------------------------------
# 2. explicit points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_points(nb, precision, n):
    cfg, b = dense_bodies(nb, n, precision, seed=n + 1)
    P, R = nc.widen(b)
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        for m in (0, 1, 256, 257, 1000):
            pts = nc.probe_points(P, m, seed=m, field=dense_field(n))
            got = st.neighbors(pts)
            assert got.shape == (m,) and got.dtype == nc.DTYPE
            nc.assert_same(got, nc.model_neighbors(P, R, points=pts), "n %d, %d points" % (n, m))
            if m >= 8:
                k = min(n, m // 4)                                # the first k points lie on bodies
                assert (got["d2"][:k] == 0).all() and (got["overlaps"][:k] >= 1).all()
                assert nc.same(got[1:2], got[m - 2:m - 1])        # the same point at two places of `points`
                assert got["overlaps"][-1] == 0 and got["index"][-1] >= 0 and got["d2"][-1] > dense_field(n) ** 2
                nc.exact_check(P, R, got, points=pts, sample=[0, k, m - 3, m - 1])
        one = st.neighbors(nc.probe_points(P, 1000, seed=1000, field=dense_field(n))[500:501])
        assert nc.same(one, got[500:501])                         # alone or among 1000: the same bits


# ---------------------------------------------------------------------------------------------------------------------
# 3. special states
# ---------------------------------------------------------------------------------------------------------------------
def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=capacity, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_ties_and_coincident_bodies(nb, precision):
    P, R = nc.lattice(8)
    with small_stepper(nb, precision, 64) as st:
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((64, 2)), np.ones(64), R, precision))
        got = st.neighbors()
        nc.assert_same(got, nc.model_neighbors(P, R), "lattice")
        assert np.array_equal(got["index"], nc.lattice_expected(8)) and (got["d2"] == 1.0).all()
        cell = st.neighbors([[2.5, 3.5], [100.0, 3.0]])
        assert cell["d2"][0] == 0.5 and cell["index"][0] == 26 and cell["index"][1] == 31
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((64, 2)), np.ones(64), np.full(64, 0.5), precision))
        touching = st.neighbors()                                 # d2 = 1 <= (1/2 + 1/2)^2: equality counts
        nc.assert_same(touching, nc.model_neighbors(P, np.full(64, 0.5)), "touching lattice")
        assert touching["overlaps"][9] == 4 and touching["overlaps"][0] == 2
        C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])
        st.upload(nb.BodiesData.from_arrays(C, np.zeros((3, 2)), np.ones(3), np.zeros(3), precision))
        got = st.neighbors()
        nc.assert_same(got, nc.model_neighbors(C, np.zeros(3)), "coincident")
        assert got["index"].tolist() == [2, 0, 0] and got["overlaps"].tolist() == [1, 0, 1]
        assert got["d2"][0] == 0 and not np.signbit(got["d2"][0])
        st.upload(nb.BodiesData.from_arrays([[10.0, 20.0]], [[0, 0]], [4.0], [1.0], precision))
        assert [tuple(r) for r in st.neighbors()] == [nc.EMPTY]   # one body: no eligible source
        seen = st.neighbors([[13.0, 24.0], [10.0, 20.0]])
        assert [tuple(r) for r in seen] == [(25.0, 0, 0), (0.0, 0, 1)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nan_coordinate_radius_and_mass(nb, precision):
    cfg, b = dense_bodies(nb, 200, precision, seed=3)
    b.Positions[150] = b.Positions[20]                            # two coincident bodies among others
    pts = nc.probe_points(nc.widen(b)[0], 70, seed=2, field=dense_field(200))
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        clean, _, _ = check_own(st, "coincident among others")
        assert clean["d2"][20] == 0 and clean["index"][20] == 150 and clean["index"][150] == 20
        bm = b.copy()
        bm.Masses[33] = np.nan                                    # the mass plays no part
        st.upload(bm)
        assert nc.same(st.neighbors(), clean) and nc.same(st.neighbors(pts), nc.model_neighbors(*nc.widen(b), points=pts))
        bx = b.copy()
        bx.Positions[133, 0] = np.nan                             # a NaN coordinate: never nearest, never an overlap
        st.upload(bx)
        got, P, R = check_own(st, "NaN coordinate")
        assert tuple(got[133]) == nc.EMPTY and (got["index"] != 133).all()
        nc.assert_same(st.neighbors(pts), nc.model_neighbors(P, R, points=pts), "NaN coordinate, points")
        br = b.copy()
        br.Radii[64] = np.nan                                     # a NaN radius: overlaps nothing, distances untouched
        st.upload(br)
        got, P, R = check_own(st, "NaN radius")
        assert got["overlaps"][64] == 0 and np.array_equal(got["d2"], clean["d2"]) and np.array_equal(got["index"], clean["index"])
        nanpts = np.array([[np.nan, 1.0], [np.inf, 0.0], [1.0, -np.inf]])
        assert [tuple(r) for r in st.neighbors(nanpts)] == [nc.EMPTY] * 3


def test_fp64_coordinate_of_1e200(nb):
    P, R = nc.random_state(140, np.float64, seed=2, field=30.0, radius=2.0)
    P[7, 1] = 1e200                                               # squares to +inf
    P[139, 0] = -1e200
    with small_stepper(nb, nb.F64, 140) as st:
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((140, 2)), np.ones(140), R, nb.F64))
        got = st.neighbors()
        nc.assert_same(got, nc.model_neighbors(P, R), "1e200")
        assert tuple(got[7]) == nc.EMPTY and tuple(got[139]) == nc.EMPTY
        assert not np.isin(got["index"], [7, 139]).any()
        pts = np.array([[1e200, 0.0], [3.0, 1e200], [3.0, 4.0], [1e160, 1.0]])
        exp = st.neighbors(pts)
        nc.assert_same(exp, nc.model_neighbors(P, R, points=pts), "1e200, points")
        assert tuple(exp[0]) == nc.EMPTY and exp["index"][1] == 7 and exp["d2"][1] < INF   # dy = 0 towards body 7
        R[3] = 1e200                                              # s*s = +inf: the one case a +inf d2 counts
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((140, 2)), np.ones(140), R, nb.F64))
        got = st.neighbors()
        nc.assert_same(got, nc.model_neighbors(P, R), "1e200 radius")
        assert got["overlaps"][3] == 139 and got["overlaps"][7] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. after steps: the current count, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1500])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics, n):
    cfg, b = dense_bodies(nb, n, seed=7003)
    pts = nc.probe_points(nc.widen(b)[0], 100, seed=4, field=dense_field(n))

    def run(with_calls):
        counts = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            for k in range(4):
                if k:
                    st.step(1)
                if with_calls:
                    got, P, R = check_own(st, "n0 %d after %d steps" % (n, k))
                    counts.append(len(got))
                    nc.assert_same(st.neighbors(pts), nc.model_neighbors(P, R, points=pts), "points after %d steps" % k)
            d = st.download()
            end = (d.numBodies, d.block.view(np.uint32).tobytes(), int(st.stats().pairs), int(st.stats().steps),
                   np.sort(st.events(), order=["step", "i", "j", "kind"]).tobytes())
        return end, counts

    plain, _ = run(False)
    called, counts = run(True)
    assert plain == called                                        # state, count, pair counter, events
    assert counts[0] == n and counts[-1] == plain[0] < n and counts == sorted(counts, reverse=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a ring-kernel context
# ---------------------------------------------------------------------------------------------------------------------
def test_ring_kernel_context(nb):
    n = 8269                                                      # ragged: 64 tiles and 77 bodies
    cfg = nb.stock_config(particleCount=n, fieldWidth=12000, fieldHeight=12000)
    with nb.Stepper(cfg) as st:
        assert "ring" in st.force_kernel_name()
        st.upload(nb.init_bodies(cfg))
        st.step(2)
        got, P, R = check_own(st, "ring kernel context")
        assert len(got) <= n
        nc.exact_check(P, R, got, sample=[0, len(got) - 1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. not collective
# ---------------------------------------------------------------------------------------------------------------------
def test_not_collective(nb):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    pts = nc.probe_points(nc.widen(b)[0], 300, seed=8, field=dense_field(n))
    grp = nb.StepperGroup(3, cfg=cfg)
    grp.upload(b)
    grp.step(2)
    P, R = nc.widen(grp.download())
    assert len(R) < n
    want, want_pts = nc.model_neighbors(P, R), nc.model_neighbors(P, R, points=pts)
    for rank in (2, 0, 1):                                        # each on its own, in no particular order
        nc.assert_same(grp.neighbors(rank=rank), want, "rank %d" % rank)
        nc.assert_same(grp.neighbors(pts, rank=rank), want_pts, "rank %d, points" % rank)
    grp.close()
    with nb.Stepper(cfg, comm_id=nb.comm_unique_id(), force_comm=True) as rc:
        rc.upload(b)
        rc.step(2)
        nc.assert_same(rc.neighbors(), want, "FORCE_COMM context")
        nc.assert_same(rc.neighbors(pts), want_pts, "FORCE_COMM context, points")


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    cfg, b = dense_bodies(nb, 300)
    st = nb.Stepper(cfg)
    out = np.zeros(300, dtype=nc.DTYPE)
    out["d2"], out["index"], out["overlaps"] = 7.0, 7, 7
    pts = nc.probe_points(nc.widen(b)[0], 4, seed=1, field=dense_field(300))
    n = ctypes.c_int(-5)
    call = nb.lib.nbody_get_neighbors
    untouched = out.tobytes()
    assert call(st._ctx, None, 300, out.ctypes.data, ctypes.byref(n)) == STATE_ERR       # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    assert call(st._ctx, pts.ctypes.data, -1, out.ctypes.data, ctypes.byref(n)) == INVALID
    assert call(st._ctx, pts.ctypes.data, 4, None, ctypes.byref(n)) == INVALID
    assert call(st._ctx, pts.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert call(st._ctx, pts.ctypes.data, (1 << 31) // 16 + 1, out.ctypes.data, ctypes.byref(n)) == INVALID
    assert call(st._ctx, None, 299, out.ctypes.data, ctypes.byref(n)) == CAPACITY_ERR    # room for fewer than the 300 bodies
    assert out.tobytes() == untouched and n.value == -5
    assert call(st._ctx, pts.ctypes.data, 0, out.ctypes.data, ctypes.byref(n)) == 0 and n.value == 0
    assert out.tobytes() == untouched
    assert call(st._ctx, None, 300, out.ctypes.data, ctypes.byref(n)) == 0 and n.value == 300
    want = nc.model_neighbors(*nc.widen(b))
    nc.assert_same(out, want, "through the C call")
    assert st.neighbors(np.zeros((0, 2))).shape == (0,)
    st.close()
    batch = nb.StepperBatch(2, 300, cfg=cfg)
    bcall = nb.lib.nbody_batch_get_neighbors
    bout = np.zeros(600, dtype=nc.DTYPE)
    bout["d2"], bout["index"], bout["overlaps"] = 7.0, 7, 7
    untouched = bout.tobytes()
    assert bcall(batch._b, None, 300, bout.ctypes.data) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, pts.ctypes.data, -1, bout.ctypes.data) == INVALID
    assert bcall(batch._b, pts.ctypes.data, 4, None) == INVALID
    assert bcall(batch._b, pts.ctypes.data, (1 << 31) // 32 + 1, bout.ctypes.data) == INVALID   # 2 systems x m x 16 bytes
    assert bcall(batch._b, pts.ctypes.data, 0, bout.ctypes.data) == 0
    assert bout.tobytes() == untouched
    assert bcall(batch._b, None, 300, bout.ctypes.data) == 0
    nc.assert_same(bout[:300], want, "batch through the C call")
    assert bout[300:].tobytes() == untouched[300 * 16:]           # the empty system writes nothing in the own form
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1500, 2048, 4096, 0]


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_and_model(nb, semantics):
    cap = 4096
    cfgs, bodies = [], []
    for s, n in enumerate(BATCH_SIZES):
        cfg, bd = dense_bodies(nb, max(n, 1), seed=40 + s)
        cfgs.append(cfg)
        bodies.append(bd if n else nb.BodiesData(0))
    S = len(BATCH_SIZES)
    assert S == 17
    batch = nb.StepperBatch(S, cap, params=[params_of(c) for c in cfgs], semantics=semantics)
    batch.upload(bodies)
    one = nb.Stepper(cfgs[-2], capacity=cap, semantics=semantics)
    pts = nc.probe_points(nc.widen(bodies[-2])[0], 300, seed=6, field=dense_field(4096))
    for steps in (0, 2):
        batch.step(steps)
        own, exp, counts = batch.neighbors(), batch.neighbors(pts), batch.counts()
        assert len(own) == S and exp.shape == (S, 300) and exp.dtype == nc.DTYPE
        if steps == 0:
            assert counts.tolist() == BATCH_SIZES
        raw = np.zeros((S, cap), dtype=nc.DTYPE)                  # the C call into a prefilled buffer: the tails stay
        raw["d2"], raw["index"], raw["overlaps"] = -3.0, -77, -78
        pattern = raw[0, 0].tobytes()
        assert nb.lib.nbody_batch_get_neighbors(batch._b, None, cap, raw.ctypes.data) == 0
        for s in range(S):
            n = int(counts[s])
            what = "system %d (n %d) after %d steps" % (s, n, steps)
            assert own[s].shape == (n,), what
            assert nc.same(raw[s, :n], own[s]), what
            assert raw[s, n:].tobytes() == pattern * (cap - n), what
            if n == 0:                                            # the empty system
                assert [tuple(r) for r in exp[s]] == [nc.EMPTY] * 300
                continue
            d = batch.download(s)
            P, R = nc.widen(d)
            one.upload(d)
            nc.assert_same(own[s], one.neighbors(), what + ": Stepper, own")
            nc.assert_same(exp[s], one.neighbors(pts), what + ": Stepper, points")
            nc.assert_same(own[s], nc.model_neighbors(P, R), what + ": model, own")
            nc.assert_same(exp[s], nc.model_neighbors(P, R, points=pts), what + ": model, points")
        if steps:
            assert int(counts[12]) < 1000 and int(counts[15]) < 4096   # the dense systems have merged bodies by now
    one.close()
    batch.close()


def test_batch_of_1024_systems_of_64(nb):
    S, n = 1024, 64
    cfg = nb.stock_config(particleCount=n, fieldWidth=500, fieldHeight=500)
    bodies = [nb.init_bodies(cfg, seed=900 + s) for s in range(S)]
    batch = nb.StepperBatch(S, n, cfg=cfg)
    batch.upload(bodies)
    batch.step(2)
    pts = nc.probe_points(nc.widen(bodies[0])[0], 16, seed=12, field=500)
    exp, own, counts = batch.neighbors(pts), batch.neighbors(), batch.counts()
    assert exp.shape == (S, 16) and len(own) == S and 0 < counts.min() and counts.max() <= n
    one = nb.Stepper(cfg, capacity=n)
    for s in range(S):
        d = batch.download(s)
        P, R = nc.widen(d)
        assert own[s].shape == (int(counts[s]),)
        nc.assert_same(own[s], nc.model_neighbors(P, R), "system %d, own" % s)
        nc.assert_same(exp[s], nc.model_neighbors(P, R, points=pts), "system %d, points" % s)
        if s in (0, 1, 63, 64, 511, 1023):
            one.upload(d)
            nc.assert_same(own[s], one.neighbors(), "system %d: Stepper, own" % s)
            nc.assert_same(exp[s], one.neighbors(pts), "system %d: Stepper, points" % s)
    one.close()
    batch.close()
