"""k-nearest-neighbour queries (nbody_get_knn, nbody_batch_get_knn; Stepper.knn, StepperGroup.knn, StepperBatch.knn) on the
MI355X: the k nearest bodies and their squared distances at the bodies' own positions and at probe points.

The definition has no fma and rounds every operation on its own, so the numpy model of knn_cases.py restates it bit for bit:
zero tolerance throughout - d2 by bits, index exactly - against the model, and product against product (nbody_get_neighbors,
another rank, a batch against a Stepper holding the same state) the same way."""
import ctypes

import numpy as np
import pytest

import knn_cases as kc
import neighbor_cases as nc
import sharded_cases as sc
from test_gpu_batch import params_of
from test_gpu_neighbors import dense_bodies, dense_field, small_stepper

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
KS = (1, 2, 5, 8, 9, 32)                                          # every tier, off a tier boundary, one past a boundary
INF = np.inf


def check_nearest(st, got, points=None):
    """knn's entry 0 against nbody_get_neighbors on the same state: the same bits."""
    near = st.neighbors(points)
    assert np.array_equal(kc.bits(got["d2"][:, 0]), kc.bits(near["d2"])) and np.array_equal(got["index"][:, 0], near["index"])


def check_own(st, ks, what):
    """points=None on the resident state of `st`, every k of `ks`, against the model of its download; k = 1 against
    neighbors()."""
    d = st.download()
    P, _ = nc.widen(d)
    out = {}
    for k in ks:
        got = st.knn(k)
        assert got["d2"].shape == (d.numBodies, k), (what, k)
        kc.assert_same(got, kc.model_knn(P, k), "%s, k %d" % (what, k))
        out[k] = got
    check_nearest(st, st.knn(1))
    return out, P


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile, wave and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1000, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_wave_and_workgroup_edges(nb, precision, n):
    cfg, b = dense_bodies(nb, n, precision, seed=n)
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        got, _ = check_own(st, KS, "n %d" % n)
    for k in KS:
        kc.check_invariants(got[k], rows=np.arange(n))
        live = min(k, n - 1)                                      # k > n - 1: the rest is padding
        assert (got[k]["index"][:, :live] >= 0).all() and (got[k]["index"][:, live:] == -1).all()
        assert kc.same(kc.sliced(got[32], (slice(None), slice(0, k))), got[k])   # the prefix property


# ---------------------------------------------------------------------------------------------------------------------
# 2. explicit points
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_explicit_points(nb, precision, n):
    cfg, b = dense_bodies(nb, n, precision, seed=n + 1)
    P, _ = nc.widen(b)
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        for m in (0, 1, 257, 700):
            pts = kc.probe_points(P, m, seed=m, field=dense_field(n))
            for k in KS:
                got = st.knn(k, pts)
                assert got["d2"].shape == (m, k) and got["index"].shape == (m, k)
                kc.assert_same(got, kc.model_knn(P, k, points=pts), "n %d, %d points, k %d" % (n, m, k))
                kc.check_invariants(got)
                if k == 1:
                    check_nearest(st, got, pts)
            if m >= 8:                                            # got: k = 32
                on = min(n, m // 4)                               # the first points lie on bodies: listed at +0
                assert (got["d2"][:on, 0] == 0).all() and np.array_equal(got["index"][:on, 0], (np.arange(on) * 7) % n)
                assert kc.same(kc.sliced(got, slice(1, 2)), kc.sliced(got, slice(m - 2, m - 1)))   # one point, two places
                assert got["d2"][-1, 0] > dense_field(n) ** 2 and (got["index"][-1] >= 0).all()    # far outside
        one = st.knn(32, kc.probe_points(P, 700, seed=700, field=dense_field(n))[500:501])
        assert kc.same(one, kc.sliced(got, slice(500, 501)))     # alone or among 700: the same bits


# ---------------------------------------------------------------------------------------------------------------------
# 3. special states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_ties_and_coincident_bodies(nb, precision):
    P, R = kc.lattice(8)
    Q = np.concatenate([P, P[[20, 20]]])                          # bodies 64 and 65 on body 20
    with small_stepper(nb, precision, 66) as st:
        st.upload(nb.BodiesData.from_arrays(Q, np.zeros((66, 2)), np.ones(66), np.full(66, 0.25), precision))
        for k in (4, 5, 8, 12):
            got = st.knn(k)
            kc.assert_same(got, kc.model_knn(Q, k), "lattice, k %d" % k)
            kc.check_invariants(got, rows=np.arange(66))
        got = st.knn(8)
        i = 3 * 8 + 3                                             # interior, away from the twins
        assert got["d2"][i].tolist() == [1.0] * 4 + [2.0] * 4
        assert got["index"][i].tolist() == [i - 8, i - 1, i + 1, i + 8, i - 9, i - 7, i + 7, i + 9]   # every tie: lowest j
        assert got["index"][20, :2].tolist() == [64, 65] and got["d2"][20, :2].tolist() == [0.0, 0.0]
        assert got["index"][64, :2].tolist() == [20, 65] and got["index"][65, :2].tolist() == [20, 64]
        assert not np.signbit(got["d2"][[20, 64, 65], :2]).any()
        assert got["index"][12, :6].tolist() == [4, 11, 13, 20, 64, 65]
        cell = st.knn(5, [[2.5, 3.5], [4.0, 2.0]])
        kc.assert_same(cell, kc.model_knn(Q, 5, points=[[2.5, 3.5], [4.0, 2.0]]), "lattice, points")
        assert cell["index"][0, :4].tolist() == [26, 27, 34, 35] and cell["index"][1, :3].tolist() == [20, 64, 65]
        check_nearest(st, st.knn(1))
        st.upload(nb.BodiesData.from_arrays([[10.0, 20.0]], [[0, 0]], [4.0], [1.0], precision))
        lone = st.knn(3)                                          # one body: no eligible source
        assert (lone["index"] == -1).all() and (lone["d2"] == INF).all() and lone["d2"].shape == (1, 3)
        seen = st.knn(2, [[13.0, 24.0]])
        assert seen["d2"].tolist() == [[25.0, INF]] and seen["index"].tolist() == [[0, -1]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_nan_coordinate_radius_and_mass(nb, precision):
    cfg, b = dense_bodies(nb, 200, precision, seed=3)
    b.Positions[150] = b.Positions[20]
    pts = kc.probe_points(nc.widen(b)[0], 70, seed=2, field=dense_field(200))
    with nb.Stepper(cfg, precision=precision) as st:
        st.upload(b)
        clean, P = check_own(st, (5, 32), "coincident among others")
        clean_pts = st.knn(5, pts)
        kc.assert_same(clean_pts, kc.model_knn(P, 5, points=pts), "points")
        assert clean[5]["d2"][20, 0] == 0 and clean[5]["index"][20, 0] == 150 and clean[5]["index"][150, 0] == 20
        bm = b.copy()
        bm.Masses[33] = np.nan                                    # masses and radii play no part
        bm.Radii[64] = np.nan
        st.upload(bm)
        assert kc.same(st.knn(5), clean[5]) and kc.same(st.knn(32), clean[32]) and kc.same(st.knn(5, pts), clean_pts)
        bx = b.copy()
        bx.Positions[133, 0] = np.nan                             # a NaN coordinate: listed nowhere, its row all empty
        st.upload(bx)
        got, P = check_own(st, (5, 32), "NaN coordinate")
        for k in (5, 32):
            assert (got[k]["index"][133] == -1).all() and (got[k]["d2"][133] == INF).all()
            assert (got[k]["index"] != 133).all()
        kc.assert_same(st.knn(9, pts), kc.model_knn(P, 9, points=pts), "NaN coordinate, points")
        nanpts = st.knn(4, np.array([[np.nan, 1.0], [np.inf, 0.0], [1.0, -np.inf]]))
        assert (nanpts["index"] == -1).all() and (nanpts["d2"] == INF).all()


def test_fp64_coordinate_of_1e200(nb):
    P, R = kc.random_state(140, np.float64, seed=2, field=30.0, radius=2.0)
    P[7, 1] = 1e200                                               # squares to +inf: not eligible
    P[139, 0] = -1e200
    with small_stepper(nb, nb.F64, 140) as st:
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((140, 2)), np.ones(140), R, nb.F64))
        got, _ = check_own(st, (3, 32), "1e200")
        for i in (7, 139):
            assert (got[32]["index"][i] == -1).all() and (got[32]["d2"][i] == INF).all()
        assert not np.isin(got[32]["index"], [7, 139]).any()
        pts = np.array([[1e200, 0.0], [3.0, 1e200], [3.0, 4.0], [1e160, 1.0]])
        exp = st.knn(3, pts)
        kc.assert_same(exp, kc.model_knn(P, 3, points=pts), "1e200, points")
        assert (exp["index"][0] == -1).all() and exp["index"][1].tolist() == [7, -1, -1] and exp["d2"][1, 0] < INF


# ---------------------------------------------------------------------------------------------------------------------
# 4. after steps: the current count, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1500])
@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_after_steps_and_no_effect_on_stepping(nb, semantics, n):
    cfg, b = dense_bodies(nb, n, seed=7003)
    pts = kc.probe_points(nc.widen(b)[0], 100, seed=4, field=dense_field(n))

    def run(with_calls):
        counts = []
        with nb.Stepper(cfg, semantics=semantics, record_events=True) as st:
            st.upload(b)
            for s in range(4):
                if s:
                    st.step(1)
                if with_calls:
                    got, P = check_own(st, (1, 9), "n0 %d after %d steps" % (n, s))
                    counts.append(len(got[9]["d2"]))
                    kc.assert_same(st.knn(5, pts), kc.model_knn(P, 5, points=pts), "points after %d steps" % s)
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
        P, _ = nc.widen(st.download())
        got = st.knn(16)
        assert got["d2"].shape == (len(P), 16) and len(P) <= n
        # the model's sort of all n x n distances takes longer than a test should: the first and the last rows, the rows
        # around every tenth wave edge and a random tenth of the rest against the model, every row's entry 0 against neighbors()
        rng = np.random.default_rng(5)
        edges = np.concatenate([np.arange(w - 2, w + 2) for w in range(640, len(P) - 2, 640)])
        rows = np.unique(np.concatenate([np.arange(130), np.arange(len(P) - 130, len(P)), edges, rng.choice(len(P), 800, replace=False)]))
        kc.assert_same(kc.sliced(got, rows), kc.model_knn(P, 16, rows=rows), "ring kernel context")
        kc.check_invariants(got, rows=np.arange(len(P)))
        check_nearest(st, got)


# ---------------------------------------------------------------------------------------------------------------------
# 6. not collective
# ---------------------------------------------------------------------------------------------------------------------
def test_not_collective(nb):
    n = 1000
    cfg, b = dense_bodies(nb, n, seed=n)
    pts = kc.probe_points(nc.widen(b)[0], 300, seed=8, field=dense_field(n))
    grp = nb.StepperGroup(2, cfg=cfg)                             # NBODY_FLAG_GROUP_EXCHANGE, both ranks on the one GPU
    grp.upload(b)
    steps = sc.LAG + 2                                            # past the exchange lag (nbody_ctx::kLag)
    assert steps > sc.LAG
    grp.step(steps)
    d = grp.download()
    P, _ = nc.widen(d)
    assert len(P) < n
    with nb.Stepper(cfg) as one:                                  # a single-rank context on the group's download
        one.upload(d)
        want, want_pts = one.knn(9), one.knn(9, pts)
    kc.assert_same(want, kc.model_knn(P, 9), "single rank")
    kc.assert_same(want_pts, kc.model_knn(P, 9, points=pts), "single rank, points")
    for rank in (1, 0):                                           # each on its own
        kc.assert_same(grp.knn(9, rank=rank), want, "rank %d" % rank)
        kc.assert_same(grp.knn(9, pts, rank=rank), want_pts, "rank %d, points" % rank)
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors on a live context and a live batch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    cfg, b = dense_bodies(nb, 300)
    st = nb.Stepper(cfg)
    k = 4
    d2 = np.full((300, k), 7.0)
    index = np.full((300, k), 7, dtype=np.int32)
    pts = kc.probe_points(nc.widen(b)[0], 4, seed=1, field=dense_field(300))
    n = ctypes.c_int(-5)
    call = nb.lib.nbody_get_knn
    D, I, N, PT = d2.ctypes.data, index.ctypes.data, ctypes.byref(n), pts.ctypes.data

    def untouched():
        return (d2 == 7.0).all() and (index == 7).all()

    assert call(st._ctx, None, 300, k, D, I, N) == STATE_ERR     # before an upload
    assert b"before" in nb.lib.nbody_last_error_string()
    st.upload(b)
    assert call(st._ctx, PT, 4, 0, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, 33, D, I, N) == INVALID
    assert call(st._ctx, PT, -1, k, D, I, N) == INVALID
    assert call(st._ctx, PT, 4, k, None, I, N) == INVALID
    assert call(st._ctx, PT, 4, k, D, None, N) == INVALID
    assert call(st._ctx, PT, 4, k, D, I, None) == INVALID
    assert call(st._ctx, PT, (1 << 31) // (12 * k) + 1, k, D, I, N) == INVALID            # m x k x 12 bytes above 2^31
    assert call(st._ctx, None, (1 << 31) // (12 * k) + 1, k, D, I, N) == INVALID          # the own form: m as given
    assert call(st._ctx, None, 299, k, D, I, N) == CAPACITY_ERR  # room for fewer than the 300 bodies
    assert untouched() and n.value == -5
    assert call(st._ctx, PT, 0, k, D, I, N) == 0 and n.value == 0
    assert untouched()
    assert call(st._ctx, None, 300, k, D, I, N) == 0 and n.value == 300
    want = kc.model_knn(nc.widen(b)[0], k)
    kc.assert_same({"d2": d2, "index": index}, want, "through the C call")
    assert st.knn(3, np.zeros((0, 2)))["d2"].shape == (0, 3)
    with pytest.raises(nb.NbodyError):
        st.knn(33)
    st.close()
    batch = nb.StepperBatch(2, 300, cfg=cfg)
    bcall = nb.lib.nbody_batch_get_knn
    d2 = np.full((2, 300, k), 7.0)
    index = np.full((2, 300, k), 7, dtype=np.int32)
    D, I = d2.ctypes.data, index.ctypes.data
    assert bcall(batch._b, None, 300, k, D, I) == STATE_ERR
    batch.upload([b, nb.BodiesData(0)])
    assert bcall(batch._b, PT, 4, 0, D, I) == INVALID
    assert bcall(batch._b, PT, 4, 33, D, I) == INVALID
    assert bcall(batch._b, PT, -1, k, D, I) == INVALID
    assert bcall(batch._b, PT, 4, k, None, I) == INVALID
    assert bcall(batch._b, PT, 4, k, D, None) == INVALID
    assert bcall(batch._b, PT, (1 << 31) // (2 * 12 * k) + 1, k, D, I) == INVALID         # 2 systems x m x k x 12 bytes
    assert bcall(batch._b, PT, 0, k, D, I) == 0
    assert untouched()
    assert bcall(batch._b, None, 300, k, D, I) == 0
    kc.assert_same({"d2": d2[0], "index": index[0]}, want, "batch through the C call")
    assert (d2[1] == 7.0).all() and (index[1] == 7).all()        # the empty system writes nothing in the own form
    batch.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. batch
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
    pts = kc.probe_points(nc.widen(bodies[-1])[0], 300, seed=6, field=dense_field(1024))
    for steps, k in ((0, 5), (3, 9), (0, 32)):
        batch.step(steps)
        own, exp, counts = batch.knn(k), batch.knn(k, pts), batch.counts()
        assert len(own) == S and exp["d2"].shape == (S, 300, k) and exp["index"].shape == (S, 300, k)
        if steps == 0 and k == 5:
            assert counts.tolist() == BATCH_SIZES
        raw_d2 = np.full((S, cap, k), -3.0)                       # the C call into prefilled buffers: the tails stay
        raw_index = np.full((S, cap, k), -77, dtype=np.int32)
        assert nb.lib.nbody_batch_get_knn(batch._b, None, cap, k, raw_d2.ctypes.data, raw_index.ctypes.data) == 0
        for s in range(S):
            n = int(counts[s])
            what = "system %d (n %d), k %d" % (s, n, k)
            assert own[s]["d2"].shape == (n, k), what
            assert kc.same({"d2": raw_d2[s, :n], "index": raw_index[s, :n]}, own[s]), what
            assert (raw_d2[s, n:] == -3.0).all() and (raw_index[s, n:] == -77).all(), what
            exp_s = kc.sliced(exp, s)
            if n == 0:                                            # the empty system
                assert (exp_s["index"] == -1).all() and (exp_s["d2"] == INF).all()
                continue
            d = batch.download(s)
            P, _ = nc.widen(d)
            one.upload(d)
            kc.assert_same(own[s], one.knn(k), what + ": Stepper, own")
            kc.assert_same(exp_s, one.knn(k, pts), what + ": Stepper, points")
            kc.assert_same(own[s], kc.model_knn(P, k), what + ": model, own")
            kc.assert_same(exp_s, kc.model_knn(P, k, points=pts), what + ": model, points")
        if steps:
            assert int(counts[4]) < 1024                          # the dense system has merged bodies by now
    one.close()
    batch.close()


def test_batch_of_1024_systems_of_64(nb):
    S, n, k = 1024, 64, 8
    cfg = nb.stock_config(particleCount=n, fieldWidth=500, fieldHeight=500)
    bodies = [nb.init_bodies(cfg, seed=900 + s) for s in range(S)]
    batch = nb.StepperBatch(S, n, cfg=cfg)
    batch.upload(bodies)
    batch.step(2)
    pts = kc.probe_points(nc.widen(bodies[0])[0], 16, seed=12, field=500)
    exp, own, counts = batch.knn(k, pts), batch.knn(k), batch.counts()
    assert exp["d2"].shape == (S, 16, k) and len(own) == S and 0 < counts.min() and counts.max() <= n
    one = nb.Stepper(cfg, capacity=n)
    for s in range(S):
        d = batch.download(s)
        P, _ = nc.widen(d)
        assert own[s]["d2"].shape == (int(counts[s]), k)
        kc.assert_same(own[s], kc.model_knn(P, k), "system %d, own" % s)
        kc.assert_same(kc.sliced(exp, s), kc.model_knn(P, k, points=pts), "system %d, points" % s)
        if s in (0, 1, 63, 64, 511, 1023):
            one.upload(d)
            kc.assert_same(own[s], one.knn(k), "system %d: Stepper, own" % s)
            kc.assert_same(kc.sliced(exp, s), one.knn(k, pts), "system %d: Stepper, points" % s)
    one.close()
    batch.close()
