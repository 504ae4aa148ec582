"""The row queries above 2^16 bodies and 2^32 pairs on the MI355X: pair counts, groups, encounters, k nearest, neighbours,
field and tracers at the sizes their kernels are described and timed at, where a row or source index passes 2^16, the pair
total passes 2^32, the triangular walk stages 782 tiles and 391 workgroups flush into one histogram, one append counter and
one log (tests/large_cases.py has the size and the states; tests/test_large_cases_cpu.py proves them on the CPU).

Every comparison is bit for bit or integer-exact, against the window references of pair_cases, group_cases and encounter_cases
and the sampled rows of model_knn and model_neighbors; the one exception is the field against the long-double oracle, with
field_cases.check_field's derived bounds.  State A (uploaded, N = 100 003) runs on an fp32 and an fp64 context, which share
one reference per query; state B (the stock configuration of 100 003 bodies in a field of 300 000, three steps on: 96 819
bodies on the CPU oracle) is fp32, the ring kernel's; the many-rows cases put 70 001 points and tracers over 300 bodies.

Measured on one MI355X, inside the whole suite (seconds per test, fp32 / fp64; the references are computed on the host inside
the first test that asks, so the fp32 case of a pair carries them; 12.3 s for the file, 13.8 s when it runs alone):
    test_pair_counts 1.00 / 0.06     test_pair_counts_with_a_nan_coordinate 0.04 / 0.04     test_groups 0.31 / 0.03
    test_encounters 0.42 / 0.15      test_knn_and_neighbors 5.19 / 0.37                     test_many_tracers 0.02 / 0.02
    test_many_rows_over_few_sources 0.89 / 0.01                                             test_stepped_state 3.79
Whole calls at N = 100 003 under the host clock (ask(), fp32): pair_counts 4.4 ms (32 ms for [0, +inf], where every pair is
binned), groups 11 to 14 ms (2 sweeps), encounters 13 to 14 ms, neighbors 8.0 ms, knn 5.3 / 7.4 / 24 ms for k = 1 / 8 / 32."""
import functools
import time

import numpy as np
import pytest

import encounter_cases as ec
import field_cases as fc
import group_cases as gc
import knn_cases as kc
import large_cases as lg
import neighbor_cases as nc
import pair_cases as pc
import tracer_cases as tc
from test_gpu_tracers import assert_same_bodies, checked_step

pytestmark = pytest.mark.gpu

CAPACITY_ERR = -7
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


def setup_module(module):
    fc.require_long_double()


def ask(what, call):
    """call() -> its result; prints the host's wall time of the call."""
    t0 = time.perf_counter()
    out = call()
    print("%-44s %8.2f ms" % (what, (time.perf_counter() - t0) * 1e3))
    return out


def bodies_of(nb, P, V, M, R, precision):
    return nb.BodiesData.from_arrays(P, V, M, R, precision)


def big_stepper(nb, precision, capacity=lg.N):
    return nb.Stepper(capacity=capacity, precision=precision, timestep=lg.DT, growthRate=0.1, fieldWidth=1000000, fieldHeight=1000000)


@pytest.fixture(scope="module", params=PRECISIONS)
def a(nb, request):
    """A context that holds state A; no test changes it."""
    assert lg.N > 92683 and lg.PAIRS == 5000250003 > 2 ** 32
    with big_stepper(nb, request.param) as st:
        st.upload(bodies_of(nb, *lg.state_a(), request.param))
        assert st.body_count() == lg.N
        yield st


# ---------------------------------------------------------------------------------------------------------------------
# 1. state A: pair counts
# ---------------------------------------------------------------------------------------------------------------------
def test_pair_counts(a):
    for name, e2 in (("pairs16", lg.E2_16), ("pairs256", lg.E2_256), ("pairs_below", lg.E2_BELOW)):
        got = ask("pair_counts %s" % name, lambda: a.pair_counts(e2, squared=True))
        print("%s: below %d, inside %d, rest %d of %d pairs" % (name, got["below"], int(got["counts"].sum()), got["rest"], got["pairs"]))
        pc.assert_same(got, lg.reference(name), name)
        pc.check_sum(got, 5000250003, name)
    assert got["below"] > 0                                       # pairs_below: the planted pairs lie under the first edge
    # one bin for everything: a count above 2^32, accumulated from 391 workgroups' flushes; no reference needed
    got = ask("pair_counts [0, +inf]", lambda: a.pair_counts(lg.E2_ALL, squared=True))
    assert (int(got["counts"][0]), got["below"], got["rest"], got["pairs"]) == (5000250003, 0, 0, 5000250003)
    pts = lg.points_a()
    got = ask("pair_counts, 300 points", lambda: a.pair_counts(lg.E2_BELOW, points=pts, squared=True))
    pc.assert_same(got, lg.reference("pairs_points"), "points")
    pc.check_sum(got, lg.FEW * lg.N, "points")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_counts_with_a_nan_coordinate(nb, precision):
    P, V, M, R = lg.state_a()
    Pn = P.copy()
    Pn[70000, 0] = np.nan                                         # its n - 1 pairs are in rest, as rows and as a source
    with big_stepper(nb, precision) as st:
        st.upload(bodies_of(nb, Pn, V, M, R, precision))
        got = st.pair_counts(lg.E2_ALL, squared=True)
        assert (got["rest"], got["below"], int(got["counts"][0])) == (lg.N - 1, 0, lg.PAIRS - (lg.N - 1))
        pc.check_sum(got, lg.PAIRS)


# ---------------------------------------------------------------------------------------------------------------------
# 2. state A: groups
# ---------------------------------------------------------------------------------------------------------------------
def test_groups(a):
    for name, link, scale in (("touching", 0.0, 1.0), ("centres", lg.CENTRE_LINK, 0.0)):
        want = lg.reference(name)
        got = ask("groups %s" % name, lambda: a.groups(link, scale))
        print("%s: %d groups, largest %d, %d sweeps" % (name, got["n_groups"], got["largest"], got["sweeps"]))
        gc.assert_same(got, want, name)
        assert 1 <= got["sweeps"] <= lg.N + 1, (name, got["sweeps"])
    assert want["largest"] >= lg.N / 2 and want["n_groups"] >= 100   # centres: the percolating component and the others
    small = lg.reference("touching")
    assert small["largest"] <= 8 and (np.bincount(small["label"]) >= 2).sum() >= 500


# ---------------------------------------------------------------------------------------------------------------------
# 3. state A: encounters
# ---------------------------------------------------------------------------------------------------------------------
def test_encounters(nb, a):
    for name, h in (("enc_0", 0.0), ("enc_dt", lg.DT), ("enc_h", lg.H)):
        got = ask("encounters h = %g" % h, lambda: a.encounters(h))
        print("h %g: %s" % (h, got[1]))
        ec.assert_same(got, lg.reference(name), name)
    want, winfo = lg.reference("enc_h")
    pairs = winfo["pairs"]
    assert pairs >= 1000 and min(ec.classes(want)) >= 100          # now, end without now, missed: at the test's horizon
    ec.assert_same(a.encounters(), lg.reference("enc_dt"), "horizon=None: the context's time step")
    info0 = lg.reference("enc_0")[1]
    assert 2 * info0["now"] == int(a.neighbors()["overlaps"].sum())
    # the C call: the counts only; one record short; the exact room
    call = nb.lib.nbody_get_encounters
    counts = (lg.N, pairs, winfo["now"], winfo["end"], winfo["missed"], lg.H)
    info = np.full(1, -7, dtype=ec.INFO_DTYPE)
    assert call(a._ctx, lg.H, None, 0, info.ctypes.data) == 0 and tuple(info[0]) == counts
    out = np.frombuffer(bytes([0x77]) * (24 * (pairs + 4)), dtype=ec.RECORD_DTYPE).copy()
    before = out.tobytes()
    info[:] = -7
    assert call(a._ctx, lg.H, out.ctypes.data, pairs - 1, info.ctypes.data) == CAPACITY_ERR    # 391 workgroups, one slot short
    assert out.tobytes() == before and tuple(info[0]) == counts
    info[:] = -7
    assert call(a._ctx, lg.H, out.ctypes.data, pairs, info.ctypes.data) == 0 and tuple(info[0]) == counts
    assert out[pairs:].tobytes() == before[24 * pairs:] and (out["reserved"][:pairs] == 0).all()
    for f in ("i", "j", "flags"):
        assert np.array_equal(out[f][:pairs], want[f]), f
    assert np.array_equal(out["t"][:pairs].view(np.uint64), want["t"].view(np.uint64))
    ec.assert_same(a.encounters(lg.H, cap=pairs - 1), (want, winfo), "the wrapper's second call")
    ec.assert_same(a.encounters(lg.H, cap=0), (want, winfo), "cap 0")


# ---------------------------------------------------------------------------------------------------------------------
# 4. state A: the k nearest and the neighbours
# ---------------------------------------------------------------------------------------------------------------------
def check_knn_own(st, n, knn_rows, ref32, ks, what):
    """knn(k) of every k on the resident state: the sampled rows against the model, every row's invariants, the prefix
    property over all rows, entry 0 with the bits of neighbors(); -> neighbors()."""
    near = ask("neighbors %s" % what, lambda: st.neighbors())
    got = {k: ask("knn(%d) %s" % (k, what), lambda: st.knn(k)) for k in ks}
    top = max(ks)
    for k in ks:
        assert got[k]["d2"].shape == (n, k), (what, k)
        kc.assert_same(kc.sliced(got[k], knn_rows), lg.knn_prefix(ref32, k), "%s, k %d" % (what, k))
        assert kc.same(kc.sliced(got[top], (slice(None), slice(0, k))), got[k]), (what, k)      # all rows
        assert np.array_equal(kc.bits(got[k]["d2"][:, 0]), kc.bits(near["d2"])) and np.array_equal(got[k]["index"][:, 0], near["index"])
    kc.check_invariants(got[top], rows=np.arange(n))
    assert (got[top]["index"] >= 0).all() and got[top]["index"].max() > 65536
    return near


def test_knn_and_neighbors(a):
    P, V, M, R = lg.state_a()
    rows, knn_rows = lg.rows_a()
    near = check_knn_own(a, lg.N, knn_rows, lg.reference("knn32"), (1, 8, 32), "state A")
    nc.assert_same(near[rows], lg.reference("neighbors"), "neighbours, sampled rows")
    pts = lg.points_a()
    nc.assert_same(a.neighbors(pts), lg.reference("neighbors_points"), "neighbours at 300 points")
    for k in (1, 8, 32):
        got = a.knn(k, pts)
        kc.assert_same(got, lg.knn_prefix(lg.reference("knn32_points"), k), "300 points, k %d" % k)
        kc.check_invariants(got)


# ---------------------------------------------------------------------------------------------------------------------
# 5. many rows over few sources: m = 70 001 over n = 300
# ---------------------------------------------------------------------------------------------------------------------
SMALL_E2 = np.linspace(0.0, 0.1 * lg.SMALL_FIELD ** 2 / np.pi, 9)


@functools.lru_cache(maxsize=None)
def many_references(m):
    """The models of the first m of the many points over the small system; the field on the 2000-point sample (all of them
    for m = 300)."""
    P, V, M, R = lg.small_system()
    pts, sample = lg.many_points()
    pts = pts[:m]
    sample = sample if m == lg.MANY else np.arange(m)
    ref = {"neighbors": nc.model_neighbors(P, R, points=pts), "knn8": kc.model_knn(P, 8, points=pts),
           "pairs": pc.model_pair_counts(P, SMALL_E2, pts), "field": fc.exact_field(P, M, points=pts[sample]), "sample": sample,
           "coincident": int(((pts[:, None, 0] == P[None, :, 0]) & (pts[:, None, 1] == P[None, :, 1])).sum())}
    return lg.freeze(ref)


def check_points(st, m, what):
    pts = lg.many_points()[0][:m]
    ref = many_references(m)
    nc.assert_same(ask("neighbors, %d points" % m, lambda: st.neighbors(pts)), ref["neighbors"], what + " neighbours")
    kc.assert_same(ask("knn(8), %d points" % m, lambda: st.knn(8, pts)), ref["knn8"], what + " knn")
    got = ask("pair_counts, %d points" % m, lambda: st.pair_counts(SMALL_E2, points=pts, squared=True))
    pc.assert_same(got, ref["pairs"], what + " pair counts")
    pc.check_sum(got, m * lg.SMALL_N, what)
    f = ask("field, %d points" % m, lambda: st.field(pts))
    acc, phi, mag, _ = ref["field"]
    assert f["acc"].shape == (m, 2) and f["coincident"] == ref["coincident"] >= lg.SMALL_N, what
    fc.check_field(f["acc"][ref["sample"]], f["phi"][ref["sample"]], acc, phi, mag, lg.SMALL_N, what + " field")
    return f


@pytest.mark.parametrize("precision", PRECISIONS)
def test_many_rows_over_few_sources(nb, precision):
    assert lg.MANY == 70001 and lg.MANY > 2 ** 16 and lg.MANY % 64 != 0
    P, V, M, R = lg.small_system()
    pts = lg.many_points()[0]
    with nb.Stepper(capacity=lg.SMALL_N, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100) as st:
        st.upload(bodies_of(nb, P, V, M, R, precision))
        f = check_points(st, lg.MANY, "m 70001")
        # a row's result does not depend on where in the grid it sits: the same points asked in two calls
        lo, hi = st.field(pts[:35000]), st.field(pts[35000:])
        assert len(hi["phi"]) == 35001 and lo["coincident"] + hi["coincident"] == f["coincident"]
        assert np.array_equal(tc.bits(np.concatenate([lo["acc"], hi["acc"]])), tc.bits(f["acc"]))
        assert np.array_equal(tc.bits(np.concatenate([lo["phi"], hi["phi"]])), tc.bits(f["phi"]))
        check_points(st, lg.FEW, "m 300 after m 70001")           # a smaller request after a larger one


# ---------------------------------------------------------------------------------------------------------------------
# 6. tracers: m = 70 001 over n = 300, two steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_many_tracers(nb, precision):
    cfg, b = tc.dense_case(nb, lg.SMALL_N, precision)
    pos, vel = tc.tracer_set(cfg, lg.MANY, seed=lg.MANY)
    assert len(pos) == 70001
    with nb.Stepper(cfg, precision=precision) as st, nb.Stepper(cfg, precision=precision) as twin:
        st.upload(b)
        twin.upload(b)
        st.set_tracers(pos, vel, walls=True)
        coin = 0
        for s in range(2):
            coin += checked_step(nb, st, twin, cfg, precision, True, s + 1, coin, "m 70001, step %d" % s)
        assert_same_bodies(st, twin, "m 70001: the bodies")


# ---------------------------------------------------------------------------------------------------------------------
# 7. state B: three steps of the stock configuration on the ring kernel
# ---------------------------------------------------------------------------------------------------------------------
B_UPLOADED, B_FIELD = 100003, 300000
B_E2 = np.geomspace(100.0 ** 2, 3000.0 ** 2, 17)


def test_stepped_state(nb):
    cfg = nb.stock_config(particleCount=B_UPLOADED, fieldWidth=B_FIELD, fieldHeight=B_FIELD)
    b = nb.init_bodies(cfg)
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as quiet:          # quiet is never asked anything until the end
        assert "ring" in st.force_kernel_name()
        st.upload(b)
        quiet.upload(b)
        st.step(3)
        quiet.step(3)
        n = st.body_count()
        print("state B: %d bodies uploaded, %d after 3 steps" % (B_UPLOADED, n))
        assert 65536 < n < B_UPLOADED                              # past a merging step: the count read from Meta
        d = st.download()
        assert d.numBodies == n
        P, V, R = ec.widen(d)
        dt = float(np.float32(cfg.timestep))
        pairs = n * (n - 1) // 2
        got = ask("state B pair_counts", lambda: st.pair_counts(B_E2, squared=True))
        pc.assert_same(got, pc.window_pair_counts(P, B_E2), "state B pair counts")
        pc.check_sum(got, pairs, "state B")
        assert got["counts"].sum() > n
        got = st.pair_counts(lg.E2_ALL, squared=True)
        assert (int(got["counts"][0]), got["below"], got["rest"]) == (pairs, 0, 0)
        link = 1.5 * 2.0 * B_FIELD / np.sqrt(n)                    # 1.5 mean spacings of the field's 2 B_FIELD width
        for name, lk, scale in (("touching", 0.0, 1.0), ("centres", link, 0.0)):
            got = ask("state B groups %s" % name, lambda: st.groups(lk, scale))
            print("state B %s: %d groups, largest %d, %d sweeps" % (name, got["n_groups"], got["largest"], got["sweeps"]))
            gc.assert_same(got, gc.window_groups(P, R, lk, scale), "state B " + name)
            assert 1 <= got["sweeps"] <= n + 1 and 1 < got["n_groups"] < n
        got = ask("state B encounters", lambda: st.encounters())
        print("state B encounters: %s" % (got[1],))
        assert got[1]["horizon"] == dt
        ec.assert_same(got, ec.window_encounters(P, V, R, dt), "state B encounters")
        assert got[1]["pairs"] > 0 and 2 * st.encounters(0.0)[1]["now"] == int(st.neighbors()["overlaps"].sum())
        rows, knn_rows = lg.sample_rows(n)
        Pw, Rw = nc.widen(d)
        near = check_knn_own(st, n, knn_rows, kc.model_knn(Pw, 32, rows=knn_rows, chunk=8), (8, 32), "state B")
        nc.assert_same(near[rows], nc.model_neighbors(Pw, Rw, rows=rows), "state B neighbours")
        # stepping on matches the context that was never asked
        st.step(2)
        quiet.step(2)
        assert_same_bodies(st, quiet, "state B, two steps on")
        assert int(st.stats().pairs) == int(quiet.stats().pairs) > 0 and st.body_count() <= n
