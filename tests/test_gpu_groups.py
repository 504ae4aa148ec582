"""Group finding (nbody_get_groups, nbody_batch_get_groups; Stepper.groups, StepperGroup.groups, StepperBatch.groups) on the
MI355X: friends-of-friends labels of the resident state.

The definition has no fma and rounds every operation on its own, so the numpy model of group_cases.py restates the links
bit for bit and a label is the lowest index of its component whichever way it is found: zero tolerance throughout - every
label against the model, and product against product (another rank, a batch against a Stepper holding the same state)."""
import ctypes

import numpy as np
import pytest

import group_cases as gc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
DTYPE_OF = {0: np.float32, 1: np.float64}


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=capacity, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)


def bodies_of(nb, P, R, precision):
    n = len(R)
    return nb.BodiesData.from_arrays(P, np.zeros((n, 2)), np.ones(n), R, precision)


def check(st, P, R, link, scale, what):
    """Stepper.groups on the resident state against the model of (P, R); -> the result."""
    got = st.groups(link, scale)
    want = gc.model_groups(P, R, link, scale)
    n = len(R)
    print("%s: n %d link %g scale %g -> %d groups, largest %d, %d sweeps" % (what, n, link, scale, got["n_groups"], got["largest"],
                                                                               got["sweeps"]))
    gc.assert_same(got, want, what)
    assert 1 <= got["sweeps"] <= n + 1, what
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. random states: many small groups, one percolating group over three tiles, the overlap predicate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_random_states(nb, precision):
    P, R = gc.random_state(300, DTYPE_OF[precision], seed=11, field=100)
    with small_stepper(nb, precision, 1000) as st:
        st.upload(bodies_of(nb, P, R, precision))
        many = check(st, P, R, 4.0, 1.0, "many small groups")
        assert many["n_groups"] > 20 and many["largest"] > 5
        one = check(st, P, R, 6.0, 1.0, "percolating")
        assert one["largest"] > 256                               # spans the three tiles and both workgroups
        touch = check(st, P, R, 0.0, 1.0, "the overlap predicate")
        label = touch["label"]
        singleton = np.bincount(label, minlength=300)[label] == 1
        assert np.array_equal(singleton, st.neighbors()["overlaps"] == 0)
        P, R = gc.random_state(1000, DTYPE_OF[precision], seed=11, field=100)
        st.upload(bodies_of(nb, P, R, precision))
        centres = check(st, P, R, 2.0, 0.0, "centres only, n 1000")
        assert 100 < centres["n_groups"] < 1000


# ---------------------------------------------------------------------------------------------------------------------
# 2. tile and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------
# 63 .. 65: the cut at the wave's last row inside tile 0; 191 .. 193: the third wave, cut at 64 entries of tile 1; 385: a second
# workgroup whose first wave has self tile 2
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_tile_edges(nb, precision, n):
    P, R = gc.random_state(n, DTYPE_OF[precision], seed=n, field=5.0 * np.sqrt(n))
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, P, R, precision))
        for link, scale in ((1.0, 1.0), (0.0, 1.0), (np.inf, 0.0)):
            got = check(st, P, R, link, scale, "n %d" % n)
            if link == np.inf:
                assert (got["label"] == 0).all() and (got["n_groups"], got["largest"]) == (1, n)
        if n == 1:
            assert got["label"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. special states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_shuffled_chain(nb, precision):
    P, R = gc.shuffled_chain(300)
    with small_stepper(nb, precision, 300) as st:
        st.upload(bodies_of(nb, P, R, precision))
        one = check(st, P, R, 0.5, 1.0, "chain, linked")          # 1 <= sweeps <= n + 1 is asserted there
        assert (one["label"] == 0).all() and (one["n_groups"], one["largest"]) == (1, 300)
        none = check(st, P, R, 0.25, 1.0, "chain, apart")
        assert np.array_equal(none["label"], np.arange(300)) and (none["n_groups"], none["largest"]) == (300, 1)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lattice_equality_counts(nb, precision):
    P, R = gc.lattice(8, 0.25)
    with small_stepper(nb, precision, 64) as st:
        st.upload(bodies_of(nb, P, R, precision))
        assert check(st, P, R, 0.5, 1.0, "lattice, d2 == s*s == 1")["n_groups"] == 1
        assert check(st, P, R, 0.49, 1.0, "lattice, just short")["n_groups"] == 64


@pytest.mark.parametrize("precision", PRECISIONS)
def test_awkward_values(nb, precision):
    P, R = gc.random_state(130, DTYPE_OF[precision], seed=2, field=30.0, radius=1.0)
    with small_stepper(nb, precision, 130) as st:
        Pn = P.copy()
        Pn[7, 0] = np.nan                                         # a NaN coordinate is a singleton, whatever the link
        st.upload(bodies_of(nb, Pn, R, precision))
        got = check(st, Pn, R, 0.5, 1.0, "NaN coordinate")
        assert got["label"][7] == 7 and (got["label"] == 7).sum() == 1
        got = check(st, Pn, R, np.inf, 1.0, "NaN coordinate, link +inf")
        assert got["n_groups"] == 2 and got["label"][7] == 7
        st.upload(bodies_of(nb, P, R, precision))
        got = check(st, P, R, np.inf, 1.0, "link +inf, n 130")
        assert (got["label"] == 0).all() and got["largest"] == 130
        C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])
        st.upload(bodies_of(nb, C, np.zeros(3), precision))
        got = check(st, C, np.zeros(3), 0.0, 1.0, "coincident, radii 0, link 0")
        assert got["label"].tolist() == [0, 1, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. a real state, and no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
def test_real_state_and_no_effect_on_stepping(nb):
    cfg = nb.stock_config(particleCount=1000, fieldWidth=5000, fieldHeight=5000)
    b = nb.init_bodies(cfg)
    with nb.Stepper(cfg) as st, nb.Stepper(cfg) as plain:
        st.upload(b)
        plain.upload(b)
        st.step(3)
        d = st.download()
        P, R = gc.widen(d)
        assert d.numBodies < 1000
        first = check(st, P, R, 0.0, 1.0, "after 3 literal steps")
        again = st.groups(0.0, 1.0)
        assert np.array_equal(first["label"], again["label"]) and first["n_groups"] == again["n_groups"]
        check(st, P, R, 250.0, 0.0, "after 3 literal steps, centres")
        st.step(1)
        plain.step(4)
        a, c = st.download(), plain.download()
        assert a.numBodies == c.numBodies and a.block.view(np.uint32).tobytes() == c.block.view(np.uint32).tobytes()
        assert int(st.stats().pairs) == int(plain.stats().pairs)


# ---------------------------------------------------------------------------------------------------------------------
# 5. not collective
# ---------------------------------------------------------------------------------------------------------------------
def test_either_rank_of_a_group(nb):
    cfg = nb.stock_config(particleCount=1000, fieldWidth=5000, fieldHeight=5000)
    grp = nb.StepperGroup(2, cfg=cfg)
    grp.upload(nb.init_bodies(cfg))
    grp.step(2)
    P, R = gc.widen(grp.download())
    want = gc.model_groups(P, R, 30.0, 1.0)
    assert 1 < want["n_groups"] < len(R)
    for rank in (1, 0):                                           # each on its own
        gc.assert_same(grp.groups(30.0, rank=rank), want, "rank %d" % rank)
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors on a live context
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    P, R = gc.random_state(300, np.float32, seed=11, field=100)
    call = nb.lib.nbody_get_groups
    label = np.full(300, -7, dtype=np.int32)
    info = np.full(1, -7, dtype=gc.INFO_DTYPE)
    untouched = (label.tobytes(), info.tobytes())
    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, 300, info.ctypes.data) == STATE_ERR      # before an upload
        assert b"before" in nb.lib.nbody_last_error_string()
        st.upload(bodies_of(nb, P, R, 0))
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, 299, info.ctypes.data) == CAPACITY_ERR
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, -1, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, 1.0, None, 300, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, 300, None) == INVALID
        assert call(st._ctx, -1.0, 1.0, label.ctypes.data, 300, info.ctypes.data) == INVALID
        assert call(st._ctx, np.nan, 1.0, label.ctypes.data, 300, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, np.inf, label.ctypes.data, 300, info.ctypes.data) == INVALID
        assert (label.tobytes(), info.tobytes()) == untouched
        assert call(st._ctx, 4.0, 1.0, label.ctypes.data, 300, info.ctypes.data) == 0
        want = gc.model_groups(P, R, 4.0)
        assert np.array_equal(label, want["label"])
        assert tuple(info[0])[:3] == (300, want["n_groups"], want["largest"]) and 1 <= info["sweeps"][0] <= 301
        st.upload(nb.BodiesData(0))                               # no bodies: nothing launched
        assert call(st._ctx, 4.0, 1.0, label.ctypes.data, 0, info.ctypes.data) == 0
        assert tuple(info[0]) == (0, 0, 0, 0) and np.array_equal(label, want["label"])
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, 100, 100)] * 2) as batch:
        labels = np.full((2, 300), -7, dtype=np.int32)
        infos = np.full(2, -7, dtype=gc.INFO_DTYPE)
        bcall = nb.lib.nbody_batch_get_groups
        assert bcall(batch._b, 1.0, 1.0, labels.ctypes.data, infos.ctypes.data) == STATE_ERR
        batch.upload([bodies_of(nb, P, R, 0), nb.BodiesData(0)])
        assert bcall(batch._b, 1.0, 1.0, None, infos.ctypes.data) == INVALID
        assert bcall(batch._b, 1.0, 1.0, labels.ctypes.data, None) == INVALID
        assert bcall(batch._b, 1.0, -2.0, labels.ctypes.data, infos.ctypes.data) == INVALID
        assert (labels == -7).all() and (infos["sweeps"] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_COUNTS = [0, 1, 127, 300, 129, 63, 64, 65, 193]


@pytest.mark.parametrize("track_ids", [False, True], ids=["plain", "track_ids"])
def test_batch_equals_stepper_and_model(nb, track_ids):
    cap, S = 300, len(BATCH_COUNTS)
    states = [gc.random_state(n, np.float32, seed=60 + s, field=max(6.0 * np.sqrt(n), 1.0)) for s, n in enumerate(BATCH_COUNTS)]
    bodies = [bodies_of(nb, P, R, 0) if len(R) else nb.BodiesData(0) for P, R in states]
    params = [(0.2, 0.1, 100, 100)] * S
    with nb.StepperBatch(S, cap, params=params, track_ids=track_ids) as batch, small_stepper(nb, 0, cap) as one:
        batch.upload(bodies)
        for link, scale in ((1.0, 1.0), (0.0, 1.0), (2.0, 0.0)):
            got = batch.groups(link, scale)
            assert len(got) == S
            raw = np.full((S, cap), -77, dtype=np.int32)          # the C call into a prefilled buffer: the tails stay
            infos = np.zeros(S, dtype=gc.INFO_DTYPE)
            assert nb.lib.nbody_batch_get_groups(batch._b, link, scale, raw.ctypes.data, infos.ctypes.data) == 0
            sweeps = got[0]["sweeps"]
            assert 1 <= sweeps <= max(BATCH_COUNTS) + 1
            for s, (P, R) in enumerate(states):
                n = BATCH_COUNTS[s]
                what = "system %d (n %d) link %g scale %g" % (s, n, link, scale)
                assert got[s]["sweeps"] == sweeps and infos["sweeps"][s] >= 1, what   # the one number of the whole call
                assert np.array_equal(raw[s, :n], got[s]["label"]) and (raw[s, n:] == -77).all(), what
                assert tuple(infos[s])[:3] == (n, got[s]["n_groups"], got[s]["largest"]), what
                gc.assert_same(got[s], gc.model_groups(P, R, link, scale), what + ": model")
                if n == 0:
                    assert (got[s]["n_groups"], got[s]["largest"]) == (0, 0) and got[s]["label"].shape == (0,)
                    continue
                one.upload(bodies[s])
                gc.assert_same(got[s], one.groups(link, scale), what + ": Stepper")
            assert 1 < got[3]["n_groups"] < 300                   # the full system is neither one clump nor all singletons
