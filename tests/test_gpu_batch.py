"""The batched stepper (StepperBatch / nbody_batch_*) on the GPU: system s of a batch is, bit for bit, what a Stepper
gives on the same input - state, survivor count and order, pair counter, event set of every step.  Zero tolerance
throughout (NaNs compare equal to NaNs where the inputs hold some: their payloads differ between x86 and gfx950).
Reads tests/golden/ and the CPU oracle only."""
import ctypes
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_FILES = sorted(glob.glob(os.path.join(GOLD, "steps_*.npz")))
DT, GROWTH = np.float32(0.2), np.float32(0.1)
LANES = [0, 1, 2, 4, 8]            # kernel_variant: automatic, or lanes per body


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bodies_equal(got, want_block, n, what=""):
    assert got.numBodies == n, (what, got.numBodies, n)
    g, w = bits(got.block), bits(np.asarray(want_block)[:6 * n])
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError("%s: %d of %d words differ, first at %s" % (what, len(bad), len(g), bad[:8]))


def nan_aware_equal(got, want):
    g, w = np.asarray(got), np.asarray(want)
    both_nan = np.isnan(g) & np.isnan(w)
    return np.array_equal(bits(g)[~both_nan.ravel()], bits(w)[~both_nan.ravel()])


def event_sets(ev, step):
    """(E_t as sorted (i, j) pairs, D_t witnesses as sorted (i, j) pairs) of one step."""
    ev = ev[ev["step"] == step]
    return (sorted((int(e["i"]), int(e["j"])) for e in ev[ev["kind"] == 0]),
            sorted((int(e["i"]), int(e["j"])) for e in ev[ev["kind"] == 1]))


def params_of(cfg):
    return (cfg.timestep, cfg.growthRate, cfg.fieldWidth, cfg.fieldHeight)


@pytest.mark.parametrize("lanes", LANES)
def test_all_goldens_in_one_batch(nb, lanes):
    """Every golden run is one system of a single batch: N = 1, 2, 3, 100, 127..130, 200, 255, 257, 1000, 1024, 2048 and
    4096, stock radii and radii 0, sparse and dense fields, side by side in one launch, each with its own parameters."""
    zs = [np.load(p) for p in STEP_FILES]
    names = [os.path.basename(p)[6:-4] for p in STEP_FILES]
    assert len(zs) >= 17
    n0 = [int(z["n0"]) for z in zs]
    params = [(float(np.float32(z["params"][0])), float(np.float32(z["params"][1])), int(z["params"][2]),
               int(z["params"][3])) for z in zs]
    with nb.StepperBatch(len(zs), max(n0), params=params, kernel_variant=lanes) as b:
        assert ("%d lane" % lanes if lanes else "forces_batch_f32") in b.kernel_name()
        b.upload([nb.BodiesData.from_block(z["init"].view(np.float32), n) for z, n in zip(zs, n0)])
        longest = max(len(z["counts"]) for z in zs)
        for k in range(1, longest + 1):
            b.step(1)
            counts = b.counts()
            for s, z in enumerate(zs):
                rec = z["counts"]
                if k > len(rec):
                    continue
                what = "%s step %d" % (names[s], k)
                if "after_%d" % k in z:
                    assert_bodies_equal(b.download(s), z["after_%d" % k].view(np.float32), int(rec[k - 1]), what)
                else:
                    assert counts[s] == rec[k - 1], what
                if k == len(rec):      # pair counter = what the oracle says the stepper evaluates
                    ns = [n0[s]] + [int(c) for c in rec[:-1]]
                    want = sum(ol.port().oracle_pairs_per_step(n, ol.LITERAL) for n in ns)
                    st = b.stats(s)
                    assert (st.pairs, st.steps, st.n_bodies) == (want, k, int(rec[-1])), what


FIELD_OF = {77: 1000, 130: 1500, 300: 2000, 1000: 5000, 1024: 5000, 1500: 6000}   # dense: collisions in every step


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
def test_batch_equals_stepper_with_events(nb, semantics):
    rng = np.random.RandomState(20 + semantics)
    sizes = [77, 130, 300, 1000, 1024, 1500] + [int(x) for x in rng.choice(sorted(FIELD_OF), 26)]
    cfgs = [nb.stock_config(particleCount=n, fieldWidth=FIELD_OF[n], fieldHeight=FIELD_OF[n],
                            timestep=float(np.float32(0.2 + 0.01 * (s % 3))),
                            growthRate=float(np.float32(0.1 + 0.05 * (s % 2))))
            for s, n in enumerate(sizes)]
    bodies = [nb.init_bodies(cfg, seed=7000 + s) for s, cfg in enumerate(cfgs)]
    S = len(sizes)
    assert S == 32
    singles = [nb.Stepper(cfg, semantics=semantics, record_events=True) for cfg in cfgs]
    for st, bd in zip(singles, bodies):
        st.upload(bd)
    oracle = {s: [bodies[s].contiguousData.copy(), sizes[s]] for s in (3, 5)}      # N = 1000 and N = 1500
    with nb.StepperBatch(S, max(sizes), params=[params_of(c) for c in cfgs], semantics=semantics,
                         record_events=True) as b:
        b.upload(bodies)
        collided = np.zeros(S, dtype=int)
        for k in range(8):
            b.step(1)
            for st in singles:
                st.step(1)
            counts = b.counts()
            for s in range(S):
                what = "system %d (N0 = %d) step %d" % (s, sizes[s], k)
                want = singles[s].download()
                assert counts[s] == want.numBodies, what
                assert_bodies_equal(b.download(s), want.block, want.numBodies, what)
                got_ev, want_ev = event_sets(b.events(s, cap=1 << 16), k), event_sets(singles[s].events(cap=1 << 16), k)
                assert got_ev == want_ev, what
                collided[s] += len(got_ev[0]) + len(got_ev[1]) > 0
                assert b.stats(s).pairs == singles[s].stats().pairs, what
            for s, (blk, cur) in oracle.items():               # not only product against product
                cfg = cfgs[s]
                cur2, _, ab, de, _ = ol.port_step(blk, cur, np.float32(cfg.timestep), cfg.fieldWidth, cfg.fieldHeight,
                                                  np.float32(cfg.growthRate), semantics=semantics)
                oracle[s][1] = cur2
                assert_bodies_equal(b.download(s), blk, cur2, "system %d against the oracle, step %d" % (s, k))
                e_t, d_t = event_sets(b.events(s, cap=1 << 16), k)
                assert e_t == sorted((int(a), int(c)) for a, c in ab)
                assert sorted(set(i for i, _ in d_t)) == sorted(int(d) for d in de)
        # the fields ARE dense: events in most steps of most systems (a literal N = 130 walks one pair per body, quirk
        # Q1, and never collides; the smallest systems run out of partners)
        assert collided.sum() >= 4 * S, collided
    for st in singles:
        st.close()


def test_screens_and_general_path_per_system(nb):
    """A coordinate beyond 2^38, coincident bodies at zero radii, a NaN mass, an empty system and an ordinary one in one
    batch: every screen of the fast path decides per system (per tile, per wave), nothing leaks into a neighbour."""
    n = 2048
    r0 = dict(particleCount=n, minRadius=0.0, maxRadius=0.0)
    huge = nb.init_bodies(nb.stock_config(**r0), seed=11)
    huge.Positions[100] = [1e20, -3e25]                       # beyond the 2^38 coordinate bound
    huge.Positions[300] = [np.inf, 5.0]
    twins = nb.init_bodies(nb.stock_config(**r0), seed=12)
    P, M = twins.Positions, twins.Masses
    P[70] = P[5]                      # same tile, same wave
    P[200] = P[130]                   # same tile, other half
    P[1000] = P[300]                  # across tiles
    P[2040] = P[3]                    # across the wrap
    P[1500] = P[1501] = P[1502]       # three on one point
    P[1700] = P[1800]
    M[1700] = M[1800]                 # equal masses: both absorb
    nanm = nb.init_bodies(nb.stock_config(**r0), seed=13)
    nanm.Masses[1300] = np.nan
    nanm.Masses[1301] = np.inf
    empty = nb.BodiesData(0)
    plain_cfg = nb.stock_config(particleCount=1500, fieldWidth=6000, fieldHeight=6000)
    plain = nb.init_bodies(plain_cfg, seed=14)
    bodies = [huge, twins, nanm, empty, plain]
    cfg0 = nb.stock_config(**r0)
    cfgs = [cfg0, cfg0, cfg0, cfg0, plain_cfg]
    singles = {}
    for s, (cfg, bd) in enumerate(zip(cfgs, bodies)):
        if bd.numBodies:                                      # the empty system has no counterpart to run
            singles[s] = nb.Stepper(cfg, capacity=n)
            singles[s].upload(bd)
    with nb.StepperBatch(5, n, params=[params_of(c) for c in cfgs]) as b, \
            nb.StepperBatch(1, n, params=[params_of(plain_cfg)]) as alone:
        b.upload(bodies)
        alone.upload([plain])
        deleted = 0
        for k in range(4):
            b.step(1)
            alone.step(1)
            for s, st in singles.items():
                st.step(1)
                want, got = st.download(), b.download(s)
                what = "system %d step %d" % (s, k)
                assert got.numBodies == want.numBodies, what
                assert nan_aware_equal(got.block, want.block), what
                assert b.stats(s).pairs == st.stats().pairs, what
            assert b.counts()[3] == 0 and b.stats(3).pairs == 0 and b.download(3).numBodies == 0
            assert_bodies_equal(b.download(4), alone.download(0).block, alone.download(0).numBodies, "ordinary system")
            deleted = n - b.counts()[1]
        assert deleted >= 5, deleted                           # the coincident bodies did collide
    for st in singles.values():
        st.close()


def test_bulk_enqueue_equals_single_steps(nb):
    """step(25) once = 25 x step(1), on 256 stock systems of N = 1024 with seeds of their own."""
    S, n, steps = 256, 1024, 25
    cfg = nb.stock_config(particleCount=n)
    bodies = [nb.init_bodies(cfg, seed=1 + s) for s in range(S)]
    with nb.StepperBatch(S, n, cfg=cfg) as bulk, nb.StepperBatch(S, n, cfg=cfg) as single:
        bulk.upload(bodies)
        single.upload(bodies)
        bulk.step(steps)
        for _ in range(steps):
            single.step(1)
            single.sync()
        a, c = bulk.download_all(), single.download_all()
        for s in range(S):
            assert_bodies_equal(a[s], c[s].block, c[s].numBodies, "system %d" % s)
        assert bulk.stats(0).steps == steps
        for s in (0, 1, 37, 100, 128, 200, 254, 255):
            with nb.Stepper(cfg) as st:
                st.upload(bodies[s])
                st.step(steps)
                want = st.download()
                assert_bodies_equal(a[s], want.block, want.numBodies, "system %d against Stepper" % s)
                assert bulk.stats(s).pairs == st.stats().pairs
        assert len(set(x.numBodies for x in a)) > 1 or any(x.numBodies < n for x in a)   # the seeds do differ


def test_four_thousand_systems(nb):
    """systems = 4096 (the system index is gridDim.y), ragged small N, a reused context: upload restarts everything."""
    S, cap = 4096, 130
    sizes = [1 + (s * 37) % cap for s in range(S)]
    cfgs = {n: nb.stock_config(particleCount=n, fieldWidth=3000, fieldHeight=3000) for n in set(sizes)}
    bodies = [nb.init_bodies(cfgs[n], seed=s) for s, n in enumerate(sizes)]
    with nb.StepperBatch(S, cap, cfg=cfgs[cap], record_events=True, event_capacity=1024) as b:
        for _ in range(2):
            b.upload(bodies)
            assert b.stats(5).steps == 0 and b.stats(5).pairs == 0 and len(b.events(5, cap=1024)) == 0
            b.step(3)
            for s in (0, 1, 127, 128, 129, 2047, 4095):
                with nb.Stepper(cfgs[sizes[s]], record_events=True) as st:
                    st.upload(bodies[s])
                    st.step(3)
                    want = st.download()
                    assert_bodies_equal(b.download(s), want.block, want.numBodies, "system %d" % s)
                    assert [event_sets(b.events(s, cap=1024), k) for k in range(3)] == \
                           [event_sets(st.events(cap=1 << 12), k) for k in range(3)]


def test_failure_is_reported_not_trusted(nb):
    """Bad calls on a live batch return the documented status and leave it usable; no device fault is provoked."""
    cfg = nb.stock_config(particleCount=100, fieldWidth=3000, fieldHeight=3000)
    ok = nb.init_bodies(cfg, seed=3)
    big = nb.init_bodies(nb.stock_config(particleCount=101), seed=3)
    with nb.StepperBatch(2, 100, cfg=cfg) as b:
        with pytest.raises(nb.NbodyError) as ei:
            b.step(1)
        assert ei.value.status == -9                           # step before upload
        with pytest.raises(nb.NbodyError) as ei:
            b.upload([ok, big])                                # 101 bodies > capacity 100
        assert ei.value.status == -1 and "system 1" in str(ei.value)
        L = nb.lib
        ptrs = (ctypes.c_void_p * 2)(ok.ptr, ok.ptr)
        assert L.nbody_batch_upload(b._b, ptrs, (ctypes.c_int * 2)(100, -1)) == -1
        assert L.nbody_batch_upload(b._b, (ctypes.c_void_p * 2)(ok.ptr, None), (ctypes.c_int * 2)(100, 0)) == -1
        assert L.nbody_batch_upload(b._b, None, (ctypes.c_int * 2)(100, 0)) == -1
        b.upload([ok, nb.BodiesData(0)])
        b.step(2)
        for bad in (-1, 2, 1 << 20):
            with pytest.raises(nb.NbodyError) as ei:
                b.download(bad)
            assert ei.value.status == -1
            with pytest.raises(nb.NbodyError) as ei:
                b.stats(bad)
            assert ei.value.status == -1
            with pytest.raises(nb.NbodyError) as ei:
                b.events(bad)
            assert ei.value.status == -1
        with nb.Stepper(cfg) as st:                            # and the batch still computes
            st.upload(ok)
            st.step(2)
            want = st.download()
            assert_bodies_equal(b.download(0), want.block, want.numBodies, "after the refused calls")
        assert b.download(1).numBodies == 0
        b.sync()
