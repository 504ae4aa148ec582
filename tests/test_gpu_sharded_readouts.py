"""Every read-out of a sharded context past the exchange lag (run with -m gpu on an MI355X).

The read-outs - nbody_group_diagnostics, nbody_get_field, nbody_get_neighbors, nbody_get_groups, nbody_render_image and the
state file - were each checked on a StepperGroup two steps after an upload, inside nbody_ctx::kLag = 4: the slots still
laid out for the uploaded count, every rank with its first range; nbody_get_knn and nbody_get_pair_counts, which came
later, each at one state on two or three ranks.  Here the runs of sharded_cases.py go 12 steps on 8 and 3
ranks (fp32 and fp64) and on the single-rank RCCL context; the count falls below a quarter, ranks - the gathering rank 0
among them - lose their range, others keep a ragged tail, and the gather areas shrink (tests/test_sharded_cases_cpu.py
proves all of that on the CPU oracle).

After EVERY step the state is anchored: the download equals the oracle bit for bit, every rank's own range is
nbody_partition's, the ranges tile [0, n).  A read-out that then disagrees with its model is wrong itself.  At the
checkpoints (upload, after steps 4, 5, 8, 12) every read-out is taken through every rank - the ranks that own nothing
included - and compared with the models (exact_phi / check_totals / check_phi, field_cases, neighbor_cases, group_cases,
knn_cases, pair_cases, the oracle's renderer) and with a plain Stepper that is stepped alongside and holds the same bits.
Every comparison is exact but the two against long-double references, which use the bounds their own test files derive."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import field_cases as fc
import group_cases as gc
import knn_cases as kc
import lineage_cases as lc
import neighbor_cases as nc
import oracle_lib as ol
import pair_cases as pc
import sharded_cases as sc
import test_gpu_diagnostics as dg
import test_gpu_field as gf
from sharded_cases import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = pytest.mark.parametrize("run", sc.RUNS, ids=sc.RUN_IDS)
KINDS = [pytest.param(8, 0, id="world8-f32"), pytest.param(8, 1, id="world8-f64"), pytest.param(3, 0, id="world3-f32"),
         pytest.param(3, 1, id="world3-f64"), pytest.param("rccl", 0, id="rccl-f32")]


def setup_module(module):
    fc.require_long_double()


@functools.lru_cache(maxsize=None)
def status_codes():
    """NBODY_ERR_* by name, from include/nbody.h."""
    with open(os.path.join(ROOT, "include", "nbody.h")) as f:
        return {name: int(value) for name, value in re.findall(r"\bNBODY_ERR_(\w+) = (-\d+)", f.read())}


def ranks_of(ctx):
    return getattr(ctx, "ranks", None) or [ctx]


def make_ctx(nb, kind, cfg, precision, semantics, **kw):
    """kind: a StepperGroup of that many ranks, or "rccl": one rank with a communicator (every gather goes through RCCL)."""
    if kind == "rccl":
        return nb.Stepper(cfg, precision=precision, semantics=semantics, comm_id=nb.comm_unique_id(), force_comm=True, **kw)
    return nb.StepperGroup(kind, cfg=cfg, precision=precision, semantics=semantics, **kw)


def assert_block(got, want, what):
    """A download against a state of the oracle: the count and every bit (the runs hold no NaN)."""
    assert got.numBodies == want.n, (what, got.numBodies, want.n)
    assert np.array_equal(bits(got.block), bits(want.block)), what


def assert_anchor(nb, ctx, want, what):
    """The cheap checks of every step; -> the download."""
    got = ctx.download()
    assert_block(got, want, what)
    ranks = ranks_of(ctx)
    ranges = [r.own_range() for r in ranks]
    assert ranges == want.ranges(nb, len(ranks)), (what, ranges)
    assert ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == want.n, (what, ranges)
    assert all(ranges[r][0] + ranges[r][1] == ranges[r + 1][0] for r in range(len(ranks) - 1)), (what, ranges)
    for g, r in enumerate(ranks):
        st = r.stats()
        assert (st.n_bodies, st.n_own, st.steps) == (want.n, ranges[g][1], want.step), (what, g, st.n_bodies, st.n_own, st.steps)
    return got


@functools.lru_cache(maxsize=None)
def probe_points(run):
    import ppa_nbody_collisions_amd as nb
    pts = gf.probe_points(lc.dense_cfg(nb, run[0]), sc.POINTS, 8)
    pts.setflags(write=False)
    return pts


KNN_K = 9                                                       # one past a tier boundary of the k nearest


def pair_edges2(run):
    """The squared edges of the pair counts of a run: 10 geometric bins up to a quarter of the field."""
    return np.geomspace(1.0, float(lc.FIELD_OF[run[0]]) ** 2 / 16.0, 11)


@functools.lru_cache(maxsize=None)
def references(run, precision, step):
    """What the models say about the oracle's state after `step` steps - the state every context under test has been shown
    to hold bit for bit before it is asked.  Computed once per state, shared by every context, never written to."""
    import ppa_nbody_collisions_amd as nb
    st = sc.trajectory(*run, precision)[step]
    b = nb.BodiesData.from_block(st.block, st.n, precision)
    P, V, M = dg.state_arrays(b)
    Pw, Rw = nc.widen(b)
    pts = probe_points(run)
    ref = {"P": P, "V": V, "M": M, "n": st.n}
    ref["phi"], ref["coincident"] = dg.exact_phi(P, M, np.arange(st.n))
    ref["neighbors"] = nc.model_neighbors(Pw, Rw)
    ref["neighbors_at_points"] = nc.model_neighbors(Pw, Rw, points=pts)
    ref["touching"] = gc.model_groups(Pw, Rw, 0.0, 1.0)
    ref["centres"] = gc.model_groups(Pw, Rw, sc.CENTRE_LINK[run], 0.0)
    assert 1 < ref["centres"]["n_groups"] < st.n, (run, step, ref["centres"]["n_groups"])
    ref["knn"] = kc.model_knn(Pw, KNN_K)
    ref["knn_at_points"] = kc.model_knn(Pw, KNN_K, points=pts)
    ref["pairs"] = pc.model_pair_counts(Pw, pair_edges2(run))
    ref["pairs_at_points"] = pc.model_pair_counts(Pw, pair_edges2(run), pts)
    assert st.n > KNN_K and ref["pairs"]["counts"].sum() > 0 and ref["pairs_at_points"]["counts"].sum() > 0, (run, step)
    if step in sc.EXACT_FIELD_AT:
        ref["field"] = fc.exact_field(P, M, rows=np.arange(st.n))
        ref["field_at_points"] = fc.exact_field(P, M, points=pts)
    if precision == nb.F32:
        w, h = sc.IMAGE
        field = lc.FIELD_OF[run[0]]
        ref["image"] = ol.port_render(np.array(st.block), st.n, st.render_blocks(run[1]), w, h, field, field)
    return ref


def check_readouts(nb, ctx, plain, got, run, precision, step, what):
    """Every read-out of `ctx`, whose download `got` equals the oracle's state after `step` steps, through every rank."""
    ref = references(run, precision, step)
    n, pts = ref["n"], probe_points(run)
    ranks = ranks_of(ctx)
    own = [r.own_range()[1] for r in ranks]
    assert_block(plain.download(), sc.trajectory(*run, precision)[step], what + ": the plain context")
    # diagnostics: twice, against the plain context, against the long-double oracle of the downloaded arrays
    d = ctx.diagnostics(potential=True)
    assert dg.diag_bits(ctx.diagnostics(potential=True)) == dg.diag_bits(d), what + ": diagnostics, called again"
    assert dg.diag_bits(plain.diagnostics(potential=True)) == dg.diag_bits(d), what + ": diagnostics, plain context"
    assert (d["step"], d["n_bodies"], d["phi"].shape) == (step, n, (n,)), (what, d["step"], d["n_bodies"])
    P, V, M = dg.state_arrays(got)
    assert all(np.array_equal(a, b) for a, b in zip((P, V, M), (ref["P"], ref["V"], ref["M"])))
    dg.check_phi(d["phi"], ref["phi"], n, what)
    assert d["coincident_pairs"] == ref["coincident"], what
    dg.check_totals(d, P, V, M, ref["phi"], what)
    # field: every rank, the ones that own nothing too; own positions and explicit points
    plain_own, plain_pts = plain.field(), plain.field(pts)
    for g, r in enumerate(ranks):
        w = "%s: field through rank %d (owns %d)" % (what, g, own[g])
        f_own, f_pts = r.field(), r.field(pts)
        assert f_own["acc"].shape == (n, 2) and f_pts["acc"].shape == (sc.POINTS, 2), w
        assert gf.field_bits(f_own) == gf.field_bits(plain_own), w
        assert gf.field_bits(f_pts) == gf.field_bits(plain_pts), w + ", points"
        assert np.array_equal(gf.bits(f_own["phi"]), gf.bits(d["phi"])) and f_own["coincident"] == d["coincident_pairs"], w
        if "field" in ref:
            acc, phi, mag, coin = ref["field"]
            assert f_own["coincident"] == coin, w
            fc.check_field(f_own["acc"], f_own["phi"], acc, phi, mag, n, w)
            acc, phi, mag, coin = ref["field_at_points"]
            assert f_pts["coincident"] == coin == 0, w
            fc.check_field(f_pts["acc"], f_pts["phi"], acc, phi, mag, n, w + ", points")
    # neighbours and groups: the bit-exact models
    for g, r in enumerate(ranks):
        w = "%s: rank %d (owns %d)" % (what, g, own[g])
        nc.assert_same(r.neighbors(), ref["neighbors"], w + " neighbours")
        nc.assert_same(r.neighbors(pts), ref["neighbors_at_points"], w + " neighbours at points")
        for key, link, scale in (("touching", 0.0, 1.0), ("centres", sc.CENTRE_LINK[run], 0.0)):
            grp = r.groups(link, scale)
            gc.assert_same(grp, ref[key], "%s groups %s" % (w, key))
            assert 1 <= grp["sweeps"] <= n + 1, (w, key, grp["sweeps"])
    # the k nearest and the pair counts: the bit-exact models and the plain context, own rows and explicit points
    e2 = pair_edges2(run)
    kc.assert_same(plain.knn(KNN_K), ref["knn"], what + ": knn, plain context")
    kc.assert_same(plain.knn(KNN_K, pts), ref["knn_at_points"], what + ": knn at points, plain context")
    pc.assert_same(plain.pair_counts(e2, squared=True), ref["pairs"], what + ": pair counts, plain context")
    pc.assert_same(plain.pair_counts(e2, points=pts, squared=True), ref["pairs_at_points"], what + ": pair counts at points, plain context")
    for g, r in enumerate(ranks):
        w = "%s: rank %d (owns %d)" % (what, g, own[g])
        kc.assert_same(r.knn(KNN_K), ref["knn"], w + " knn")
        kc.assert_same(r.knn(KNN_K, pts), ref["knn_at_points"], w + " knn at points")
        got_pairs = r.pair_counts(e2, squared=True)
        pc.assert_same(got_pairs, ref["pairs"], w + " pair counts")
        pc.check_sum(got_pairs, n * (n - 1) // 2, w)
        got_pairs = r.pair_counts(e2, points=pts, squared=True)
        pc.assert_same(got_pairs, ref["pairs_at_points"], w + " pair counts at points")
        pc.check_sum(got_pairs, sc.POINTS * n, w)
    # render: fp32 against the oracle's renderer on the downloaded block, fp64 (the oracle draws fp32 only) against the
    # plain context
    width, height = sc.IMAGE
    want = ref["image"] if precision == nb.F32 else plain.render_image(width, height)
    assert (want != 254).any() and (want == 254).any(), what
    for g, r in enumerate(ranks):
        img = r.render_image(width, height)
        assert img.shape == (height, width) and np.array_equal(img, want), "%s: image of rank %d (owns %d)" % (what, g, own[g])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the read-outs along a run
# ---------------------------------------------------------------------------------------------------------------------
@RUNS
@pytest.mark.parametrize("kind,precision", KINDS)
def test_readouts_along_a_collapsing_run(nb, kind, precision, run):
    n0, semantics = run
    cfg, bodies = lc.dense_bodies(nb, n0, precision)
    traj = sc.trajectory(n0, semantics, precision)
    assert np.array_equal(bits(bodies.block), bits(traj[0].block))
    ctx = make_ctx(nb, kind, cfg, precision, semantics)
    quiet = make_ctx(nb, kind, cfg, precision, semantics)          # never asked anything until the end
    plain = nb.Stepper(cfg, precision=precision, semantics=semantics)
    try:
        for c in (ctx, quiet, plain):
            c.upload(bodies)
        emptied = set()
        for want in traj:
            what = "n0 %d %s %s step %d" % (n0, "clean" if semantics else "literal", kind, want.step)
            if want.step:
                for c in (ctx, quiet, plain):
                    c.step(1)
            got = assert_anchor(nb, ctx, want, what)
            emptied |= {g for g, r in enumerate(ranks_of(ctx)) if r.own_range()[1] == 0}
            if want.step in sc.CHECKPOINTS:
                check_readouts(nb, ctx, plain, got, run, precision, want.step, what)
        if (kind, n0) in ((8, 1500), (3, 1000)):
            assert 0 in emptied, emptied                            # the gathering rank has lost its range on the way
        # no effect on stepping: the group that was never asked holds the same bits and has walked the same pairs
        end = ctx.download()
        assert_block(quiet.download(), traj[-1], "the context that was never asked")
        assert_block(end, traj[-1], "the context that was asked")
        assert sum(r.stats().pairs for r in ranks_of(ctx)) == sum(r.stats().pairs for r in ranks_of(quiet)) > 0
    finally:
        for c in (ctx, quiet, plain):
            c.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. state files
# ---------------------------------------------------------------------------------------------------------------------
def peek(nb, path):
    prec, n, steps = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    assert nb.lib.nbody_state_peek(os.fsencode(path), ctypes.byref(prec), ctypes.byref(n), ctypes.byref(steps)) == 0
    return prec.value, n.value, steps.value


def payload(path, precision):
    return np.fromfile(path, dtype=np.uint64 if precision else np.uint32, offset=64)


@RUNS
def test_rccl_context_state_file(nb, run, tmp_path):
    """The RCCL-path context saves through its collective download: after step 8 the file is the state, and a plain context
    goes on from it to the oracle's step 12."""
    n0, semantics = run
    cfg, bodies = lc.dense_bodies(nb, n0)
    traj = sc.trajectory(n0, semantics, nb.F32)
    path = str(tmp_path / "rccl.nbody")
    with make_ctx(nb, "rccl", cfg, nb.F32, semantics) as rc, nb.Stepper(cfg, semantics=semantics) as plain:
        rc.upload(bodies)
        rc.step(8)
        got = assert_anchor(nb, rc, traj[8], "RCCL context, step 8")
        rc.save_state(path)
        assert peek(nb, path) == (nb.F32, traj[8].n, 8)
        assert os.path.getsize(path) == 64 + 24 * traj[8].n
        assert np.array_equal(payload(path, nb.F32), bits(got.block))
        plain.load_state(path)
        assert plain.stats().steps == 8
        plain.step(4)
        assert_block(plain.download(), traj[12], "a plain context from the RCCL context's file, 4 steps on")
        rc.step(4)                                                  # and the save left the saving context as it was
        assert_block(rc.download(), traj[12], "the RCCL context, 4 steps after its save")


def test_state_file_refusals_on_a_live_context(nb, tmp_path):
    """Every refusal of nbody_state_load returns its documented status and leaves the context as it was: it then steps
    once and equals the oracle."""
    err = status_codes()
    run = (1000, ol.CLEAN)
    cfg, bodies = lc.dense_bodies(nb, run[0])
    traj = sc.trajectory(*run, nb.F32)
    good = str(tmp_path / "good.nbody")
    raw = None

    def damaged(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        return p

    with nb.Stepper(cfg, semantics=run[1]) as st:
        st.upload(bodies)
        st.save_state(good)
        raw = open(good, "rb").read()
        assert len(raw) == 64 + 24 * run[0] and raw[:8] == b"NBODYST1" and peek(nb, good) == (nb.F32, run[0], 0)
        as_f64 = bytearray(raw)
        as_f64[8:12] = np.int32(nb.F64).tobytes()                   # the precision field of the header
        cases = [("truncated by one byte", damaged("short.nbody", raw[:-1]), err["PARSE"]),
                 ("an fp64 file", damaged("f64.nbody", bytes(as_f64)), err["INVALID"]),
                 ("a wrong magic", damaged("magic.nbody", b"NBODYST2" + raw[8:]), err["PARSE"])]
        for k, (name, path, status) in enumerate(cases):
            with pytest.raises(nb.NbodyError) as e:
                st.load_state(path)
            assert e.value.status == status, (name, e.value.status, str(e.value))
            assert st.stats().steps == k                            # neither the state nor the step counter moved
            st.step(1)
            assert_block(st.download(), traj[k + 1], "one step after refusing " + name)
    # a file of n bodies into a context of capacity n - 1, which holds a state of its own
    m = run[0] - 1
    small = nb.BodiesData.from_arrays(bodies.Positions[:m], bodies.Velocities[:m], bodies.Masses[:m], bodies.Radii[:m])
    blk = small.block.copy()
    with nb.Stepper(cfg, capacity=m, semantics=run[1]) as st:
        st.upload(small)
        with pytest.raises(nb.NbodyError) as e:
            st.load_state(good)
        assert e.value.status == err["CAPACITY"], (e.value.status, str(e.value))
        st.step(1)
        n1, *_ = ol.port_step(blk, m, np.float32(cfg.timestep), cfg.fieldWidth, cfg.fieldHeight, np.float32(cfg.growthRate),
                              semantics=run[1], want_events=False)
        out = st.download()
        assert out.numBodies == n1 < m and np.array_equal(bits(out.block), bits(blk[:6 * n1]))
    assert len({err["PARSE"], err["INVALID"], err["CAPACITY"], 0}) == 4 and open(good, "rb").read() == raw


def test_state_of_no_bodies_round_trips(nb, tmp_path):
    cfg, bodies = lc.dense_bodies(nb, 1000)
    path = str(tmp_path / "empty.nbody")
    with nb.Stepper(cfg) as a, nb.Stepper(cfg) as b:
        a.upload(nb.BodiesData(0))
        assert nb.lib.nbody_ctx_set_steps(a._ctx, 7) == 0           # a counter a fresh upload does not have
        a.save_state(path)
        assert os.path.getsize(path) == 64 and peek(nb, path) == (nb.F32, 0, 7)
        b.upload(bodies)                                            # the loading context holds something else
        b.step(1)
        b.load_state(path)
        assert b.body_count() == 0 and b.download().numBodies == 0
        assert (b.stats().steps, b.stats().n_bodies) == (7, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the checkpoint of a sharded run
# ---------------------------------------------------------------------------------------------------------------------
def test_rank_of_a_group_refuses_to_save(nb, tmp_path):
    """A rank of a group holds its own velocities only, nbody_download gives zeros for the rest: nbody_state_save refuses
    (NBODY_ERR_STATE, naming the group call) instead of writing a file that is not the state."""
    run = (1000, ol.CLEAN)
    cfg, bodies = lc.dense_bodies(nb, run[0])
    traj = sc.trajectory(*run, nb.F32)
    fresh, kept = str(tmp_path / "never_written.nbody"), str(tmp_path / "kept.nbody")
    with open(kept, "wb") as f:
        f.write(b"what was here before")
    grp = nb.StepperGroup(3, cfg=cfg, semantics=run[1])
    try:
        grp.upload(bodies)
        grp.step(6)
        whole = assert_anchor(nb, grp, traj[6], "step 6")
        assert whole.Velocities.any(axis=1).all()                   # every body moves: a zero velocity is not the state
        for g, r in enumerate(grp.ranks):
            for path in (fresh, kept):
                with pytest.raises(nb.NbodyError) as e:
                    r.save_state(path)
                assert e.value.status == status_codes()["STATE"], (g, e.value.status)
                assert "nbody_group_state_save" in str(e.value), str(e.value)
            assert not os.path.exists(fresh), "rank %d created a file" % g
            assert open(kept, "rb").read() == b"what was here before", "rank %d wrote over a file" % g
        grp.step(1)                                                 # and the group goes on
        assert_anchor(nb, grp, traj[7], "one step after the refusals")
    finally:
        grp.close()


def test_group_state_file(nb, tmp_path):
    """StepperGroup.save_state after step 12 of the clean run on 3 ranks, where rank 0 owns nothing: the file is the group's
    download, velocities included, and both a fresh group of 8 and a plain context go on from it to the oracle's step 15."""
    run = (1000, ol.CLEAN)
    cfg, bodies = lc.dense_bodies(nb, run[0])
    traj = sc.trajectory(*run, nb.F32, sc.STEPS + 3)
    path = str(tmp_path / "group.nbody")
    grp = nb.StepperGroup(3, cfg=cfg, semantics=run[1])
    try:
        grp.upload(bodies)
        grp.step(12)
        got = assert_anchor(nb, grp, traj[12], "step 12")
        assert grp.ranks[0].own_range() == (0, 0)
        grp.save_state(path)
        assert peek(nb, path) == (nb.F32, 201, 12) and traj[12].n == 201
        assert np.array_equal(payload(path, nb.F32), bits(got.block))
        assert got.Velocities.any(axis=1).all()
        assert_anchor(nb, grp, traj[12], "after the save")
    finally:
        grp.close()
    for loader in (nb.StepperGroup(8, cfg=cfg, semantics=run[1]), nb.Stepper(cfg, semantics=run[1])):
        try:
            loader.load_state(path)
            assert_anchor(nb, loader, traj[12], "loaded")
            loader.step(3)
            assert_anchor(nb, loader, traj[15], "3 steps after the load")
        finally:
            loader.close()
