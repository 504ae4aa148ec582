"""GPU tests of the per-step screen bookkeeping (run with -m gpu on an MI355X).

The fp32 ring kernel trusts Meta::summary and tile_rmax, which describe the whole replica and are rebuilt on the device
every step (compact_count clears, unpack_slots refills), written by nbody_upload on the host, and by ref_layout_pack_f32
for the reference-shaped launches.  Here they are compared - through nbody_debug_screen_state, on every rank, after every
upload and every step - with their numpy statement (tests/regime_cases.py: equality, not superset), on runs whose regime
CHANGES while they run, on one context that is given several different states, and on reference-shaped launches fed edge
states through one process-wide workspace.  The state itself is compared with the CPU oracle bit for bit (tolerance
zero; NaNs compare equal to NaNs: payloads differ between x86 and gfx950).  tests/test_regime_cases_cpu.py proves on the
CPU that every case reaches the regimes it declares."""
import numpy as np
import pytest

import oracle_lib as ol
import regime_cases as rc

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def nan_aware_equal(got, want):
    g, w = np.asarray(got), np.asarray(want)
    both_nan = np.isnan(g) & np.isnan(w)
    return g.shape == w.shape and np.array_equal(bits(g)[~both_nan.ravel()], bits(w)[~both_nan.ravel()])


def ranks_of(ctx):
    return getattr(ctx, "ranks", None) or [ctx]


def events_of(ctx):
    return np.concatenate([r.events() for r in ranks_of(ctx)])


def assert_events(ev, step, ab, de, what):
    ev = ev[ev["step"] == step]
    assert sorted((int(e["i"]), int(e["j"])) for e in ev[ev["kind"] == 0]) == sorted((int(a), int(b)) for a, b in ab), \
        "%s: E_t" % what
    assert sorted(set(int(e["i"]) for e in ev[ev["kind"] == 1])) == sorted(int(d) for d in de), "%s: D_t" % what


def make_ctx(nb, kind, **kw):
    """kind: 1, 2, 3 = StepperGroup of that many ranks; "rccl" = one rank with a communicator (slot all-gather through RCCL)."""
    if kind == "rccl":
        return nb.Stepper(comm_id=nb.comm_unique_id(), force_comm=True, **kw)
    return nb.StepperGroup(kind, **kw)


def case_ctx(nb, case, kind, **kw):
    return make_ctx(nb, kind, capacity=case["n"], precision=case["precision"], semantics=case["semantics"],
                    timestep=float(case["dt"]), growthRate=float(case["growth"]), fieldWidth=case["field"],
                    fieldHeight=case["field"], **kw)


# ---------------------------------------------------------------------------------------------------------
# C. regime changes during a run
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trajectory():
    memo = {}

    def get(case):
        if case["name"] not in memo:
            memo[case["name"]] = rc.oracle_trajectory(case, want_events=True)
        return memo[case["name"]]
    return get


def run_case(nb, case, kind, variant, trajectory):
    ctx = case_ctx(nb, case, kind, kernel_variant=variant, record_events=True)
    what = "%s variant %d ranks %s" % (case["name"], variant, kind)
    try:
        ctx.upload(case["bodies"])
        rc.assert_screen_state(ctx, case["bodies"], what + " upload")
        assert ranks_of(ctx)[0].screen_state()[0] == case["summary0"], what
        for s, (n, blk, ab, de) in enumerate(trajectory(case)):
            ctx.step(1)
            out = ctx.download()
            w = "%s step %d" % (what, s + 1)
            assert out.numBodies == n, (w, out.numBodies, n)
            assert nan_aware_equal(out.block, blk), w
            assert_events(events_of(ctx), s, ab, de, w)
            rc.assert_screen_state(ctx, out, w)
            for r in ranks_of(ctx):                          # the sequence the CPU file proved for the oracle
                assert r.screen_state()[0] == case["summaries"][s], (w, r.screen_state()[0], case["summaries"][s])
    finally:
        ctx.close()


F32_CASES, F64_CASES = rc.mid_run_cases_f32(), rc.mid_run_cases_f64()
_ids = lambda cases: [c["name"] for c in cases]


@pytest.mark.parametrize("variant", [0, 50, 52, 54, 31, 1])
@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_regime_changes_mid_run(nb, case, variant, trajectory):
    """Cases a-d on one rank with the automatic choice, the three ring shapes, the one-lane and the general kernel."""
    run_case(nb, case, 1, variant, trajectory)


@pytest.mark.parametrize("kind", [2, 3, "rccl"])
@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_regime_changes_mid_run_partitioned(nb, case, kind, trajectory):
    """The same on 2 and 3 ranks (every rank rebuilds the bookkeeping of the WHOLE replica from all slots; a wave of
    unpack_slots then starts at a slot offset that is no multiple of 64) and on the single-rank RCCL context."""
    run_case(nb, case, kind, 0, trajectory)


@pytest.mark.parametrize("kind,variant", [(1, 0), (1, 1), (2, 0), (3, 0)])
@pytest.mark.parametrize("case", F64_CASES, ids=_ids(F64_CASES))
def test_regime_changes_mid_run_fp64(nb, case, kind, variant, trajectory):
    """Cases b and d against the fp64 oracle: summary bits 0 and 1, coordinate bound 2^249."""
    run_case(nb, case, kind, variant, trajectory)


# ---------------------------------------------------------------------------------------------------------
# C'. planted states: one value at one index, at the edges of every per-body rule (tests/regime_cases.py)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [rc.F32, rc.F64], ids=["f32", "f64"])
def test_planted_states_at_upload_and_after_a_step(nb, precision):
    """nbody_upload's rule (the host's nbody_block_pack) and unpack_slots' rule against the numpy statement, for every
    planted state, in ONE context per precision that is given one state after the other.  Time step 0, so that a planted
    value survives the step wherever the arithmetic lets it (x + 0 * v; a NaN or infinite value spreads, a radius in reach
    of another body deletes): the state after the step is the oracle's, bit for bit, and the bookkeeping is compared with
    the numpy statement of THAT state."""
    field = 100000
    real = float if precision == rc.F64 else np.float32
    ctx = nb.StepperGroup(1, capacity=rc.PLANT_N, precision=precision, timestep=0.0, growthRate=0.1, fieldWidth=field,
                          fieldHeight=field)
    kept = 0
    try:
        for s in rc.planted_states(precision):
            b = s["bodies"]
            ctx.upload(b)
            rc.assert_screen_state(ctx, b, s["name"] + " upload")
            assert ranks_of(ctx)[0].screen_state()[0] == s["summary"], s["name"]
            ctx.step(1)
            out = ctx.download()
            blk = b.block.copy()
            n, *_ = ol.port_step(blk, rc.PLANT_N, real(0.0), field, field, real(0.1), want_events=False)
            assert out.numBodies == n and nan_aware_equal(out.block, blk[:6 * n]), s["name"] + " step 1: != oracle"
            rc.assert_screen_state(ctx, out, s["name"] + " step 1")
            kept += int(n == rc.PLANT_N and nan_aware_equal(out.Positions.ravel(), b.Positions.ravel()) and
                        nan_aware_equal(out.Radii, b.Radii) and nan_aware_equal(out.Masses, b.Masses))
    finally:
        ctx.close()
    assert kept >= len(rc.planted_states(precision)) // 2, kept   # most planted values do survive a step of length 0


def test_wave_of_unpack_slots_straddles_two_tiles(nb, trajectory):
    """Two ranks, n = 300: after step 1 rank 1's slot is unpacked at offset 127, and the two planted radii lie on the two
    sides of the tile edge inside its first wave (tests/test_regime_cases_cpu.py proves both with the oracle)."""
    case = rc.case_wave_straddles_a_tile()
    run_case(nb, case, 2, 0, trajectory)
    ctx = case_ctx(nb, case, 2)
    try:
        ctx.upload(case["bodies"])
        ctx.step(1)
        for r in ranks_of(ctx):
            assert r.screen_state()[1][:3].tolist() == [0.25, 0.5, 0.0]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------
# D. one context, several different states
# ---------------------------------------------------------------------------------------------------------
DT, GROWTH = np.float32(0.2), np.float32(0.1)
LAG = 4                                                      # nbody_ctx::kLag


@pytest.mark.parametrize("kind", [1, 2, 3, "rccl"])
def test_one_context_several_states(nb, kind, tmp_path):
    """S1 (n = 8000, dense, stock radii, an out-of-range coordinate and a NaN radius; the count collapses), then WITHOUT
    closing S2 (n = 1500, radii 0, calm: summary 0 and every tile_rmax entry 0 although S1 left non-zero ones, stale
    records past the new n), S3 (n = 8192: larger than the live bound S1's exchange had shrunk to), then a state file
    saved mid-run by another context.  After every upload / load and every step the reused context equals a fresh context
    given the same state and the oracle; its bookkeeping, counters, exchange layout and event log restart with the upload."""
    field, cap = rc.REUSE_FIELD, rc.REUSE_CAPACITY
    kw = dict(capacity=cap, timestep=float(DT), growthRate=float(GROWTH), fieldWidth=field, fieldHeight=field,
              record_events=True)
    world = 1 if kind == "rccl" else kind
    exchanges = kind != 1
    # a file saved mid-run by a different context
    donor_cfg = nb.stock_config(particleCount=4096, fieldWidth=field, fieldHeight=field)
    donor = nb.Stepper(donor_cfg)
    donor.upload(nb.init_bodies(donor_cfg))
    donor.step(4)
    path = str(tmp_path / "mid_run.nbody")
    donor.save_state(path)
    loaded = donor.download()
    donor.close()
    assert 0 < loaded.numBodies < 4096

    def stride(n):
        return rc.exchange_stride(n, world)

    def download_bytes(n):                                   # a download of an exchanging context gathers velocities and Meta
        return world * (((n + 127) // 128 + world - 1) // world * 128 * 8 + 32)

    ctx = make_ctx(nb, kind, **kw)
    watched = ranks_of(ctx)[-1]                              # group: a rank other than 0 (rank 0 also receives the downloads)
    states = [(name, b, steps, 0) for name, b, steps in rc.reuse_states()] + [("loaded", loaded, 3, 4)]
    left = None                                              # bodies the previous state ended with
    try:
        for name, bodies, steps, step0 in states:
            if name in ("S2", "loaded"):                     # tiles past the new end were in use a moment ago
                assert bodies.numBodies + 128 < left, (name, bodies.numBodies, left)
            fresh = make_ctx(nb, kind, **kw)
            if name == "loaded":
                for c in ranks_of(ctx) + ranks_of(fresh):
                    c.load_state(path)
            else:
                ctx.upload(bodies)
                fresh.upload(bodies)
            n0 = bodies.numBodies
            rc.assert_screen_state(ctx, bodies, name + " upload")
            st = watched.stats()
            assert (st.steps, st.pairs, st.n_bodies, st.exchange_bytes) == (step0, 0, n0, 0), name
            assert st.slot_bytes_now == (stride(n0) if exchanges else 0), name
            assert len(events_of(ctx)) == 0, name            # the log restarts with the upload
            got = ctx.download()
            assert got.numBodies == n0 and nan_aware_equal(got.block, bodies.block), name
            dl = download_bytes(n0) if kind == "rccl" else 0
            blk, cur, counts, pairs, expect = bodies.block.copy(), n0, [], 0, 0
            for s in range(steps):
                w = "%s step %d (ranks %s)" % (name, s + 1, kind)
                ctx.step(1)
                fresh.step(1)
                pairs += ol.port().oracle_pairs_per_step(cur, ol.LITERAL)
                expect += world * stride(n0 if s < LAG else counts[s - LAG])
                cur, _, ab, de, _ = ol.port_step(blk, cur, DT, field, field, GROWTH)
                counts.append(cur)
                st = watched.stats()
                assert st.steps == step0 + s + 1 and st.n_bodies == cur, w
                assert sum(r.stats().pairs for r in ranks_of(ctx)) == pairs, w
                assert st.exchange_bytes == (expect + dl if exchanges else 0), (w, st.exchange_bytes, expect, dl)
                assert st.slot_bytes_now == (stride(n0 if s < LAG else counts[s - LAG]) if exchanges else 0), w
                out, ref = ctx.download(), fresh.download()
                dl += download_bytes(cur) if kind == "rccl" else 0
                assert out.numBodies == ref.numBodies == cur, w
                assert np.array_equal(bits(out.block), bits(ref.block)), w + ": reused context != fresh context"
                assert nan_aware_equal(out.block, blk[:6 * cur]), w + ": != oracle"
                rc.assert_screen_state(ctx, out, w)
                ev = events_of(ctx)
                assert set(ev["step"].tolist()) <= set(range(step0, step0 + s + 1)), w   # of the current upload only
                assert_events(ev, step0 + s, ab, de, w)
            if name == "S1":
                assert counts[-1] < n0 - 512                 # the exchange's live bound did shrink before the next uploads
            if name == "S3" and exchanges:                   # laid out for 8192 again, not for what S1 had shrunk to
                assert expect == world * (4 * stride(8192) + stride(counts[0]) + stride(counts[1])) and \
                    stride(8192) > stride(counts[0]), (expect, counts)
            left = cur
            fresh.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------
# E. reference-shaped launches on edge states
# ---------------------------------------------------------------------------------------------------------
def edge_states():
    """[(name, block, n, dt, growth, field)]: the step-0 states of the cases above and of the edge tests of
    tests/test_gpu_parity.py, between two visits of a large calm state."""
    import ppa_nbody_collisions_amd as nb
    big = nb.init_bodies(nb.stock_config(particleCount=20000, minRadius=0.0, maxRadius=0.0))
    out = [("calm n=20000", big.block, 20000, DT, GROWTH, 100000)]
    for c in F32_CASES:
        out.append((c["name"], c["bodies"].block, c["n"], c["dt"], c["growth"], c["field"]))
    for c in rc.planted_states(rc.F32):                       # n = 257: two whole blocks and a body that gets no thread
        out.append(("planted " + c["name"], c["bodies"].block, rc.PLANT_N, DT, GROWTH, 100000))
    _, rb, field = rc.radius_bounds_bodies(3000)
    out.append(("radius bounds n=3000", rb.block, 3000, DT, GROWTH, field))
    out.append(("coincident bodies", rc.coincident_bodies(4096).block, 4096, DT, GROWTH, 100000))
    out.append(("coincident bodies, one small coordinate", rc.coincident_bodies(4096, True).block, 4096, DT, GROWTH, 100000))
    out.append(("extreme values", rc.extreme_bodies(2048).block, 2048, DT, GROWTH, 100000))
    out.append(("calm n=20000 again", big.block, 20000, DT, GROWTH, 100000))
    return out


def _launch_step(nb, torch, dev, n, dt, growth, field):
    upd_m = dev[4 * n:5 * n].clone()                         # src/nbody.cu:467-470
    upd_r = dev[5 * n:6 * n].clone()
    blocks = nb.lib.nbody_num_blocks(n)
    stream = torch.cuda.current_stream().cuda_stream
    assert nb.lib.nbody_launch_compute_forces_f32(dev.data_ptr(), upd_m.data_ptr(), upd_r.data_ptr(), n, float(dt), field,
                                                  field, blocks, float(growth), stream) == 0, nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_launch_move_bodies_f32(dev.data_ptr(), upd_m.data_ptr(), upd_r.data_ptr(), n, float(dt), blocks,
                                               stream) == 0, nb.lib.nbody_last_error_string()
    torch.cuda.synchronize()
    return dev.cpu().numpy()


@pytest.mark.parametrize("path", [0, 1, 2], ids=["production-kernel", "general-kernel", "one-lane-kernel"])
def test_reference_shaped_launches_on_edge_states(nb, path, monkeypatch):
    """nbody_launch_compute_forces_f32 / nbody_launch_move_bodies_f32 in ONE process, in this order: a large calm state,
    then smaller states in other regimes (negative, NaN, infinite and giant radii, coincident pairs at radius 0,
    out-of-range, tiny and NaN coordinates, masses at the bound), then the large one again - through one process-wide
    workspace whose Meta and radius bounds ref_layout_pack_f32 rebuilds per launch.  Three steps each with the host
    compaction in between; the block after move_bodies against the oracle's PRE-compaction block, bit for bit."""
    import torch
    monkeypatch.setenv("NBODY_REF_LAUNCH_GENERAL", "1" if path == 1 else "0")
    monkeypatch.setenv("NBODY_REF_LAUNCH_ONE_LANE", "1" if path == 2 else "0")
    assert nb.lib.nbody_launch_workspace_release() == 0
    for name, block, n, dt, growth, field in edge_states():
        host = np.array(block[:6 * n], dtype=np.float32)
        want = host.copy()
        for s in range(3):
            dev = torch.from_numpy(host[:6 * n].copy()).cuda()
            blk = _launch_step(nb, torch, dev, n, dt, growth, field)
            n_want, _, _, _, pre = ol.port_step(want, n, np.float32(dt), field, field, np.float32(growth), want_events=False,
                                                pre=True)
            assert nan_aware_equal(blk, pre), "%s step %d" % (name, s + 1)
            n_new = nb.lib.nbody_block_compact(blk.ctypes.data, n, nb.F32)     # src/nbody.cu:488-510
            assert n_new == n_want, (name, s, n_new, n_want)
            assert nan_aware_equal(blk[:6 * n_new], want[:6 * n_new]), "%s step %d, compacted" % (name, s + 1)
            host, n = blk, n_new
    # the workspace is released and comes back with the next launch
    assert nb.lib.nbody_launch_workspace_release() == 0
    name, block, n, dt, growth, field = edge_states()[-3]
    dev = torch.from_numpy(np.array(block[:6 * n], dtype=np.float32)).cuda()
    blk = _launch_step(nb, torch, dev, n, dt, growth, field)
    want = np.array(block[:6 * n], dtype=np.float32)
    pre = ol.port_step(want, n, np.float32(dt), field, field, np.float32(growth), want_events=False, pre=True)[4]
    assert nan_aware_equal(blk, pre), name + " after the release"
    assert nb.lib.nbody_launch_workspace_release() == 0
