"""The fp32 ring kernel's persistent form (rings that pull walk segments from a queue) against its one-shot
form (kernel_variant 52) and the CPU oracle: BIT-EXACT positions, velocities, masses, radii, survivor counts, pair
counters and event logs.  kernel_variant 61 / 62 force the persistent form with every walk cut into segments of 1 / 3
tiles, so that tiny systems cross every kind of segment boundary:

    N = 512   one round of turns per tile; with 1-tile segments there are as many segments as tiles
    N = 640   with 3-tile segments the last segment is a remainder (5 tiles = 3 + 2)
    N = 1000  the truncated last tile of 1000 mod 129 entries inside the last segment; frozen bodies (896 ... 999)
    N = 2053  unaligned windows after the wrap; 32 rings on 8 workgroups' slots, 16 or 6 segments each: a ring slot
              pulls many items, and a segment's predecessor ran on another slot

One reference per case (oracle and variant 52, three steps), computed once and shared."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

DT, GROWTH = np.float32(0.2), np.float32(0.1)
STEPS = 3
QUEUE_VARIANTS = [61, 62]

CASES = {
    "n512": dict(n=512),
    "n640": dict(n=640),
    "n1000": dict(n=1000),
    "n2053": dict(n=2053),
    # two coincident bodies at radii 0: the NaN-sum path redoes a turn; with 1-tile segments every turn of the walk is
    # the first or last of its wave in a segment, so the redone turn sits at a segment boundary
    "n512-coincident": dict(n=512, coincident=True),
    # stock radii in a dense field, events recorded (the kLog build): absorptions and deletions whose mnew / rnew /
    # deleted have to survive the boundaries that follow them
    "n1000-stock-events": dict(n=1000, stock=True, field=5000),
}


def _bodies(nb, case):
    c = CASES[case]
    field = c.get("field", 100000)
    kw = {} if c.get("stock") else {"minRadius": 0.0, "maxRadius": 0.0}
    cfg = nb.stock_config(particleCount=c["n"], fieldWidth=field, fieldHeight=field, **kw)
    bodies = nb.init_bodies(cfg)
    if c.get("coincident"):
        bodies.Positions[300] = bodies.Positions[17]       # across tiles, across rings
    return cfg, bodies, field


def _events(st, step):
    ev = st.events()
    ev = ev[ev["step"] == step]
    return (sorted((int(e["i"]), int(e["j"])) for e in ev[ev["kind"] == 0]),
            sorted(set(int(e["i"]) for e in ev[ev["kind"] == 1])))


def _run(nb, case, variant):
    """-> per step (survivors, state words, pair counter, absorptions, deletions)"""
    cfg, bodies, _ = _bodies(nb, case)
    out = []
    with nb.Stepper(cfg, kernel_variant=variant, record_events=True) as st:
        st.upload(bodies)
        for s in range(STEPS):
            st.step(1)
            d = st.download()
            out.append((d.numBodies, d.block.view(np.uint32).copy(), int(st.stats().pairs)) + _events(st, s))
    return out


_REFERENCE = {}


def _reference(nb, case):
    if case not in _REFERENCE:
        cfg, bodies, field = _bodies(nb, case)
        blk = bodies.contiguousData.copy()
        cur, oracle = CASES[case]["n"], []
        for _ in range(STEPS):
            cur, _, ab, de, _ = ol.port_step(blk, cur, DT, field, field, GROWTH)
            oracle.append((cur, blk[:6 * cur].view(np.uint32).copy(), sorted((int(a), int(b)) for a, b in ab),
                           sorted(int(d) for d in de)))
        _REFERENCE[case] = (oracle, _run(nb, case, 52))
    return _REFERENCE[case]


def _assert_same(got, oracle, one_shot, what):
    for s in range(STEPS):
        n, words, pairs, absorbed, deleted = got[s]
        assert n == oracle[s][0] == one_shot[s][0], (what, s, n, oracle[s][0], one_shot[s][0])
        assert np.array_equal(words, oracle[s][1]), "%s step %d: state differs from the oracle" % (what, s)
        assert np.array_equal(words, one_shot[s][1]), "%s step %d: state differs from variant 52" % (what, s)
        assert pairs == one_shot[s][2], (what, s, pairs, one_shot[s][2])
        assert absorbed == oracle[s][2] == one_shot[s][3], "%s step %d: absorptions" % (what, s)
        assert deleted == oracle[s][3] == one_shot[s][4], "%s step %d: deletions" % (what, s)


@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
@pytest.mark.parametrize("case", list(CASES))
def test_persistent_form_three_steps(nb, case, variant):
    """Three consecutive steps on one context (the item counter and the done words are never cleared by the host)."""
    oracle, one_shot = _reference(nb, case)
    if case == "n512-coincident":
        assert oracle[0][2] and oracle[0][0] < 512         # the coincident pair did collide
    if case == "n1000-stock-events":
        assert oracle[0][2] and oracle[0][3]               # absorptions and deletions in the first step
    _assert_same(_run(nb, case, variant), oracle, one_shot, "%s variant %d" % (case, variant))


@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_upload_step_upload_step(nb, variant):
    """A second upload on a context that has stepped: the queue's words carry nothing over."""
    oracle, _ = _reference(nb, "n2053")
    cfg, bodies, _ = _bodies(nb, "n2053")
    with nb.Stepper(cfg, kernel_variant=variant) as st:
        for _ in range(2):
            st.upload(bodies)
            st.step(1)
            d = st.download()
            assert d.numBodies == oracle[0][0] and np.array_equal(d.block.view(np.uint32), oracle[0][1])


@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_force_launches_back_to_back(nb, variant):
    """nbody_debug_force_only twice, no host wait in between: the second launch starts from a clean item counter and does
    not take the first launch's done words for its own; the pair counter says both walked everything, and the step
    that follows is the oracle's."""
    oracle, one_shot = _reference(nb, "n2053")
    cfg, bodies, _ = _bodies(nb, "n2053")
    with nb.Stepper(cfg, kernel_variant=variant) as st:
        st.upload(bodies)
        st.force_only(2)
        assert st.stats().pairs == 2 * one_shot[0][2]
        st.step(1)
        d = st.download()
        assert d.numBodies == oracle[0][0] and np.array_equal(d.block.view(np.uint32), oracle[0][1])
        assert st.stats().pairs == 3 * one_shot[0][2]


@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_rings_without_own_bodies(nb, variant):
    """Steps enqueued without a look at the device in between: the launches stay sized for the uploaded count while
    collisions in a dense field remove most bodies, so many rings of the later launches have no own bodies.  Their items
    are dropped where they are drawn; the rest of the queue runs as ever."""
    n, field, steps = 2053, 5000, 5
    cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field)
    bodies = nb.init_bodies(cfg)
    blk = bodies.contiguousData.copy()
    cur = n
    for _ in range(steps):
        cur, *_ = ol.port_step(blk, cur, DT, field, field, GROWTH, want_events=False)
    assert cur < n - 256                                   # at least four rings' worth of bodies are gone
    with nb.Stepper(cfg, kernel_variant=variant) as st:
        st.upload(bodies)
        st.step(steps)
        d = st.download()
        assert d.numBodies == cur and np.array_equal(d.block.view(np.uint32), blk[:6 * cur].view(np.uint32))
