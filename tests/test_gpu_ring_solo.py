"""The fp32 ring kernel's SOLO form (one wave per 64 bodies takes every turn of its walk) against the one-shot
4 x 4 ring (kernel_variant 52): BIT-EXACT positions, velocities, masses, radii, survivor counts and pair counters, and the
same event log where one is recorded.  kernel_variant 70 forces the solo form one-shot, 71 with the segment queue at the
best cut measured, 72 with the queue and one-tile items everywhere, so that small systems cross an item boundary
after every tile - the truncated last tile is then an item of its own, next to a boundary.

    N = 1, 2          fewer bodies than a tile: tile 0 is the truncated tile and holds the self position
    N = 64, 65        a lone full wave; a second ring of one body (63 lanes without one)
    N = 127 ... 130   one tile short of / exactly / just over 128: literal walks one tile (129 = N mod 129 = 0 entries!),
                      clean walks a partial second one
    N = 200, 255, 257 partial waves and tiles, the wrap of an unaligned window
    N = 1000, 4099    many tiles, frozen bodies (literal), more than one workgroup of 16 solo waves (4099: 66 rings)

One reference run per case (variant 52), computed once and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOLO_VARIANTS = [70, 71, 72]
SIZES = [1, 2, 64, 65, 127, 128, 129, 130, 200, 255, 257, 1000, 4099]
SOLO_NAME = "forces_ring_f32 (16 solo waves per workgroup)"
SOLO_QUEUE_NAME = "forces_ring_f32 (16 solo waves per workgroup, persistent)"
RING_QUEUE_NAME = "forces_ring_f32 (4 rings x 4 waves per workgroup, persistent)"


def _plain(nb, n, field=100000, stock=False):
    kw = {} if stock else {"minRadius": 0.0, "maxRadius": 0.0}
    cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field, **kw)
    return cfg, nb.init_bodies(cfg)


def _coincident(nb):
    """as test_coincident_bodies_at_zero_radii sets them up"""
    cfg, bodies = _plain(nb, 4096)
    P, M = bodies.Positions, bodies.Masses
    P[70] = P[5]                      # same tile, same wave
    P[200] = P[130]                   # same tile, other half
    P[1000] = P[300]                  # across tiles
    P[4090] = P[3]                    # across the wrap (last tile / tile 0)
    P[2000] = P[2001] = P[2002]       # three on one point
    P[2500] = P[2600]
    M[2500] = M[2600]                 # equal masses: both absorb, neither is deleted
    P[129] = P[128]                   # the twin sits at walk position 1 of its partner, right after the self position
    return cfg, bodies


def _non_finite_mass(nb):
    """Meta::summary bit 3: the launch runs the v_min3 screen although every radius is +0"""
    cfg, bodies = _plain(nb, 2048)
    bodies.Masses[700] = np.nan
    bodies.Masses[1500] = np.inf
    bodies.Masses[1501] = -np.inf
    bodies.Positions[900] = bodies.Positions[40]
    return cfg, bodies


def _events(st):
    ev = st.events()
    return sorted((int(e["step"]), int(e["kind"]), int(e["i"]), int(e["j"])) for e in ev)


def _run(nb, cfg, bodies, variant, steps, semantics=0, events=False, look=True):
    """-> per step (survivors, state words, pair counter) and the event log; look=False: all steps enqueued at once"""
    out = []
    with nb.Stepper(cfg, kernel_variant=variant, semantics=semantics, record_events=events) as st:
        st.upload(bodies)
        for _ in range(steps if look else 1):
            st.step(1 if look else steps)
            d = st.download()
            out.append((d.numBodies, d.block.view(np.uint32).copy(), int(st.stats().pairs)))
        return out, (_events(st) if events else None), st.force_kernel_name()


def _assert_same(got, ref, what):
    (g_steps, g_events, _), (r_steps, r_events, _) = got, ref
    for s, (g, r) in enumerate(zip(g_steps, r_steps)):
        assert g[0] == r[0], "%s step %d: %d bodies, variant 52 has %d" % (what, s, g[0], r[0])
        assert np.array_equal(g[1], r[1]), "%s step %d: state differs from variant 52" % (what, s)
        assert g[2] == r[2], "%s step %d: %d pairs, variant 52 counted %d" % (what, s, g[2], r[2])
    assert g_events == r_events, "%s: event log differs from variant 52" % what


_REFERENCE = {}


def _reference(nb, key, make, **kw):
    if key not in _REFERENCE:
        cfg, bodies = make()
        _REFERENCE[key] = _run(nb, cfg, bodies, 52, **kw)
    return _REFERENCE[key]


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_radii_three_steps(nb, n, semantics):
    make = lambda: _plain(nb, n)
    kw = dict(steps=3, semantics=semantics)
    ref = _reference(nb, ("plain", n, semantics), make, **kw)
    for variant in SOLO_VARIANTS:
        got = _run(nb, *make(), variant, **kw)
        assert got[2] == (SOLO_NAME if variant == 70 else SOLO_QUEUE_NAME)
        _assert_same(got, ref, "N %d variant %d" % (n, variant))


@pytest.mark.parametrize("n", [1000, 4099])
def test_stock_radii_five_steps_with_events(nb, n):
    """Flagged lanes, absorptions and deletions in walk order; the event log is variant 52's."""
    make = lambda: _plain(nb, n, field=5000, stock=True)
    kw = dict(steps=5, events=True)
    ref = _reference(nb, ("stock", n), make, **kw)
    assert any(e[1] == 0 for e in ref[1]) and any(e[1] == 1 for e in ref[1])      # absorptions and deletions happened
    assert ref[0][-1][0] < n
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "N %d variant %d" % (n, variant))


@pytest.mark.parametrize("case", ["coincident", "non-finite-mass"])
def test_screens(nb, case):
    """coincident: radii 0, the NaN-sum screen sends the lanes of coincident bodies down the exact path.
    non-finite-mass: summary bit 3 forces the v_min3 screen per pair."""
    make = (lambda: _coincident(nb)) if case == "coincident" else (lambda: _non_finite_mass(nb))
    kw = dict(steps=3)
    ref = _reference(nb, case, make, **kw)
    if case == "coincident":
        assert ref[0][0][0] <= 4096 - 6                    # the coincident bodies did collide
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "%s variant %d" % (case, variant))


def test_launch_sized_for_more_bodies_than_exist(nb):
    """Five steps enqueued without a look at the device in between: the launches stay sized for the uploaded count while
    collisions in a dense field remove bodies, so waves of the later launches have no own bodies and drop their items."""
    make = lambda: _plain(nb, 2053, field=5000, stock=True)
    kw = dict(steps=5, look=False)
    ref = _reference(nb, "shrinking", make, **kw)
    assert ref[0][0][0] < 2053 - 256                       # at least four rings' worth of bodies are gone
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "variant %d" % variant)


@pytest.mark.parametrize("variant", SOLO_VARIANTS)
def test_force_launches_back_to_back(nb, variant):
    """Two force launches with no host wait in between: the second starts from a clean item counter and does not take the
    first launch's done words for its own; both walk everything, and the step that follows is variant 52's."""
    make = lambda: _plain(nb, 2053)
    ref = _reference(nb, "back-to-back", make, steps=1)
    cfg, bodies = make()
    with nb.Stepper(cfg, kernel_variant=variant) as st:
        st.upload(bodies)
        st.force_only(2)
        assert st.stats().pairs == 2 * ref[0][0][2]
        st.step(1)
        d = st.download()
        assert d.numBodies == ref[0][0][0] and np.array_equal(d.block.view(np.uint32), ref[0][0][1])
        assert st.stats().pairs == 3 * ref[0][0][2]


def test_default_selection_at_the_flagship_shape(nb):
    """The solo form is selected where the own range is exactly one wave per wave slot of the device (16 per CU) and the event
    log is off.  Checked through the kernel name only: N = 262144 on a device of 256 CUs, and half of that, where the
    persistent 4 x 4 ring stays."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    names = {}
    for n, events in [(262144, False), (262144, True), (131072, False)]:
        cfg, bodies = _plain(nb, n)
        with nb.Stepper(cfg, record_events=events) as st:
            st.upload(bodies)
            names[n, events] = st.force_kernel_name()
    assert names[262144, False] == (SOLO_QUEUE_NAME if 262144 // 64 == 16 * cus else RING_QUEUE_NAME), (cus, names)
    assert names[262144, True] == RING_QUEUE_NAME and names[131072, False] == RING_QUEUE_NAME, (cus, names)
