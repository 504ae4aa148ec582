"""The solo ring kernel's trimmed turn (profiles/ring_solo_trim.txt) against the one-shot 4 x 4 ring
(kernel_variant 52): BIT-EXACT positions, velocities, masses, radii, survivor counts and pair counters, with the event log
off (the builds that carry the trims).  70 = solo one-shot, 71 = solo with the segment queue, 72 = 71 with one-tile items.

What each case pins:
    sizes            the window's entry offsets per quarter of a tile (4 l + 128 h bytes in the scalar base, the wrapped
                     offset for h = 3), aligned and unaligned windows, truncated tiles next to item boundaries; 129, 258, 387
                     and 516 are multiples of 129, where the literal last tile has N mod 129 = 0 entries
    coincident pair  the NaN look after the chain and the redo from the sums kept in registers, with the NaN term in every
                     quarter of a tile, at a turn's first and last position
    stock radii      flagged lanes, absorptions and deletions in walk order; the radius bound carried as a scalar
    shrinking        waves without own bodies never take a turn, so their tile count stays 0: the priority rule must not
                     wait for them nor change a bit
    pair counts      one flush per slot for all its items (variant 72: many items per slot)

One reference run per case (variant 52), computed once and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOLO_VARIANTS = [70, 71, 72]
SIZES = [31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130, 191, 193, 256, 257, 258, 383, 385, 387, 516, 1000, 4099]
# walk position of the coincident partner in the tile: first and last position of the turn of each quarter (position 0 of
# the first quarter is the body itself in the literal walk, so position 1 stands in for it there)
PLACEMENTS = [(0, "first"), (0, "last"), (1, "first"), (1, "last"), (2, "first"), (2, "last"), (3, "first"), (3, "last")]


def _plain(nb, n, field=100000, stock=False):
    kw = {} if stock else {"minRadius": 0.0, "maxRadius": 0.0}
    cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field, **kw)
    return cfg, nb.init_bodies(cfg)


def _run(nb, cfg, bodies, variant, steps, semantics=0, look=True):
    """-> per step (survivors, state words, pair counter); look=False: all steps enqueued at once"""
    out = []
    with nb.Stepper(cfg, kernel_variant=variant, semantics=semantics) as st:
        st.upload(bodies)
        for _ in range(steps if look else 1):
            st.step(1 if look else steps)
            d = st.download()
            out.append((d.numBodies, d.block.view(np.uint32).copy(), int(st.stats().pairs)))
    return out


def _assert_same(got, ref, what):
    assert len(got) == len(ref)
    for s, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0], "%s step %d: %d bodies, variant 52 has %d" % (what, s, g[0], r[0])
        assert np.array_equal(g[1], r[1]), "%s step %d: state differs from variant 52" % (what, s)
        assert g[2] == r[2], "%s step %d: %d pairs, variant 52 counted %d" % (what, s, g[2], r[2])


_REFERENCE = {}


def _reference(nb, key, make, **kw):
    if key not in _REFERENCE:
        cfg, bodies = make()
        _REFERENCE[key] = _run(nb, cfg, bodies, 52, **kw)
    return _REFERENCE[key]


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
@pytest.mark.parametrize("n", SIZES)
def test_quarter_and_tile_edges(nb, n, semantics):
    make = lambda: _plain(nb, n)
    kw = dict(steps=3, semantics=semantics)
    ref = _reference(nb, ("plain", n, semantics), make, **kw)
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "N %d variant %d" % (n, variant))


def _coincident_pair(nb, semantics, quarter, where):
    """N = 300, radii 0, one coincident pair.  Literal: body 5 meets body (5 + p) mod 128 at walk position p of its first
    tile (entry (t + p) mod 128 of its own block; the partner meets body 5 at position 128 - p).  Clean: body 200 of the second tile meets body p at walk position p of
    tile 0 (its own tile is not a fast one)."""
    cfg, bodies = _plain(nb, 300)
    p = quarter * 32 + (31 if where == "last" else 0)
    if semantics == 0:
        p = max(p, 1)
        bodies.Positions[(5 + p) % 128] = bodies.Positions[5]
    else:
        bodies.Positions[p] = bodies.Positions[200]
    return cfg, bodies


@pytest.mark.parametrize("semantics", [0, 1], ids=["literal", "clean"])
@pytest.mark.parametrize("quarter,where", PLACEMENTS)
def test_coincident_pair_in_each_quarter(nb, quarter, where, semantics):
    make = lambda: _coincident_pair(nb, semantics, quarter, where)
    kw = dict(steps=3, semantics=semantics)
    ref = _reference(nb, ("pair", quarter, where, semantics), make, **kw)
    assert ref[0][0] < 300                                  # the pair did collide
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "quarter %d %s variant %d" % (quarter, where, variant))


@pytest.mark.parametrize("n", [1000, 4099])
def test_stock_radii_five_steps(nb, n):
    make = lambda: _plain(nb, n, field=5000, stock=True)
    kw = dict(steps=5)
    ref = _reference(nb, ("stock", n), make, **kw)
    assert ref[-1][0] < n                                   # bodies were absorbed
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "N %d variant %d" % (n, variant))


def test_launch_sized_for_more_bodies_than_exist(nb):
    """Six steps enqueued without a look at the device in between, in a field dense enough to lose bodies quickly: the
    launches stay sized for the uploaded count, so waves of the later launches have no own bodies, drop their items and
    never count a tile."""
    make = lambda: _plain(nb, 2053, field=2500, stock=True)
    kw = dict(steps=6, look=False)
    ref = _reference(nb, "shrinking", make, **kw)
    assert ref[0][0] < 2053 - 256                           # at least four rings' worth of bodies are gone
    for variant in SOLO_VARIANTS:
        _assert_same(_run(nb, *make(), variant, **kw), ref, "variant %d" % variant)


def test_pair_counts_across_items_and_launches(nb):
    """Variant 72 at N = 4099: one-tile items, so every slot adds up many items before its one flush.  Two force launches
    back to back, then a step: the totals are variant 52's."""
    make = lambda: _plain(nb, 4099)
    ref = _reference(nb, "pairs", make, steps=1)
    per_launch = ref[0][2]
    assert per_launch > 0
    cfg, bodies = make()
    with nb.Stepper(cfg, kernel_variant=72) as st:
        st.upload(bodies)
        st.force_only(2)
        assert st.stats().pairs == 2 * per_launch
        st.step(1)
        d = st.download()
        assert d.numBodies == ref[0][0] and np.array_equal(d.block.view(np.uint32), ref[0][1])
        assert st.stats().pairs == 3 * per_launch
