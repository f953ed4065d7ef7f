"""The line-of-sight pass (k_los_blocks, k_los, k_los_pairs) at its region, group, trip, tile, list
and slab edges, on at most 1546 rows and (but for two cases) 1025 spectra.

Every case goes through ctx.los_accumulate with host columns and is compared with
oracle.np_oracle.los_iteration, the KD-tree restatement of the reference, on the same samples,
spectra, ladders and g-value tables: npackets, `included`, n_used and the set of (spectrum, row)
pairs exactly, radiance to rtol 1e-10; two device routes of one input agree exactly and to 1e-12.

The inputs are constructed so that ONE lost, doubled or misplaced block shows
(tests/los_edge_cases.py): the samples fill a small ball beside the planet, "hot" lines of sight
look at it -- half of them with the whole ball inside their cone, so every row of a case is in a
used pair of the reference, the other half with a part of it, so the exact cone test still
decides -- and "cold" ones look away and collect nothing.  All rows have different `frac`.  These
conditions on the inputs are asserted on the ORACLE's output in case(), for every case.

What only the device knows -- the slot a block takes in the stream -- is observed through the
sphere-test counter with culling switched off (test_culling_off), which must equal a function of
the restated layout (tests/los_blocks_restatement.py)."""
import functools

import numpy as np
import pandas as pd
import pytest

from oracle import np_oracle as O
from tests import los_blocks_restatement as LB
from tests import los_edge_cases as LC
from tests import tile_plan_restatement as TP

pytestmark = pytest.mark.gpu

D_LINES = (5891, 5897)
FOUR_LINES = (3303, 5891, 5897, 5891)     # 53 KB of g-value tables: k_los keeps a smaller tile of spectra
LDS_HEADER = 4224                         # NXC_HEADER_BYTES (nxc_device.hpp)
LOS_WAVE_BYTES = 128*12 + 64*32 + 16*32 + 8*32 + 512*2 + 256*2       # NXC_LOS_WAVE_BYTES
# hot spectra on both sides of every tile edge k_los can have (tile_cap = 512 halved down to 32)
# and of the rounds of 64 spectra, the first and the last spectrum among them
TILE_EDGES = (0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)


def stage_bytes(lines):
    return LDS_HEADER + sum(TP.lut_bytes(len(v)) for v, _ in LC.g_tables(lines))


def tile_cap(lines):
    """los_run (nxc_api.hip): the spectra of a tile of k_los, from its own expression."""
    rest = ((stage_bytes(lines) + 31) & ~31) + 16*LOS_WAVE_BYTES + 32
    cap = 512
    while cap > 32 and rest + cap*7*8 > 160*1024:
        cap >>= 1
    return cap


def lds_sums(lines, n_ladder, S):
    """los_run: does k_los_pairs keep its per-spectrum sums in LDS?"""
    return ((stage_bytes(lines) + 31) & ~31) + ((n_ladder + 3) & ~3)*8 + S*16 <= 80*1024


@functools.lru_cache(maxsize=None)
def case(layout, rows=None, S=6, hot=(0, 2, 3, 5), lines=D_LINES, use_index=True, f32=False,
         scaled=None, seed=0):
    """The inputs of a case and the reference's answer, made once and shared (read-only).
    layout, rows: LC.layout_ids; S, hot: LC.lines_of_sight; use_index = False: no index column
    (one packet, `included` by row); f32: float32 columns (the reference gets them widened);
    scaled: the boresight that is multiplied by 1 + 1e-8."""
    from nexoclom_amd.LOSResult import POSITION, BORESIGHT, arccos_threshold, los_geometry
    ids = LC.layout_ids(layout, rows)
    P = len(ids)
    if not use_index:
        assert len(LC.LAYOUTS[layout]) == 1
    smp = LC.cloud(ids, seed)
    dtype = np.float32 if f32 else np.float64
    cols = [np.ascontiguousarray(smp[k].astype(dtype)) for k in ('x', 'y', 'z', 'vy', 'frac')]
    assert len(np.unique(cols[4])) == P                        # all `frac` different
    pos, look = LC.lines_of_sight(S, hot, seed)
    if scaled is not None:
        look[scaled] *= 1 + 1e-8
        b2 = np.sum(look[scaled]**2)
        assert abs(b2 - 1) > 1e-9 and abs(b2 - 1) < 1e-7       # beyond los_run's bound for culling
    spectra = pd.DataFrame(dict(zip(POSITION + BORESIGHT, list(pos.T) + list(look.T))))
    f = LC.forces()
    gt = LC.g_tables(lines)
    dphi = LC.DPHI
    cut, lengths, ladder = los_geometry(spectra, LC.OUTEREDGE, dphi)
    sc = np.vstack([pos.T, look.T, cut, lengths.astype(float)])
    setup = (dphi, np.sin(dphi), np.sin(2*dphi), arccos_threshold(dphi), f.vrplanet, f.R_km*1e5,
             gt, ladder, sc)
    n_index = int(ids.max()) + 1 if use_index else P
    wide = dict(zip(('x', 'y', 'z', 'vy', 'frac'), (c.astype(np.float64) for c in cols)))
    wide['Index'] = ids if use_index else np.arange(P)
    scd = {c: spectra[c].values for c in spectra.columns}
    r, n, inc, used = O.los_iteration(wide, scd, dphi, LC.OUTEREDGE, f.vrplanet, gt, f.R_km*1e5,
                                      n_index=n_index)
    pairs = {(i, int(row)) for i, rows_ in enumerate(used) for row in rows_}
    # the conditions on the inputs, on the reference's answer: every row is in a used pair, so a
    # block that is lost shows; hot spectra collect, cold ones do not
    assert {row for _, row in pairs} == set(range(P))
    cold = np.setdiff1d(np.arange(S), hot)
    assert (n[cold] == 0).all() and (r[cold] == 0).all() and inc.all()
    assert (n[list(hot)[0::2]] == P).all() and (r[list(hot)[0::2]] > 0).all()
    # (the hot spectra that see a part of the ball leave the exact cone test something to decide)
    part = n[list(hot)[1::2]]
    assert P < 200 or ((0 < part) & (part < P)).all()        # (a few rows may all lie on one side)
    for a in cols + [r, n, inc, ids, sc]:
        a.setflags(write=False)
    return dict(P=P, S=S, setup=setup, cols=cols, index=ids if use_index else None, n_index=n_index,
                radiance=r, npackets=n, included=inc, pairs=pairs, m=len(pairs), lines=lines,
                n_ladder=len(ladder))


def run(ctx, c, used_cap=None):
    return ctx.los_accumulate(*c['setup'], *c['cols'], index=c['index'], n_index=c['n_index'],
                              used_cap=c['m'] + 64 if used_cap is None else used_cap)


def pair_list(res):
    got = list(zip(res['used'][0].tolist(), res['used'][1].tolist()))
    assert len(got) == len(set(got))                           # no pair twice
    return set(got)


def check(res, c):
    """A device result against the reference's: the project's own figures for this pass."""
    assert np.array_equal(res['npackets'], c['npackets'])
    assert np.array_equal(res['included'], c['included'])
    assert res['n_used'] == c['m'] == res['used'].shape[1]
    assert pair_list(res) == c['pairs']
    np.testing.assert_allclose(res['radiance'], c['radiance'], rtol=1e-10, atol=0)


def same(res, other):
    """Two device routes of one input."""
    assert np.array_equal(res['npackets'], other['npackets'])
    assert np.array_equal(res['included'], other['included'])
    assert res['n_used'] == other['n_used'] and pair_list(res) == pair_list(other)
    np.testing.assert_allclose(res['radiance'], other['radiance'], rtol=1e-12, atol=0)


# ---- a. block formation ------------------------------------------------------------------------

FORMATION = [(name, True) for name in LC.LAYOUTS] + \
            [(name, False) for name in LC.LAYOUTS if len(LC.LAYOUTS[name]) == 1]


@pytest.mark.parametrize('layout,use_index', FORMATION,
                         ids=[n + ('' if u else '-no-index') for n, u in FORMATION])
def test_block_formation_edges(ctx, layout, use_index):
    """Hand-built index columns (tests/los_edge_cases.py, LAYOUTS) under four hot and two cold
    spectra: one packet of 1 .. 513 rows (4 rows a lane, 8 a block, 8 blocks a group, 256 rows a
    region, each with one row less and one more), packets back to back over the region edges in
    both orders, a block per row, a group per packet, packet starts on every row of a lane's four,
    and packets that a region's end cuts to 9, 8 and 1 rows -- where the fresh-group decision
    flips.  One-packet layouts also without an index column."""
    c = case(layout, use_index=use_index)
    check(run(ctx, c), c)


def test_block_formation_float32_columns(ctx):
    """The back-to-back layout through nxc_los_accumulate_f32: float32 columns, widened exactly
    on the device; the reference gets the widened values."""
    c = case('b2b', f32=True)
    assert c['cols'][0].dtype == np.float32
    check(run(ctx, c), c)


# ---- b. slabs ----------------------------------------------------------------------------------

SLABS = [(name, True) for name in LC.SLAB_LAYOUTS] + [('one-513', False)]


@pytest.mark.parametrize('layout,use_index', SLABS,
                         ids=[n + ('' if u else '-no-index') for n, u in SLABS])
def test_slab_edges(ctx, monkeypatch, layout, use_index):
    """Slabs of 256 rows (NXC_TEST_LOS_SLAB_ROWS at its minimum: one region a slab), a last slab
    of ONE row, a packet across every slab edge (asserted in tests/test_los_blocks_cpu.py): the
    answers are those of the single slab.  Row numbers of the pair list and `included` slots are
    global: the reference's pairs name every row of every slab, and without an index column
    `included` is by row."""
    rows = LC.SLAB_LAYOUTS[layout]
    c = case(layout, rows=rows, use_index=use_index)
    assert c['P'] == rows and rows % 256 == 1
    one = run(ctx, c)
    monkeypatch.setenv('NXC_TEST_LOS_SLAB_ROWS', '256')
    slabs = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_SLAB_ROWS')
    same(slabs, one)
    check(slabs, c)
    check(one, c)
    assert max(row for _, row in pair_list(slabs)) == rows - 1


# ---- c. spectrum tiles and rounds --------------------------------------------------------------

@pytest.mark.parametrize('lines', [D_LINES, FOUR_LINES], ids=['two-lines', 'four-lines'])
def test_spectrum_tile_and_round_edges(ctx, lines):
    """1025 spectra over 769 rows in packets of 1 to 40: the hot ones sit on both sides of every
    tile edge (tile_cap 512 with two emission lines, 128 with four: a tile edge is a new
    blockIdx.y and a new s0) and of the 64-spectrum rounds inside a tile; the last tile holds ONE
    spectrum, a hot one.  All the other spectra are cold."""
    assert tile_cap(lines) == (512 if lines == D_LINES else 128)
    c = case('mixed', S=1025, hot=TILE_EDGES, lines=lines)
    check(run(ctx, c), c)


@pytest.mark.parametrize('S', [1, 63, 64, 65])
def test_last_spectrum_of_a_ragged_round(ctx, S):
    """1, 63, 64 and 65 spectra, only the last one hot: the last lane of a round that is not
    full, of a full one, and a round of one."""
    c = case('mixed', S=S, hot=(S - 1,))
    check(run(ctx, c), c)


# ---- d. culling off ----------------------------------------------------------------------------

CULL_OFF = [('mixed', 70), ('singles', 70), ('nines', 70), ('mixed', 64), ('mixed', 65), ('mixed', 130)]


def culling_off_case(layout, S, which):
    scaled = {'first': 0, 'middle': S//2, 'last': S - 1}[which]
    return case(layout, S=S, hot=tuple(range(S)), scaled=scaled)


def check_sphere_tests(ctx, c, slab_rows=1 << 24):
    """DevCounters.samples of the last pass against the restated slot layout."""
    slabs = LB.layouts(c['P'], c['index'], slab_rows)
    assert ctx.counters()['samples'] == LB.sphere_tests_without_culling(slabs, c['S'])
    return slabs


@pytest.mark.parametrize('which', ['first', 'middle', 'last'])
@pytest.mark.parametrize('layout,S', CULL_OFF + [('b2b', 70), ('region-tail', 70)])
def test_culling_off(ctx, layout, S, which):
    """One boresight times 1 + 1e-8 -- what a pointing vector that went through float32 looks
    like -- makes los_run set K.cull = 0 for the whole pass: k_los_blocks gives every non-empty
    slot R = +inf, so every block, half group and group passes every cone.  `pairs` then fills to
    exactly NXC_LOS_PAIRS = 512 in every full round (8 groups x 64 spectra), pairs2 to
    NXC_LOS_PAIRS2 = 256 (block_tests runs once n2 exceeds 192, and 64 more may arrive first), and
    the LosQueue ring runs full and wraps.  All spectra are hot.  The reference gets the same
    boresights: the exact pair test uses them as given on both sides.

    The sphere-test counter.  k_los adds to wave_tests (flushed to DevCounters.samples), per trip
    of 64 slots and tile of ns spectra:
      level 1   `wave_tests += 8 * (ns - c0 < 64 ? ns - c0 : 64);`           per round c0: 8 ns
      level 2   `wave_tests += 2 * (npair - at0 < 32 ? npair - at0 : 32);`   in all 2 npair
      level 3   `wave_tests += 4 * (n2 - b0 < 16 ? n2 - b0 : 16);`           in all 4 n2
    A trip is taken while `base < count` (count = the stream's length, a multiple of 8), so there
    are T = ceil(slots / 64) trips per tile, and the tiles' ns add up to S: level 1 counts 8 S T.
    With R = +inf, los_sphere_hits is true for every sphere with R >= 0, i.e. for every group and
    half group that holds a block (reach() gives -1 only where `has` is false, and the maximum
    over the group is +inf as soon as one slot has a block): npair sums to G S, n2 to H S.  So
        samples = S (8 T + 2 G + 4 H)
    with T, G, H of the restated layout -- which ties the device's slot layout (which packets open
    a group, what a region's end does to a packet, the padding of a region's last group) to
    tests/los_blocks_restatement.py exactly.  Whoever changes the culling levels or what they
    count changes this formula with them."""
    c = culling_off_case(layout, S, which)
    res = run(ctx, c)
    check_sphere_tests(ctx, c)
    check(res, c)


def test_culling_off_in_slabs(ctx, monkeypatch):
    """The counter adds up over slabs: one region a slab, every slab a trip of its own."""
    c = culling_off_case('mixed', 65, 'middle')
    monkeypatch.setenv('NXC_TEST_LOS_SLAB_ROWS', '256')
    res = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_SLAB_ROWS')
    slabs = check_sphere_tests(ctx, c, 256)
    assert len(slabs) == 4 and sum(s['T'] for s in slabs) > LB.layouts(c['P'], c['index'])[0]['T']
    check(res, c)


# ---- e. pair list full -------------------------------------------------------------------------

def with_pair_chunks(ctx, monkeypatch, c, chunks):
    # more candidates than the list holds: a pair the reference counts passed k_los' coarse cone
    # test, and every chunk a wave fills holds 64 at most -- the fallback is reached
    assert c['npackets'].sum() > 64*chunks
    monkeypatch.setenv('NXC_TEST_LOS_PAIR_CHUNKS', str(chunks))
    try:
        return run(ctx, c)
    finally:
        monkeypatch.delenv('NXC_TEST_LOS_PAIR_CHUNKS')


@pytest.mark.parametrize('chunks', [1, 2, 8])
@pytest.mark.parametrize('which', ['formation', 'culling-off'])
def test_pair_list_full(ctx, monkeypatch, which, chunks):
    """NXC_TEST_LOS_PAIR_CHUNKS = 1, 2, 8 chunks of 64 pairs instead of 2^15: once a wave's chunk
    number reaches that, k_los decides its pairs itself -- from a spectrum rebuilt out of the LDS
    tile and the ladder length in sc[7 S + ...], with the ladder in memory and sums added straight
    to memory, while k_los_pairs works through the chunks that were filled with its sums in LDS.
    Same answers as without the hook and as the reference."""
    c = case('b2b') if which == 'formation' else culling_off_case('mixed', 130, 'middle')
    assert lds_sums(c['lines'], c['n_ladder'], c['S'])
    full = run(ctx, c)
    res = with_pair_chunks(ctx, monkeypatch, c, chunks)
    same(res, full)
    check(res, c)
    check(full, c)


def test_pair_list_full_without_lds_sums(ctx, monkeypatch):
    """2800 spectra over 600 rows: too many for k_los_pairs' sums in LDS, so both kernels add to
    memory; six tiles of spectra, 40 hot ones spread over all of them, the last one among them."""
    S = 2800
    hot = tuple(range(0, S, 72)) + (S - 1,)
    c = case('mixed', rows=600, S=S, hot=hot)
    assert not lds_sums(c['lines'], c['n_ladder'], S)
    full = run(ctx, c)
    res = with_pair_chunks(ctx, monkeypatch, c, 2)
    same(res, full)
    check(res, c)
    check(full, c)


# ---- f. host pair list too small ---------------------------------------------------------------

def test_host_pair_list_too_small(ctx):
    """used_cap below, at and above the number of used pairs m: n_used counts on, `used` holds
    min(m, used_cap) different pairs of the reference, nothing else changes -- and the next call
    with room finds everything again (the n_used word lies right behind the list in the
    scratch: a write past the cap would land in it or in the call after)."""
    c = case('b2b')
    m = c['m']
    assert m > 2000
    for cap in (1, m - 1, m, m + 1):
        res = ctx.los_accumulate(*c['setup'], *c['cols'], index=c['index'], n_index=c['n_index'],
                                 used_cap=cap)
        assert res['n_used'] == m and res['used'].shape == (2, min(m, cap))
        assert pair_list(res) <= c['pairs'] and len(pair_list(res)) == min(m, cap)
        assert np.array_equal(res['npackets'], c['npackets'])
        assert np.array_equal(res['included'], c['included'])
        np.testing.assert_allclose(res['radiance'], c['radiance'], rtol=1e-10, atol=0)
        check(run(ctx, c), c)
