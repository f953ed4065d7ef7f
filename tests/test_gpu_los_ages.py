"""The line-of-sight ages (nxc_los_ages_*: k_los<.., LOS_AGES>, k_los_pairs<.., LOS_AGES>) against
their NumPy restatement (tests/los_ages_restatement.py), on the shapes of tests/los_edge_cases.py: at
most 1546 rows and (but for one case) 1025 spectra.

Every route is compared in check(): the zero pattern of the records exactly, the records to rtol
1e-10 (the pass's own figure for radiance against the oracle), npackets, `included` and the pair
set exactly, and radiance to rtol 1e-12 against the plain pass over the same input (the pass's own
figure for two device routes); a plain pass and a profile pass afterwards leave the ages block bit
for bit as it was, and an ages pass leaves an enabled profile block as it was."""
import contextlib
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from oracle import np_oracle as O
from tests import helpers as H
from tests import los_ages_cases as AC
from tests import los_edge_cases as LC
from tests import tile_plan_restatement as TP
from tests.los_ages_restatement import los_ages

pytestmark = pytest.mark.gpu

INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
LDS_HEADER = 4224                         # NXC_HEADER_BYTES (nxc_device.hpp)
# hot spectra on both sides of every tile edge k_los can have and of the rounds of 64 spectra
TILE_EDGES = (0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
PLAIN = ('x', 'y', 'z', 'vy', 'frac')
PROFILE_BINS = (5, -1.5e-3, 2.5e-3)       # of the profile block that an ages pass must leave alone


def lds_sums(c):
    """los_run (nxc_api.hip): does k_los_pairs keep its per-spectrum sums in LDS?  16 bytes per
    spectrum for an ages pass, as for the plain one: the records are no sums of that kind."""
    stage = LDS_HEADER + sum(TP.lut_bytes(len(v)) for v, _ in LC.g_tables(c['lines']))
    return ((stage + 31) & ~31) + ((c['n_ladder'] + 3) & ~3)*8 + c['S']*16 <= 80*1024


def samples_of(c, **extra):
    """How the case's samples reach los_accumulate: its host columns, or c['rows'] of a store."""
    if 'rows' in c:
        return dict(rows=c['rows'], n_index=c['n_index'])
    cols = c['cols']
    args = dict(zip(PLAIN, (cols[k] for k in PLAIN)))
    return dict(args, index=c['index'], n_index=c['n_index'], **{k: v(cols) for k, v in extra.items()})


def run(ctx, c, enable=True, used_cap=None):
    """One ages pass over the case's samples: (result, sums)."""
    if enable:
        ctx.los_ages_enable(c['S'], *c['bins'])
    res = ctx.los_accumulate(*c['setup'], used_cap=c['m'] + 64 if used_cap is None else used_cap,
                             ages=True, **samples_of(c, time=lambda cols: cols['time']))
    return res, ctx.los_ages_download()


def run_plain(ctx, c):
    return ctx.los_accumulate(*c['setup'], used_cap=c['m'] + 64, **samples_of(c))


def run_profile(ctx, c):
    """A profile pass over the same samples; any velocities will do (zeros of the columns' type)."""
    zero = lambda cols: np.zeros_like(cols['x'])              # noqa: E731
    return ctx.los_accumulate(*c['setup'], used_cap=c['m'] + 64, profile=True,
                              **samples_of(c, vx=zero, vz=zero))


def pair_list(res):
    got = list(zip(res['used'][0].tolist(), res['used'][1].tolist()))
    assert len(got) == len(set(got))                           # no pair twice
    return set(got)


def check_sums(sums, want, times=1):
    """The records against the restatement's (times: the passes that were added up)."""
    assert sums.shape == want.sums.shape
    assert np.array_equal(sums == 0, want.sums == 0)
    np.testing.assert_allclose(sums, times*want.sums, rtol=1e-10, atol=0)


def check(ctx, c, got):
    res, sums = got
    want = c['want']
    assert np.array_equal(res['npackets'], want.npackets)
    assert np.array_equal(res['included'], want.included)
    assert res['n_used'] == c['m'] == res['used'].shape[1] and pair_list(res) == want.pairs
    np.testing.assert_allclose(res['radiance'], want.radiance, rtol=1e-10, atol=0)
    check_sums(sums, want)
    hot = want.npackets > 0
    np.testing.assert_allclose(sums[hot, :, 0].sum(1), res['radiance'][hot], rtol=1e-12, atol=0)
    plain = run_plain(ctx, c)
    assert np.array_equal(res['npackets'], plain['npackets'])
    assert np.array_equal(res['included'], plain['included'])
    assert pair_list(res) == pair_list(plain)
    np.testing.assert_allclose(res['radiance'], plain['radiance'], rtol=1e-12, atol=0)
    # the plain pass and a profile pass leave the ages alone ...
    ctx.los_profile_enable(c['S'], *PROFILE_BINS)
    prof = run_profile(ctx, c)
    assert np.array_equal(prof['npackets'], plain['npackets'])
    assert np.array_equal(ctx.los_ages_download(), sums)
    # ... and an ages pass the profile
    before = ctx.los_profile_download()
    assert before[0].any() == bool(c['m'])
    again = ctx.los_accumulate(*c['setup'], used_cap=c['m'] + 64, ages=True,
                               **samples_of(c, time=lambda cols: cols['time']))
    assert np.array_equal(again['npackets'], plain['npackets'])
    after = ctx.los_profile_download()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1], equal_nan=True)
    ctx.los_profile_enable(c['S'], 0)
    np.testing.assert_allclose(ctx.los_ages_download(), 2*sums, rtol=1e-12, atol=0)


# ---- 1. layouts, column types, index column -------------------------------------------------------
@pytest.mark.parametrize('use_index', [True, False], ids=['index', 'no-index'])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('layout', ['b2b', 'mixed'])
def test_layouts_and_column_types(ctx, layout, f32, use_index):
    c = AC.case(layout, f32=f32, use_index=use_index)
    assert c['cols']['time'].dtype == (np.float32 if f32 else np.float64)
    assert lds_sums(c) and c['P'] <= 1546
    check(ctx, c, run(ctx, c))


# ---- 2. slabs ---------------------------------------------------------------------------------------
def test_slabs_of_256_rows(ctx, monkeypatch):
    """769 rows in slabs of 256: the last slab is one row, and the time moves with the slab."""
    c = AC.case('mixed')
    assert c['P'] == 769
    one = run(ctx, c)
    check(ctx, c, one)
    monkeypatch.setenv('NXC_TEST_LOS_SLAB_ROWS', '256')
    slabs = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_SLAB_ROWS')
    check(ctx, c, slabs)
    np.testing.assert_allclose(slabs[1], one[1], rtol=1e-12, atol=0)
    assert max(row for _, row in pair_list(slabs[0])) == 768


# ---- 3. the pair list full: k_los decides pairs itself ---------------------------------------------
@pytest.mark.parametrize('chunks', [1, 8])
def test_pair_list_full(ctx, monkeypatch, chunks):
    """NXC_TEST_LOS_PAIR_CHUNKS: k_los' own route -- sums in memory, the time loaded there -- beside
    k_los_pairs with its sums in LDS."""
    c = AC.case('b2b')
    assert lds_sums(c)
    # more candidates than the list holds: the fallback is reached
    assert c['want'].npackets.sum() > 64*chunks
    monkeypatch.setenv('NXC_TEST_LOS_PAIR_CHUNKS', str(chunks))
    got = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_PAIR_CHUNKS')
    check(ctx, c, got)


# ---- 4. the sums of k_los_pairs in memory ----------------------------------------------------------
def test_without_lds_sums(ctx, monkeypatch):
    """2800 spectra over 600 rows: the pass does not keep its sums in LDS; also with a full list."""
    S = 2800
    c = AC.case('mixed', rows=600, S=S, hot=tuple(range(0, S, 72)) + (S - 1,))
    assert not lds_sums(c)
    check(ctx, c, run(ctx, c))
    monkeypatch.setenv('NXC_TEST_LOS_PAIR_CHUNKS', '2')
    got = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_PAIR_CHUNKS')
    check(ctx, c, got)


# ---- 5. tile edges -----------------------------------------------------------------------------------
def test_spectrum_tile_edges(ctx):
    """1025 spectra, hot ones on both sides of every tile and round edge, the last tile ONE hot
    spectrum; S * 16 bytes fit k_los_pairs' LDS."""
    c = AC.case('mixed', S=1025, hot=TILE_EDGES)
    assert lds_sums(c)
    check(ctx, c, run(ctx, c))


# ---- 6. bin edges exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_bin_edges(ctx, f32):
    """A time on every edge, one ulp either side of it and at -0.0 (tests/los_ages_cases.py,
    edge_case): every row alone decides where its own, different, wtemp goes."""
    c, record = AC.edge_case(f32)
    got = run(ctx, c)
    check(ctx, c, got)
    assert np.array_equal(got[1][0, :, 0] != 0, np.bincount(record, minlength=10) > 0)


# ---- 7. pairs without weight -------------------------------------------------------------------------
def test_shadowed_foot_points_with_nan_times(ctx):
    """The ball behind the planet (y > 0, rho < 1), seen from further behind, every time a NaN:
    every pair is decided and counted, every wtemp is 0, the time is not read and the records stay
    exactly 0 -- the top plane too."""
    ids = LC.layout_ids('mixed', 300)
    smp = dict(LC.cloud(ids, 8))
    smp['y'] = -smp['y']                                      # the ball around (0, +3, 0)
    smp['time'] = np.full(300, np.nan)
    pos = np.array([[0.0, 8.0, 0.0], [0.0, 8.0, 0.0]])
    look = np.array([[0.0, -1.0, 0.0], [0.0, 1.0, 0.0]])      # at the ball; away from it
    c = AC.build(smp, ids, pos, look, filled=False)
    want = c['want']
    assert list(want.npackets) == [300, 0] and want.included.all() and not want.pairs
    assert not want.radiance.any()
    res, sums = run(ctx, c, used_cap=8)
    assert np.array_equal(res['npackets'], want.npackets) and res['n_used'] == 0
    assert np.array_equal(res['included'], want.included)
    assert not res['radiance'].any() and not sums.any()


def test_rows_without_frac_with_nan_times(ctx):
    """frac = 0 and a NaN time on every third row, and bins that reach past every age: the rows
    are counted, add nothing, and nothing reaches the top plane."""
    ids = LC.layout_ids('mixed', 300)
    smp = dict(LC.cloud(ids, 9))
    smp['time'] = np.random.default_rng(9).uniform(0.0, AC.T0, 300)
    smp['frac'] = smp['frac'].copy()
    smp['frac'][::3] = 0.0
    smp['time'][::3] = np.nan
    pos, look = LC.lines_of_sight(4, (0, 2), 9)
    c = AC.build(smp, ids, pos, look, bins=(AC.NA, AC.T0, 0.0, 4000.0), filled=False)
    want = c['want']
    assert want.npackets[0] == 300 and not want.sums[:, -1].any() and not want.sums[:, 0].any()
    assert not any(row % 3 == 0 for _, row in want.pairs) and c['m'] >= 200
    got = run(ctx, c)
    check(ctx, c, got)
    assert not got[1][:, -1].any()


# ---- 8. accumulation, state --------------------------------------------------------------------------
def test_accumulation_reenable_and_the_plain_pass(ctx):
    c = AC.case('mixed')
    first = run(ctx, c)
    plain = run_plain(ctx, c)                                  # between the two: adds nothing
    second = run(ctx, c, enable=False)
    np.testing.assert_allclose(second[0]['radiance'], plain['radiance'], rtol=1e-12, atol=0)
    check_sums(second[1], c['want'], times=2)
    np.testing.assert_allclose(second[1], 2*first[1], rtol=1e-12, atol=0)
    ctx.los_ages_enable(c['S'], *c['bins'])
    assert not ctx.los_ages_download().any()
    check(ctx, c, run(ctx, c, enable=False))
    # another shape replaces it
    ctx.los_ages_enable(3, 2, 10.0, -1.0, 1.0)
    sums = ctx.los_ages_download()
    assert sums.shape == (3, 4, 2) and not sums.any()


def test_state_and_argument_errors(ctx):
    from nexoclom_amd import hip_api
    c = AC.case('mixed')
    ctx.los_ages_enable(c['S'], 0)                             # off
    for call in (lambda: run(ctx, c, enable=False), ctx.los_ages_download):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'nxc_los_ages_enable' in str(err.value)
    run_plain(ctx, c)                                          # the plain entry needs no block
    ctx.los_ages_enable(c['S'] + 1, *c['bins'])
    with pytest.raises(hip_api.HipError) as err:
        run(ctx, c, enable=False)
    assert err.value.code == hip_api.NXC_ERR_ARG
    sums = ctx.los_ages_download()
    assert sums.shape == (c['S'] + 1, AC.NA + 2, 2) and not sums.any()
    for bad in ((0, 4, 10.0, 0.0, 1.0), (4, -1, 10.0, 0.0, 1.0), (4, 4, 10.0, 1.0, 1.0),
                (4, 4, 10.0, np.nan, 1.0), (4, 4, np.inf, 0.0, 1.0), (4, 4, 10.0, 0.0, np.inf),
                (4, 4, 10.0, -1.7e308, 1.7e308), (2**20, 2**11 - 2, 10.0, 0.0, 1.0)):
        with pytest.raises(hip_api.HipError) as err:
            ctx.los_ages_enable(*bad)
        assert err.value.code == hip_api.NXC_ERR_ARG and 'line-of-sight ages' in str(err.value)
        assert ctx.los_ages_download().shape == sums.shape     # refused before anything changed
    ctx.los_ages_enable(c['S'], *c['bins'])
    assert not run(ctx, dict(c, cols={k: v[:0] for k, v in c['cols'].items()}, index=c['index'][:0]),
                   enable=False, used_cap=8)[1].any()          # P == 0 adds nothing
    ctx.los_ages_enable(1, 0)


# ---- 9. row stores -----------------------------------------------------------------------------------
STORE_BINS = (50, 3000.0, -15.0, 1485.0)        # the step is 30 s: no age on an edge


@pytest.fixture(scope='module', params=[True, False], ids=['narrow', 'wide'])
def store(request, ctx):
    """Rows of integrate_const_rows in HBM (float32 / int32, or 64-bit), their host copy and index:
    15 packets over 100 steps."""
    endtime, step = STORE_BINS[1], 30.
    X0 = H.sample_x0(15, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, LC.forces())
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    st = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=request.param, resident=True)['store']
    try:
        assert st.narrow == request.param and 400 < st.total <= 1546
        rows, idx = st.download()
        assert rows.dtype == (np.float32 if request.param else np.float64)
        yield st, rows, idx
    finally:
        st.free()


@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, store, part):
    """Rows in HBM (narrow and wide stores), whole and as a slice with first > 0 that ends inside
    the store, against the same rows sent from the host in their own width, and both against the
    restatement.  Six spectra look straight down at a lit row each."""
    st, rows, idx = store
    first, count = (0, st.total) if part == 'whole' else (77, st.total - 77 - 99)
    part_rows = rows[:, first:first + count].astype(np.float64)
    smp = dict(zip(('time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'), part_rows))
    lit = np.nonzero(((smp['y'] < 0) | (smp['x']**2 + smp['z']**2 > 1)) & (smp['frac'] > 0))[0]
    at = lit[np.linspace(0, len(lit) - 1, 6).astype(int)]
    target = np.stack([smp['x'][at], smp['y'][at], smp['z'][at]], 1)
    up = target/np.linalg.norm(target, axis=1)[:, None]
    c = AC.build(smp, idx[first:first + count].astype(np.int64), target + 4.0*up, -up,
                 bins=STORE_BINS, f32=st.narrow, filled=False, n_index=15)
    assert np.array_equal(c['cols']['time'], rows[0, first:first + count])
    assert c['m'] >= 6 and np.count_nonzero(c['want'].sums[..., 0].sum(0)) >= 3
    host = run(ctx, c)
    check(ctx, c, host)
    in_hbm = dict(c, rows=(st, first, count, 0))
    got = run(ctx, in_hbm)
    check(ctx, in_hbm, got)
    assert np.array_equal(got[0]['npackets'], host[0]['npackets'])
    assert np.array_equal(got[0]['included'], host[0]['included'])
    assert pair_list(got[0]) == pair_list(host[0])
    assert np.array_equal(got[1] == 0, host[1] == 0)
    np.testing.assert_allclose(got[1], host[1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[0]['radiance'], host[0]['radiance'], rtol=1e-12, atol=0)


# ---- 10. the public class ----------------------------------------------------------------------------
def test_losresult_ages_resident_and_restored(ctx, tmp_path):
    from nexoclom_amd import Input, LOSResult, SpacecraftData
    from nexoclom_amd.Output import Output
    inputs = Input(INPUT, savepath=str(tmp_path))
    inputs.options.endtime = type(inputs.options.endtime)(3000., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2000, packs_per_it=1000, seed=81, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 2 and all(o.resident_rows(ctx) is not None for o in outs)
    restored = Input(INPUT)
    restored.options.endtime = inputs.options.endtime
    files = inputs.search()[1]
    for k, f in enumerate(files):
        back = Output.restore(f)
        back.idnum = k + 1
        restored._catalogue.append(back)
    rng = np.random.default_rng(4)
    th = np.linspace(0, 2*np.pi, 40, endpoint=False)
    r = 1.6 + 1.2*rng.random(40)
    pos = np.stack([0.3*r*np.cos(th), r*np.sin(th)*0.6 - 0.4, r*np.sin(th)*0.8], 1)
    look = -pos + 0.6*rng.normal(size=pos.shape)
    look /= np.linalg.norm(look, axis=1)[:, None]
    taken = np.linspace(0.0, 7800.0, 40)
    sc = SpacecraftData(*pos.T, *look.T, time=taken)
    sc.data.index = np.arange(100, 140)                       # results follow the data's index
    ages, dphi = (-15.0, 2685.0, 9), np.radians(3.0)          # off the grid of the rows' times
    with contextlib.redirect_stdout(io.StringIO()):
        plain = LOSResult(sc, inputs, dphi=dphi, context=ctx)
        plain.simulate_data_from_inputs(sc)
        resident = LOSResult(sc, inputs, dphi=dphi, context=ctx, ages=ages)
        resident.simulate_data_from_inputs(sc)
        host = LOSResult(sc, restored, dphi=dphi, context=ctx, ages=ages)
        host.simulate_data_from_inputs(sc)
    assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
    assert not hasattr(plain, 'age_profile') and not hasattr(plain, 'age_sums')
    # the restatement over the stored (float32) rows of both Outputs
    unit = resident.unit_km
    scd = {c: sc.data[c].values for c in sc.data.columns}
    sums, radiance = 0, 0
    for out, f in zip(outs, files):
        X = Output.restore(f).X
        smp = {c: X[c].values.astype(np.float64) for c in AC.COLUMNS}
        smp['Index'] = Output.packet_index(X)
        want = los_ages(smp, scd, dphi, inputs.options.outeredge, float(out.vrplanet)/unit,
                        resident.g_tables(float(out.aplanet)), unit*1e5, ages[2], 3000.0,
                        ages[0], ages[1], n_index=int(out.npackets))
        sums, radiance = sums + want.sums, radiance + want.radiance
    lit = radiance > 0
    assert lit.sum() >= 3 and np.count_nonzero(sums[..., 1:-1, 0].sum(0)) >= 5
    assert sums[:, -1, 0].sum() > 0                           # rows older than 2685 s
    scale = resident.atoms_per_packet/1e3
    for obj in (resident, host):
        assert np.array_equal(obj.npackets_los.values, plain.npackets_los.values)
        np.testing.assert_allclose(obj.radiance.values, plain.radiance.values, rtol=1e-12, atol=0)
        assert list(obj.radiance.index) == list(obj.age_profile.index) == list(obj.age_below.index)
        assert obj.age_profile.shape == (40, 9) and obj.age_sums.shape == (40, 11, 2)
        assert np.array_equal(obj.age_sums == 0, sums == 0)
        np.testing.assert_allclose(obj.age_sums, sums, rtol=1e-10, atol=0)
        total = obj.age_profile.sum(1) + obj.age_below + obj.age_above
        np.testing.assert_allclose(total.values, obj.radiance.values, rtol=1e-12, atol=0)
        np.testing.assert_allclose(obj.age_profile.values, obj.age_sums[:, 1:-1, 0]*scale, rtol=1e-15)
        np.testing.assert_allclose(obj.age_edges, np.linspace(-15, 2685, 10), atol=1e-12)
        assert obj.age_axis.shape == (9,) and obj.age_effective_packets.shape == (40, 9)
        assert not obj.age_effective_packets.values[~lit].any()
        # the steady state: a constant history of one, at the spectra's own times
        steady = obj.transient(([0.0], [1.0]))
        assert np.array_equal(steady.times, taken) and np.all(steady.kernel == 1.0)
        ordered = np.zeros(40)
        for k in range(11):
            ordered = ordered + obj.age_sums[:, k, 0]
        assert np.array_equal(steady.radiance.values, ordered*scale)
        np.testing.assert_allclose(steady.radiance.values, obj.radiance.values, rtol=1e-12, atol=0)
        assert np.all(steady.effective_packets.values[lit] >= 1 - 1e-12)
        # a source switched on at t = 3000 s: early spectra see nothing, late ones all but the old rows
        on = obj.transient(([3000.0, 3000.0 + 1e-3], [0.0, 1.0]))
        assert not on.radiance.values[taken < 2900].any()
        late = lit & (taken > 3000 + 2700)
        assert late.any()
        np.testing.assert_allclose(on.radiance.values[late],
                                   (obj.radiance - obj.age_above).values[late], rtol=1e-9, atol=0)
        A = obj.transient_design([0.0, 3000.0, 6000.0])
        np.testing.assert_allclose(A.sum(1), obj.radiance.values, rtol=1e-12, atol=0)
    np.testing.assert_allclose(resident.age_sums, host.age_sums, rtol=1e-10, atol=0)
