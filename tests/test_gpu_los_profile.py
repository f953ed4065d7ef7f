"""The line-of-sight profile (nxc_los_profile_*: k_los<.., true>, k_los_pairs<.., true>) against its
NumPy restatement (tests/los_profile_restatement.py), on the shapes of tests/los_edge_cases.py: at
most 1546 rows and (but for one case) 1025 spectra.

Every route is compared in check(): the zero pattern of the records exactly, the records to rtol
1e-10 (the pass's own figure for radiance against the oracle), each moment sum to 1e-10 of the sum
of its terms' magnitudes (the terms are signed and may cancel: no rtol), npackets, `included` and
the pair set exactly, and radiance to rtol 1e-12 against the plain pass over the same input (the
pass's own figure for two device routes)."""
import contextlib
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from tests import los_edge_cases as LC
from tests import los_profile_cases as PC
from tests import tile_plan_restatement as TP
from tests.los_profile_restatement import los_profile

pytestmark = pytest.mark.gpu

INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
LDS_HEADER = 4224                         # NXC_HEADER_BYTES (nxc_device.hpp)
# hot spectra on both sides of every tile edge k_los can have and of the rounds of 64 spectra
TILE_EDGES = (0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
PLAIN = ('x', 'y', 'z', 'vy', 'frac')


def lds_sums(c, profile):
    """los_run (nxc_api.hip): does k_los_pairs keep its per-spectrum sums in LDS?  16 bytes per
    spectrum for the plain pass, 48 with the four moment sums."""
    stage = LDS_HEADER + sum(TP.lut_bytes(len(v)) for v, _ in LC.g_tables(c['lines']))
    return ((stage + 31) & ~31) + ((c['n_ladder'] + 3) & ~3)*8 + c['S']*(48 if profile else 16) <= 80*1024


def run(ctx, c, enable=True, used_cap=None):
    """One profile pass over the case's host columns: (result, sums, moments)."""
    if enable:
        ctx.los_profile_enable(c['S'], *c['bins'])
    cols = c['cols']
    res = ctx.los_accumulate(*c['setup'], *(cols[k] for k in PLAIN), index=c['index'],
                             n_index=c['n_index'], used_cap=c['m'] + 64 if used_cap is None else used_cap,
                             vx=cols['vx'], vz=cols['vz'], profile=True)
    return (res,) + ctx.los_profile_download()


def run_plain(ctx, c):
    return ctx.los_accumulate(*c['setup'], *(c['cols'][k] for k in PLAIN), index=c['index'],
                              n_index=c['n_index'], used_cap=c['m'] + 64)


def pair_list(res):
    got = list(zip(res['used'][0].tolist(), res['used'][1].tolist()))
    assert len(got) == len(set(got))                           # no pair twice
    return set(got)


def check_sums(sums, moments, want, times=1, nonfinite=()):
    """Records and moments against the restatement's (times: the passes that were added up;
    nonfinite: spectra whose m1, m2, m3 must not be finite)."""
    assert sums.shape == want.sums.shape and moments.shape == want.moments.shape
    assert np.array_equal(sums == 0, want.sums == 0)
    np.testing.assert_allclose(sums, times*want.sums, rtol=1e-10, atol=0)
    finite = np.ones(moments.shape, dtype=bool)
    finite[list(nonfinite), :3] = False
    assert np.array_equal(np.isfinite(moments), finite)
    assert np.array_equal(np.isfinite(want.moments), finite)
    err = np.abs(moments - times*want.moments)[finite]
    assert np.all(err <= 1e-10*times*want.moment_mags[finite])


def check(ctx, c, got, nonfinite=()):
    res, sums, moments = got
    want = c['want']
    assert np.array_equal(res['npackets'], want.npackets)
    assert np.array_equal(res['included'], want.included)
    assert res['n_used'] == c['m'] == res['used'].shape[1] and pair_list(res) == want.pairs
    np.testing.assert_allclose(res['radiance'], want.radiance, rtol=1e-10, atol=0)
    check_sums(sums, moments, want, nonfinite=nonfinite)
    plain = run_plain(ctx, c)
    assert np.array_equal(res['npackets'], plain['npackets'])
    assert np.array_equal(res['included'], plain['included'])
    assert pair_list(res) == pair_list(plain)
    np.testing.assert_allclose(res['radiance'], plain['radiance'], rtol=1e-12, atol=0)
    # the plain pass left the profile alone
    again = ctx.los_profile_download()
    assert np.array_equal(again[0], sums) and np.array_equal(again[1], moments, equal_nan=True)


# ---- 1. layouts, column types, index column -------------------------------------------------------
@pytest.mark.parametrize('use_index', [True, False], ids=['index', 'no-index'])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('layout', ['b2b', 'mixed'])
def test_layouts_and_column_types(ctx, layout, f32, use_index):
    c = PC.case(layout, f32=f32, use_index=use_index)
    assert c['cols']['vx'].dtype == (np.float32 if f32 else np.float64)
    assert lds_sums(c, True)
    check(ctx, c, run(ctx, c))


# ---- 2. slabs ---------------------------------------------------------------------------------------
def test_slabs_of_256_rows(ctx, monkeypatch):
    """769 rows in slabs of 256: the last slab is one row, and vx, vz move with the slab."""
    c = PC.case('mixed')
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
    """NXC_TEST_LOS_PAIR_CHUNKS: k_los' own route -- sums in memory, vx and vz loaded there -- beside
    k_los_pairs with its sums in LDS."""
    c = PC.case('b2b')
    assert lds_sums(c, True)
    # more candidates than the list holds: the fallback is reached
    assert c['want'].npackets.sum() > 64*chunks
    monkeypatch.setenv('NXC_TEST_LOS_PAIR_CHUNKS', str(chunks))
    got = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_PAIR_CHUNKS')
    check(ctx, c, got)


# ---- 4. the sums of k_los_pairs in memory ----------------------------------------------------------
def test_without_lds_sums(ctx, monkeypatch):
    """2800 spectra over 600 rows: neither pass keeps its sums in LDS; also with a full list."""
    S = 2800
    c = PC.case('mixed', rows=600, S=S, hot=tuple(range(0, S, 72)) + (S - 1,))
    assert not lds_sums(c, True) and not lds_sums(c, False)
    check(ctx, c, run(ctx, c))
    monkeypatch.setenv('NXC_TEST_LOS_PAIR_CHUNKS', '2')
    got = run(ctx, c)
    monkeypatch.delenv('NXC_TEST_LOS_PAIR_CHUNKS')
    check(ctx, c, got)


# ---- 5. (and 4.) tile edges; plain sums in LDS, the profile's not ------------------------------------
def test_spectrum_tile_edges(ctx):
    """1025 spectra, hot ones on both sides of every tile and round edge, the last tile ONE hot
    spectrum.  S * 16 bytes fit k_los_pairs' LDS, S * 48 do not: the profile pass adds to memory
    where the plain pass over the same input adds in LDS."""
    c = PC.case('mixed', S=1025, hot=TILE_EDGES)
    assert lds_sums(c, False) and not lds_sums(c, True)
    check(ctx, c, run(ctx, c))


# ---- 6. bin edges exactly ----------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_bin_edges(ctx, f32):
    """vlos == vy on every edge, one ulp below it and at -0.0 (tests/los_profile_cases.py,
    edge_case): every row alone decides where its own, different, wtemp goes."""
    c, record = PC.edge_case(f32)
    got = run(ctx, c)
    check(ctx, c, got)
    assert np.array_equal(got[1][0, :, 0] != 0, np.bincount(record, minlength=10) > 0)


# ---- 7. non-finite velocities ------------------------------------------------------------------------
def test_nonfinite_velocities(ctx):
    """vx = inf and NaN under the boresight (0, 1, 0): 0 * inf is not a number, the pairs go to
    record nv + 1 and m1, m2, m3 of that spectrum are not finite (ww is).  A second spectrum that
    does not see those rows is untouched."""
    ids = LC.layout_ids('mixed', 300)
    smp = dict(LC.cloud(ids, 7))
    smp['vx'], smp['vz'] = PC.velocities(300, 7)
    side = np.array([5.0, 0.0, 0.0])/np.sqrt(25.0)            # a part of the ball, from the side
    pos = np.vstack([PC.ALONG_Y[0], LC.CENTRE + 5.0*side])
    off = np.radians(4.0)
    look = np.vstack([PC.ALONG_Y[1], -np.cos(off)*side + np.sin(off)*np.array([0.0, 0.0, 1.0])])
    first = PC.build(smp, ids, pos, look, filled=False)
    seen = {row for s, row in first['want'].pairs if s == 1}
    unseen = sorted(set(range(300)) - seen)
    assert 20 < len(seen) < 280 and first['want'].npackets[0] == 300
    smp['vx'] = smp['vx'].copy()
    smp['vx'][unseen[:4]] = [np.inf, np.nan, -np.inf, np.nan]
    c = PC.build(smp, ids, pos, look, filled=False)
    want = c['want']
    assert want.pairs == first['want'].pairs
    assert all(want.planes[(0, row)] == PC.NV + 1 for row in unseen[:4])
    assert np.array_equal(want.sums[1], first['want'].sums[1])
    got = run(ctx, c)
    check(ctx, c, got, nonfinite=(0,))
    assert ctx.counters()['nonfinite'] == 0                   # the weights are finite


# ---- 8. the foot points in shadow --------------------------------------------------------------------
def test_shadowed_foot_points(ctx):
    """The ball behind the planet (y > 0, rho < 1), seen from further behind: every pair is decided
    and counted, every wtemp is 0, records and moments stay exactly 0."""
    ids = LC.layout_ids('mixed', 300)
    smp = dict(LC.cloud(ids, 8))
    smp['y'] = -smp['y']                                      # the ball around (0, +3, 0)
    smp['vx'], smp['vz'] = PC.velocities(300, 8)
    pos = np.array([[0.0, 8.0, 0.0], [0.0, 8.0, 0.0]])
    look = np.array([[0.0, -1.0, 0.0], [0.0, 1.0, 0.0]])      # at the ball; away from it
    c = PC.build(smp, ids, pos, look, filled=False)
    want = c['want']
    assert list(want.npackets) == [300, 0] and want.included.all() and not want.pairs
    assert not want.radiance.any()
    res, sums, moments = run(ctx, c, used_cap=8)
    assert np.array_equal(res['npackets'], want.npackets) and res['n_used'] == 0
    assert np.array_equal(res['included'], want.included)
    assert not res['radiance'].any() and not sums.any() and not moments.any()


# ---- 9. accumulation, 10. state ----------------------------------------------------------------------
def test_accumulation_reenable_and_the_plain_pass(ctx):
    c = PC.case('mixed')
    first = run(ctx, c)
    plain = run_plain(ctx, c)                                  # between the two: adds nothing
    second = run(ctx, c, enable=False)
    np.testing.assert_allclose(second[0]['radiance'], plain['radiance'], rtol=1e-12, atol=0)
    check_sums(second[1], second[2], c['want'], times=2)
    np.testing.assert_allclose(second[1], 2*first[1], rtol=1e-12, atol=0)
    ctx.los_profile_enable(c['S'], *c['bins'])
    sums, moments = ctx.los_profile_download()
    assert not sums.any() and not moments.any()
    check(ctx, c, run(ctx, c, enable=False))
    # another shape replaces it
    ctx.los_profile_enable(3, 2, -1.0, 1.0)
    sums, moments = ctx.los_profile_download()
    assert sums.shape == (3, 4, 2) and not sums.any() and not moments.any()


def test_state_and_argument_errors(ctx):
    from nexoclom_amd import hip_api
    c = PC.case('mixed')
    ctx.los_profile_enable(c['S'], 0)                          # off
    for call in (lambda: run(ctx, c, enable=False), ctx.los_profile_download):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'nxc_los_profile_enable' in str(err.value)
    ctx.los_profile_enable(c['S'] + 1, *c['bins'])
    with pytest.raises(hip_api.HipError) as err:
        run(ctx, c, enable=False)
    assert err.value.code == hip_api.NXC_ERR_ARG
    sums, moments = ctx.los_profile_download()
    assert sums.shape == (c['S'] + 1, PC.NV + 2, 2) and not sums.any() and not moments.any()
    for bad in ((0, 4, -1.0, 1.0), (4, -1, -1.0, 1.0), (4, 4, 1.0, 1.0), (4, 4, np.nan, 1.0),
                (2**20, 2**11 - 2, -1.0, 1.0)):
        with pytest.raises(hip_api.HipError) as err:
            ctx.los_profile_enable(*bad)
        assert err.value.code == hip_api.NXC_ERR_ARG
        assert ctx.los_profile_download()[0].shape == sums.shape     # refused before anything changed
    ctx.los_profile_enable(c['S'], *c['bins'])
    assert not run(ctx, dict(c, cols={k: v[:0] for k, v in c['cols'].items()}, index=c['index'][:0]),
                   enable=False, used_cap=8)[1].any()          # P == 0 adds nothing
    ctx.los_profile_enable(1, 0)


# ---- 11. the public classes --------------------------------------------------------------------------
def test_losresult_profile_resident_and_restored(ctx, tmp_path):
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
    sc = SpacecraftData(*pos.T, *look.T)
    sc.data.index = np.arange(100, 140)                       # results follow the data's index
    profile, dphi = (-6.0, 6.0, 12), np.radians(3.0)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = LOSResult(sc, inputs, dphi=dphi, context=ctx)
        plain.simulate_data_from_inputs(sc)
        resident = LOSResult(sc, inputs, dphi=dphi, context=ctx, profile=profile)
        resident.simulate_data_from_inputs(sc)
        host = LOSResult(sc, restored, dphi=dphi, context=ctx, profile=profile)
        host.simulate_data_from_inputs(sc)
    assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
    assert not hasattr(plain, 'profile') and not hasattr(plain, 'moment_sums')
    # the restatement over the stored (float32) rows of both Outputs
    unit = resident.unit_km
    scd = {c: sc.data[c].values for c in sc.data.columns}
    sums, moments, mags, radiance = 0, 0, 0, 0
    for out, f in zip(outs, files):
        X = Output.restore(f).X
        smp = {c: X[c].values.astype(np.float64) for c in PC.COLUMNS}
        smp['Index'] = Output.packet_index(X)
        want = los_profile(smp, scd, dphi, inputs.options.outeredge, float(out.vrplanet)/unit,
                           resident.g_tables(float(out.aplanet)), unit*1e5, profile[2],
                           profile[0]/unit, profile[1]/unit, n_index=int(out.npackets))
        sums, moments, mags = sums + want.sums, moments + want.moments, mags + want.moment_mags
        radiance = radiance + want.radiance
    lit = radiance > 0
    assert lit.sum() >= 3 and np.count_nonzero(sums[..., 1:-1, 0].sum(0)) >= 2
    scale = resident.atoms_per_packet/1e3
    for obj in (resident, host):
        assert np.array_equal(obj.npackets_los.values, plain.npackets_los.values)
        np.testing.assert_allclose(obj.radiance.values, plain.radiance.values, rtol=1e-12, atol=0)
        assert list(obj.radiance.index) == list(obj.profile.index) == list(obj.velocity.index)
        assert obj.profile.shape == (40, 12) and obj.profile_sums.shape == (40, 14, 2)
        assert np.array_equal(obj.profile_sums == 0, sums == 0)
        np.testing.assert_allclose(obj.profile_sums, sums, rtol=1e-10, atol=0)
        assert np.all(np.abs(obj.moment_sums - moments) <= 1e-10*mags)
        total = obj.profile.sum(1) + obj.profile_below + obj.profile_above
        np.testing.assert_allclose(total.values, obj.radiance.values, rtol=1e-9, atol=0)
        np.testing.assert_allclose(obj.profile.values, obj.profile_sums[:, 1:-1, 0]*scale, rtol=1e-15)
        S0 = obj.radiance.values/scale
        np.testing.assert_allclose(obj.velocity.values[lit], obj.moment_sums[lit, 0]/S0[lit]*unit,
                                   rtol=1e-12, atol=0)
        assert np.isnan(obj.velocity.values[~lit]).all() and not obj.effective_packets.values[~lit].any()
        assert np.all(obj.effective_packets.values[lit] >= 1 - 1e-12)
        np.testing.assert_allclose(obj.velocity_edges, np.linspace(-6, 6, 13), atol=1e-14)
        assert obj.velocity_axis.shape == (12,) and obj.profile_effective_packets.shape == (40, 12)
    np.testing.assert_allclose(resident.profile_sums, host.profile_sums, rtol=1e-10, atol=0)
