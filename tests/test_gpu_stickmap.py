"""Sticking from a surface map (sticking law 2: bounce_packet / stick_map_at) on the GPU: one
impact at a time, through every kernel variant that carries BOUNCE, through the public API and
at the C ABI.

Single impacts use the construction of tests/test_gpu_bounce.py (single_impact, libm_rows,
check_rows are imported from there); the restatement is tests/stickmap_restatement.py, put in the
place of bounce_cases.restate for the length of a test so that the one-ulp harness nudges the
atan2 and asin of the impact point too.

Tolerance.  Time and position bit for bit; velocity at the bound of test_gpu_bounce.py (the map
does not touch it); frac relative to the restatement's within 4x the larger of the CPU-measured
spread and the row's own spread.  The spread is what one ulp of atan2 / asin does to
1 - S(lon, lat): an ulp of atan2 moves the impact longitude (atan2 + 2 pi) % 2 pi by up to one
double around 2.5 pi, 8.9e-16, and S by that times the map's slope, relative to 1 - S.  Measured on
the CPU over the random rows of the golden cases 'tempdep' and 'elastic' (STICKMAP_SPREAD;
tests/test_stickmap_cpu.py re-measures it), largest relative change of frac:
    smooth map (36 x 18, slopes below 0.4 / rad, 1 - S >= 0.13)          1.2e-15
    steep map (0.05 -> 0.95 across one 10-degree cell, 1 - S >= 0.05)     8.4e-14
    longitude map (1-D, 24 uneven nodes)                                  3.1e-15
so the bound of a row is 4.8e-15, 3.4e-13 and 1.2e-14 unless its own spread is larger.  check_rows
applies the temperature law's 4 x 1.7e-14 as its floor, which is the wider one for the smooth and
the 1-D map: ``check`` below asserts the map's own bound after it.  (The steep map's figure:
the step is 0.9 across 0.1745 rad, 5.2 / rad, so one double of longitude, 8.9e-16, is 4.6e-15 of
S and 9e-14 of 1 - S at the 0.95 end.)  Seen on the GPU: 1.1e-15, 6e-14 and 2e-15.
"""
import contextlib
import io
import os
import types

import numpy as np
import pytest

from nexoclom_amd import hip_api, surface
from tests import bounce_cases as B
from tests import helpers as H
from tests import stickmap_restatement as SR
from tests import test_gpu_bounce as TB
from tests.test_gpu_bounce import check_rows, libm_rows, single_impact

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLE = os.path.join(os.path.dirname(HERE), 'nexoclom_amd', 'inputfiles', 'Na.mercury.stickmap.input')
STICKMAP_SPREAD = {'smooth': 1.2e-15, 'steep': 8.4e-14, 'longitude': 3.1e-15}     # frac, relative
GOLDEN_CASES = ('tempdep', 'elastic')             # with and without accommodation


@pytest.fixture(scope='module')
def golden():
    return np.load(B.GOLDEN, allow_pickle=False)


@pytest.fixture
def map_law(monkeypatch):
    """bounce_cases.restate knows the map law for the length of the test (libm_rows calls it)."""
    monkeypatch.setattr(B, 'restate', SR.restate)


def golden_map_config(g, name, which):
    taa, accom = float(g[f'{name}_scalars'][0]), float(g[f'{name}_scalars'][1])
    return SR.map_config(taa, accom, SR.MAPS[which](), float(g['GM']), float(g['unit_km']), int(g['seed']))


def stickmap_spread(g, which):
    """Largest relative change of frac under libm_rows over the random rows of the golden cases,
    for map ``which`` (CPU only)."""
    worst = 0.0
    saved, B.restate = B.restate, SR.restate
    try:
        for name in GOLDEN_CASES:
            cfg = golden_map_config(g, name, which)
            rows = libm_rows(g[f'{name}_X'], cfg, g[f'{name}_ids'], g[f'{name}_nb'], g[f'{name}_hit'])
            worst = max(worst, rows[g[f'{name}_edge'] == 0, 2].max())
    finally:
        B.restate = saved
    return worst


def check(got, want, spread, cfg, which, label):
    """check_rows, then frac at the map's own bound; no row is left out."""
    check_rows(got, want, spread, cfg, label)
    tol = 4*np.maximum(spread[:, 2], STICKMAP_SPREAD[which])
    rel = np.divide(np.abs(got[:, 7] - want[:, 7]), want[:, 7], out=np.zeros(len(got)), where=want[:, 7] > 0)
    print(f'{label}: frac max {rel.max():.3g}, worst ratio to its bound {np.max(rel/tol):.3g}, '
          f'smallest bound {tol.min():.3g}, largest {tol.max():.3g}')
    assert np.all(rel <= tol), (label, np.nonzero(rel > tol)[0][:10])


def impacts_against_restatement(ctx, coracle, cfg, which, target, first, label, r0=None, hit=None,
                                min_hits=40):
    entered, rec = single_impact(ctx, coracle, cfg, target, first)
    ids = np.uint64(first) + np.arange(len(target), dtype=np.uint64)
    zero = np.zeros(len(target), dtype=np.int64)
    if r0 is None:
        r0 = np.sqrt((entered[:, 1]**2 + entered[:, 2]**2) + entered[:, 3]**2)
        hit = (r0 - 1.) < 0
    assert hit.sum() >= min_hits and (~hit).sum() >= 8, (label, hit.sum())
    want = TB.after_fate(SR.restate(entered, cfg, ids, zero, hit), r0)
    assert np.array_equal(rec[~hit], entered[~hit])
    check(rec[hit], want[hit], libm_rows(entered, cfg, ids, zero, hit)[hit], cfg, which, label)
    # the map touches frac alone: position and velocity are those of constant sticking, to the bit
    plain = dict(cfg, temp_dependent=0, stickcoef=0.0, stick_map=None)
    _, rec0 = single_impact(ctx, coracle, plain, target, first)
    alive = rec[:, 7] > 0
    assert np.array_equal(rec[alive, :7], rec0[alive, :7]), label
    assert np.array_equal(rec[~alive, 1:7], rec0[~alive, 1:7]), label
    return entered, rec, want, hit


# ---- single impacts ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('which', list(SR.MAPS))
@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_golden_impact_rows(ctx, coracle, golden, map_law, name, which):
    g = golden
    cfg = golden_map_config(g, name, which)
    X, ids, hit = (g[f'{name}_{k}'] for k in ('X', 'ids', 'hit'))
    impacts_against_restatement(ctx, coracle, cfg, which, X, int(ids[0]), f'{name} / {which} map',
                                r0=g[f'{name}_r0'], hit=hit)


def placed_rows(stick_map, unit_km):
    """Radial impacts at chosen (lon, lat): on nodes, around the 2 pi seam and the end longitude
    nodes, beyond the end latitudes, at the sub-solar point; every third row lifted off."""
    lon_n, lat_n, _ = stick_map
    lat_n = np.array([-0.4, 0.0, 0.7]) if lat_n is None else lat_n
    at = [(lo, la) for lo in lon_n[::5] for la in lat_n[1:-1:4]]                     # nodes
    at += [(lo, 0.3) for lo in lon_n] + [(0.8, la) for la in lat_n[1:-1]]
    tiny = (1e-3, 1e-9, 3e-16)
    for la in (-0.9, 0.0, 0.5):                                                      # the seam
        at += [(2*np.pi - e, la) for e in tiny] + [(e, la) for e in tiny]
        at += [(lon_n[-1] + s*e, la) for e in tiny for s in (-1, 1)]
        at += [(max(lon_n[0] + s*e, 0.0), la) for e in tiny for s in (-1, 1)]
    for la in (lat_n[0], lat_n[-1]):                                                 # end latitudes
        edge = np.sign(la)*(np.pi/2 - 1e-3)
        la = np.sign(la)*min(abs(la), abs(edge))
        at += [(lo, v) for lo in (0.4, 2.0, 3.5, 5.9) for v in (la, edge, 0.5*(la + edge),
                                                                    np.sign(la)*(np.pi/2 - 1e-6))]
    at = np.array(at)
    n = len(at) + 9
    X = np.zeros((n, 8))
    lon, lat = at[:, 0], at[:, 1]
    p = np.stack([np.sin(lon)*np.cos(lat), -np.cos(lon)*np.cos(lat), np.sin(lat)], 1)
    v = 1.5/unit_km
    X[:len(at), 1:4] = p*(1 - 1e-4)
    X[:len(at), 4:7] = -p*v
    X[len(at):, 1:4] = [0.0, -(1 - 1e-4), 0.0]                                       # sub-solar,
    X[len(at):, 4:7] = [0.0, v, 0.0]                                                 # longitude exactly 0
    X[:, 0] = 600. + np.arange(n)
    X[:, 7] = np.linspace(0.2, 1.0, n)
    # the lifted rows are copies of their neighbours, so that no chosen point is lost
    return TB.with_bystanders(np.repeat(X, 2, axis=0)[:3*(2*n//3)])


@gpu
@pytest.mark.parametrize('which', list(SR.MAPS))
def test_impacts_on_nodes_seam_end_latitudes_and_subsolar_point(ctx, coracle, golden, map_law, which):
    g = golden
    cfg = golden_map_config(g, 'tempdep', which)
    X = placed_rows(cfg['stick_map'], cfg['unit_km'])
    entered, rec, want, hit = impacts_against_restatement(ctx, coracle, cfg, which, X, 0, f'placed / {which} map',
                                                          min_hits=100)
    lon, lat = SR.impact_point(want[hit])
    L, T, _ = cfg['stick_map']
    assert (lon >= L[-1]).sum() >= 3 and (lon == 0).sum() >= 3
    assert L[0] == 0 or (lon < L[0]).sum() >= 3
    if T is not None and T[-1] < np.pi/2:
        assert (lat < T[0]).sum() >= 3 and (lat > T[-1]).sum() >= 3


# ---- exact cases ------------------------------------------------------------------------------------
def flat_map(value, nlon=12, nlat=7):
    return (np.arange(nlon)*(2*np.pi/nlon), np.linspace(-np.pi/2, np.pi/2, nlat), np.full((nlon, nlat), value))


@gpu
@pytest.mark.parametrize('one_d', [False, True])
def test_maps_of_zeros_and_ones(ctx, coracle, golden, one_d):
    g = golden
    GM, unit_km = float(g['GM']), float(g['unit_km'])
    X = TB.with_bystanders(TB.radial_impacts(150, 31, unit_km))
    const0 = B.config(1.3, 0.2, 0, 0.0, (0., 0., 0.), GM, unit_km, 9)
    entered, rec0 = single_impact(ctx, coracle, const0, X, 0)
    hit = np.sqrt((entered[:, 1]**2 + entered[:, 2]**2) + entered[:, 3]**2) - 1. < 0
    assert hit.sum() >= 90
    for value in (0.0, 1.0):
        lon, lat, coef = flat_map(value)
        stick_map = (lon, None, coef[:, 0]) if one_d else (lon, lat, coef)
        _, rec = single_impact(ctx, coracle, SR.map_config(1.3, 0.2, stick_map, GM, unit_km, 9), X, 0)
        assert np.array_equal(rec[:, 1:7], rec0[:, 1:7])
        assert np.array_equal(rec[~hit], rec0[~hit])
        if value == 0.0:
            assert np.array_equal(rec, rec0)                    # frac and time too: stickcoef = 0
        else:
            assert np.all(rec[hit, 7] == 0) and np.all(rec[hit, 0] == 0)


# ---- cross-check against the temperature law --------------------------------------------------------
@gpu
def test_one_degree_map_of_the_temperature_law(ctx, coracle, golden, map_law):
    """The law tabulated on 1-degree nodes and read back through the map differs from the law
    itself by the interpolation error at each impact point, and by nothing else."""
    g = golden
    name = 'tempdep'
    law_cfg = B.golden_config(g, name)
    inputs = types.SimpleNamespace(geometry=B.geometry(float(g[f'{name}_scalars'][0])),
                                   surfaceinteraction=types.SimpleNamespace(A=tuple(g[f'{name}_A'])))
    smap = surface.sticking_map_from_law(inputs, np.radians(np.arange(360.)), np.radians(np.arange(-90., 91.)))
    map_cfg = SR.map_config(float(g[f'{name}_scalars'][0]), law_cfg['accomfactor'],
                            (smap.longitude, smap.latitude, smap.abundance), law_cfg['GM'],
                            law_cfg['unit_km'], law_cfg['seed'])
    X, ids, hit = (g[f'{name}_{k}'] for k in ('X', 'ids', 'hit'))
    first = int(ids[0])
    zero = np.zeros(len(X), dtype=np.int64)
    entered, rec_law = single_impact(ctx, coracle, law_cfg, X, first)
    entered2, rec_map = single_impact(ctx, coracle, map_cfg, X, first)
    assert np.array_equal(entered, entered2)
    want = SR.restate(entered, map_cfg, ids, zero, hit)
    lon, lat = SR.impact_point(want[hit])
    s_map = map_cfg['surf'].stickcoef(lon, lat)
    s_law = surface.SurfaceInteraction._sticking_law(inputs.geometry, law_cfg['A'])(lon, lat)
    f_in = entered[hit, 7]
    libm = 4*(np.maximum(libm_rows(entered, law_cfg, ids, zero, hit)[hit, 2], TB.LIBM_SPREAD[2])*f_in*(1 - s_law) +
              np.maximum(libm_rows(entered, map_cfg, ids, zero, hit)[hit, 2], 1.7e-14)*f_in*(1 - s_map))
    bound = f_in*np.abs(s_map - s_law) + libm
    # (a packet one law absorbs and the other keeps has frac below 1e-10 on one side: inside f_in |dS|
    # only when both are compared before the threshold, so those rows are compared before it)
    f_law = np.where(rec_law[hit, 7] == 0, f_in*(1 - s_law), rec_law[hit, 7])
    f_map = np.where(rec_map[hit, 7] == 0, f_in*(1 - s_map), rec_map[hit, 7])
    diff = np.abs(f_map - f_law)
    print(f'1-degree map of the law: {hit.sum()} impacts, |S_interp - S_law| max {np.abs(s_map - s_law).max():.3g}, '
          f'frac differs by at most {diff.max():.3g}, worst ratio to the bound '
          f'{np.max(np.divide(diff, bound, out=np.zeros_like(diff), where=bound > 0)):.3g}')
    assert np.all(diff <= bound), np.nonzero(diff > bound)[0][:10]
    assert np.array_equal(rec_map[hit, 1:7], rec_law[hit, 1:7])
    # (next to a terminator the law climbs from 1 to 0.4 within a degree, |cos|^0.25: there the
    # 1-degree map is a third off; elsewhere it is within 1e-4)
    assert np.median(np.abs(s_map - s_law)) < 1e-4 and diff.max() > 0


# ---- every kernel variant that carries BOUNCE -------------------------------------------------------
@pytest.fixture(scope='module')
def stuck(ctx, golden):
    """low_and_slow of test_gpu_bounce.py with the smooth map in place of the temperature law: the
    dense trajectory from the GPU."""
    c = TB.low_and_slow('tempdep', golden)
    taa, accom = B.CASES['tempdep'][:2]
    c['cfg'] = SR.map_config(taa, accom, SR.smooth_map(), c['f'].GM, c['f'].R_km, 41)
    c['dense'] = TB.run_with_bounce(ctx, c, lambda: ctx.integrate_const(
        c['step'], c['n_iter'], c['edge'], nrec=c['nsteps'])['traj'])
    return c


@gpu
def test_trajectory_finals_and_rows_are_the_same_arithmetic(ctx, stuck):
    c = stuck
    dense = c['dense']
    frac = dense[7].T
    live = frac > 0
    work = int(live[:, :-1].sum())                              # a step per live record but the last
    r = np.sqrt(dense[1]**2 + dense[2]**2 + dense[3]**2).T
    impacts = ((np.abs(r[:, 1:] - 1.) < 1e-14) & live[:, 1:]).sum(1)
    assert (impacts >= 3).mean() > 0.2 and impacts.max() >= 5
    # the same packets with constant sticking 0: the map changes frac and nothing else
    plain = dict(c, cfg=dict(c['cfg'], temp_dependent=0, stickcoef=0.0, stick_map=None))
    dense0 = TB.run_with_bounce(ctx, plain, lambda: ctx.integrate_const(
        c['step'], c['n_iter'], c['edge'], nrec=c['nsteps'])['traj'])
    for col in range(7):
        assert np.array_equal(dense[col].T[live], dense0[col].T[live])
    assert (frac[live] < dense0[7].T[live]).sum() > 1000
    fin = TB.run_with_bounce(ctx, c, lambda: ctx.integrate_const(
        c['step'], c['n_iter'], c['edge'], want_final=True, want_steps=True))
    assert ctx.counters()['particle_steps'] == work and ctx.counters()['nonfinite'] == 0
    last = np.minimum(fin['steps'], c['nsteps'] - 1)
    assert np.array_equal(fin['final'], np.transpose(dense, (2, 0, 1))[np.arange(c['n']), :, last])
    wide = TB.run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(c['step'], c['n_iter'], c['edge']))
    assert ctx.counters()['unfinished'] == 0
    assert np.array_equal(wide['lengths'], live.sum(1))
    for col in range(8):
        assert np.array_equal(wide['rows'][col], dense[col].T[live])
    lossfrac = np.zeros_like(frac)
    for ct in range(1, c['nsteps']):
        act = frac[:, ct-1] > 0
        lossfrac[act, ct] = (lossfrac[act, ct-1] + frac[act, ct-1]) - frac[act, ct]
    assert np.array_equal(wide['rows'][8], lossfrac[live])
    narrow = TB.run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(
        c['step'], c['n_iter'], c['edge'], narrow=True))
    assert np.array_equal(narrow['rows'], wide['rows'].astype(np.float32))
    res = TB.run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(
        c['step'], c['n_iter'], c['edge'], resident=True))
    try:
        rows, index = res['store'].download()
        assert np.array_equal(rows, wide['rows'])
        assert np.array_equal(index, np.repeat(np.arange(c['n']), wide['lengths']))
    finally:
        res['store'].free()


@gpu
@pytest.mark.parametrize('quantity', ['radiance', 'column'])
@pytest.mark.parametrize('downcast', [False, True])
def test_fused_image_with_the_map(ctx, stuck, quantity, downcast):
    """k_const_fused<IMAGE = 1 | 2, BOUNCE = true> with law 2: the check of test_gpu_bounce.py
    (counts equal, image to 1e-11 against image_accumulate over the dense live records)."""
    TB.test_fused_image_with_bounce(ctx, stuck, quantity, downcast)


# ---- public API -------------------------------------------------------------------------------------
@gpu
def test_example_input_through_the_public_api(ctx, tmp_path, monkeypatch):
    from nexoclom_amd import Input, ModelImage
    monkeypatch.chdir(tmp_path)
    params = {'quantity': 'column', 'dims': '40,40', 'width': '6,6'}
    kw = dict(npackets=3000, packs_per_it=3000, seed=37, context=ctx)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            lon, lat, coef = SR.smooth_map()
            from nexoclom_amd.sourcemap import SourceMap
            SourceMap(dict(abundance=coef, longitude=lon, latitude=lat)).save('stickmap.npz')
            inputs = Input(EXAMPLE)
            assert inputs.surfaceinteraction.sticktype == 'surface map'
            inputs.run(3000, packs_per_it=3000, seed=37, context=ctx)
            stored = inputs.produce_image(params, context=ctx)
            streamed = ModelImage(inputs, params, **kw)
            kw = dict(kw, packs_per_it=1000, sampler='device')
            whole = ModelImage(inputs, params, **kw)
            shards = [ModelImage(inputs, params, finalize=False, shard=s, **kw)
                      for s in ((0, 1301), (1301, 3000))]
            # and the map does something: the same run with the coefficient halved keeps more
            SourceMap(dict(abundance=0.5*coef, longitude=lon, latitude=lat)).save('stickmap.npz')
            weaker = ModelImage(Input(EXAMPLE), params, **kw)
    finally:
        ctx.set_bounce(None)
        ctx.set_stick_map(None)
    assert stored.packet_image.sum() > 10000
    assert np.array_equal(streamed.packet_image, stored.packet_image)
    np.testing.assert_allclose(streamed.image, stored.image, rtol=1e-11, atol=0)
    assert np.array_equal(sum(s.packet_image for s in shards), whole.packet_image)
    assert weaker.image.sum() > 1.05*whole.image.sum()


# ---- the C ABI --------------------------------------------------------------------------------------
@gpu
def test_map_refusals_state_and_set_up_order(ctx, coracle, golden):
    g = golden
    f = H.mercury_forces('Na', 1.3)
    lon, lat, coef = SR.smooth_map()
    good = SR.map_config(1.3, 0.2, (lon, lat, coef), f.GM, f.R_km, 3)
    bare = {k: v for k, v in good.items() if k != 'stick_map'}

    def changed(a, k, value):
        a = a.copy()
        a[k] = value
        return a

    bad = {
        'nan coefficient': (lon, lat, changed(coef, (3, 4), np.nan)),
        'coefficient above 1': (lon, lat, changed(coef, (0, 0), 1.0000001)),
        'negative coefficient': (lon, lat, changed(coef, (35, 17), -1e-9)),
        'inf coefficient': (lon, None, changed(coef[:, 0], 5, np.inf)),
        'decreasing longitude': (changed(lon, 7, lon[5]), lat, coef),
        'repeated latitude': (lon, changed(lat, 7, lat[6]), coef),
        'longitude 2 pi': (changed(lon, 35, 2*np.pi), lat, coef),
        'negative longitude': (changed(lon, 0, -0.01), lat, coef),
        'latitude beyond the pole': (lon, changed(lat, 17, 1.6), coef),
        'nan node': (changed(lon, 4, np.nan), lat, coef),
        'one longitude node': (lon[:1], lat, coef[:1]),
        'one latitude node': (lon, lat[:1], coef[:, :1]),
    }
    X0 = H.sample_x0(2000, 3, 3000.)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(None)
    ctx.set_stick_map(None)
    try:
        # law 2 and no map: refused at the launch, by every entry that launches; the handle works on
        ctx.set_bounce(bare)
        ctx.upload_packets(X0)
        for call in (lambda: ctx.integrate_const(30., 100, 15., want_final=True),
                     lambda: ctx.integrate_const_rows(30., 100, 15.)):
            with pytest.raises(hip_api.HipError) as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        ctx.set_stick_map(lon, lat, coef)                        # the map after the description
        ctx.upload_packets(X0)
        after = ctx.integrate_const(30., 100, 15., want_final=True)['final']
        # bad maps: refused, and the map that is set stays
        for what, stick_map in bad.items():
            with pytest.raises(hip_api.HipError) as err:
                ctx.set_stick_map(*stick_map)
                pytest.fail(f'{what}: accepted')
            assert err.value.code == hip_api.NXC_ERR_ARG, what
        ctx.upload_packets(X0)
        again = ctx.integrate_const(30., 100, 15., want_final=True)['final']
        assert np.array_equal(again, after)
        # the map before the description; clearing the description keeps the map
        ctx.set_bounce(None)
        ctx.set_stick_map(None)
        ctx.set_stick_map(lon, lat, coef)
        ctx.set_bounce(None)
        ctx.set_bounce(bare)
        ctx.upload_packets(X0)
        before = ctx.integrate_const(30., 100, 15., want_final=True)['final']
        assert np.array_equal(before, after) and np.all(np.isfinite(after))
        # both in one call, as Output does
        ctx.set_stick_map(None)
        ctx.set_bounce(good)
        ctx.upload_packets(X0)
        assert np.array_equal(ctx.integrate_const(30., 100, 15., want_final=True)['final'], after)
        # a map without law 2 is ignored
        const = B.config(*B.CASES['const'], f.GM, f.R_km, 3)
        ctx.set_bounce(const)
        ctx.upload_packets(X0)
        with_map = ctx.integrate_const(30., 100, 15., want_final=True)['final']
        ctx.set_stick_map(None)
        ctx.upload_packets(X0)
        assert np.array_equal(ctx.integrate_const(30., 100, 15., want_final=True)['final'], with_map)
        assert not np.array_equal(with_map, after)
        # set_bounce(None): perfect sticking, bit-equal to the C oracle
        ctx.set_stick_map(lon, lat, coef)
        ctx.set_bounce(None)
        ctx.upload_packets(X0)
        plain = ctx.integrate_const(30., 100, 15., want_final=True, want_steps=True)
        ref = coracle.integrate_const(f, X0, 30., 100, 15., threads=4)
        assert np.array_equal(plain['final'], ref['final']) and np.array_equal(plain['steps'], ref['steps'])
        assert not np.array_equal(plain['final'], after)
    finally:
        ctx.set_bounce(None)
        ctx.set_stick_map(None)
