"""LOSResult.make_source_map on the device against the NumPy restatement of make_source_map.py and
LOSResult.py:338-447 (tests/sourcemap_restatement.py): hand-made packets at the edges of every
rule, end to end from Input.run (resident, fitted and restored Outputs), and one full-size run.

Counts (n_total, n_included, unweighted bins) must be exact; weighted sums agree to 1e-12
relative (LDS sums in no fixed order), NaN equal to NaN.  The kernel's fp64 sin / cos need not
match NumPy's to the last bit, so the hand-made fixture drops every packet whose haversine value
lies within 1e-12 (relative) of some grid point's threshold."""
import contextlib
import io
import os

import numpy as np
import pandas as pd
import pytest

import nexoclom_amd
from nexoclom_amd import Input, LOSResult, LOSResultFitted, Output, SourceMap, SpacecraftData
from tests import sourcemap_restatement as R

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
R_KM = 2439.7
SMALL = dict(nlonbins=24, nlatbins=13, nvelbins=7, naltbins=5, nazbins=6,
             smear_radius=np.radians(20))
EXACT = ('n_total', 'n_included')
KEYS = ('abundance', 'abundance_uncor', 'fraction_observed', 'speed_dist', 'speed_dist_map',
        'altitude_dist', 'altitude_dist_map', 'azimuth_dist', 'azimuth_dist_map', 'altitude',
        'azimuth', 'speed', 'longitude', 'latitude') + EXACT


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def away_from_thresholds(lat, lon, p):
    """Packets whose haversine value is not within 1e-12 (relative) of any point's threshold."""
    glon, glat = R.grid_points(p)
    keep = np.ones(len(lat), dtype=bool)
    for phi in glat:
        thr = np.sin(0.5*p['smear_radius']*np.cos(phi))**2
        h = R.haversine(phi, glon[:, None], lat[None, :], lon[None, :])
        keep &= ~(np.abs(h - thr) <= 1e-12*thr).any(axis=0)
    return keep


def edge_outputs(grid_params, seed=0):
    """Three Outputs of hand-made packets: longitudes at 0 and 2 pi, latitudes within 1e-6 of
    +-pi/2, altitude pi/2 and azimuth 2 pi exactly, v*R = vmax exactly, frac = 0 packets; a
    fourth Output whose every frac is 0 and a fifth with no packet."""
    p = R.params(grid_params)
    rng = np.random.default_rng(seed)
    outs = []
    for k, n in enumerate((3000, 2500, 2000, 400)):
        lat = np.arcsin(rng.uniform(-1, 1, n))
        lon = rng.uniform(0, 2*np.pi, n)
        v = rng.uniform(0, (3.0 + k)/R_KM, n)
        alt = rng.uniform(0, np.pi/2, n)
        az = rng.uniform(0, 2*np.pi, n)
        frac = rng.uniform(0, 1, n)
        frac[rng.random(n) < 0.2] = 0
        lon[:6] = [0, 2*np.pi, 0, 2*np.pi, 1e-12, 2*np.pi - 1e-12]
        lat[:6] = [np.pi/2 - 1e-7, -np.pi/2 + 5e-7, np.pi/2 - 9e-7, -np.pi/2 + 1e-7, 0.3, -0.3]
        alt[6:9] = np.pi/2
        az[9:12] = 2*np.pi
        vmax = np.ceil(v.max()*R_KM)
        v[12] = vmax/R_KM                      # v*R lands on (or next to) the right edge
        frac[12] = 0.5
        if k == 3:
            frac[:] = 0
        keep = away_from_thresholds(lat, lon, p)
        outs.append(dict(longitude=lon[keep], latitude=lat[keep], v=v[keep], altitude=alt[keep],
                         azimuth=az[keep], frac=frac[keep]))
    outs.append({c: np.zeros(0) for c in outs[0]})
    return outs


class Run:
    def __init__(self, X0):
        self.X0 = pd.DataFrame(X0)


def result_over(ctx, outs, sourcerate=1.7):
    res = LOSResult.__new__(LOSResult)
    res.inputs = type('Inputs', (), {})()
    res.inputs._catalogue = [Run(X0) for X0 in outs]
    res.unit_km, res.sourcerate, res._ctx = R_KM, sourcerate, ctx
    return res


def check(got, want):
    for key in KEYS:
        g, w = np.asarray(getattr(got, key)), np.asarray(want[key])
        if key in EXACT:
            assert np.array_equal(g, w), key
        else:
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, equal_nan=True, err_msg=key)


@pytest.mark.parametrize('grid', ['small', 'default'])
@pytest.mark.parametrize('smear', [True, False])
def test_edge_packets_against_restatement(ctx, grid, smear):
    gp = dict(SMALL if grid == 'small' else {}, smear_abundance=smear)
    outs = edge_outputs(gp)
    res = result_over(ctx, outs)
    for normalize in (False, True):
        with quiet():
            source, available = res.make_source_map(gp, normalize=normalize)
        assert isinstance(source, SourceMap) and isinstance(available, SourceMap)
        for todo, got in (('source', source), ('available', available)):
            want = R.source_map(outs, R_KM, gp, todo, normalize, 1.7)
            check(got, want)
            if not normalize and todo == 'available':
                # unweighted, factor-1 histograms are counts
                assert np.array_equal(got.altitude_dist_map, want['altitude_dist_map'])
                assert np.array_equal(got.azimuth_dist_map, want['azimuth_dist_map'])
    assert source.n_total.sum() > 0 and (source.n_included < source.n_total).any()


def test_only_one_map_and_device_sampled_outputs(ctx):
    outs = edge_outputs(SMALL)
    res = result_over(ctx, outs)
    with quiet():
        source, available = res.make_source_map(SMALL, do_available=False)
    assert available is None and source is not None
    res.inputs._catalogue.append(Run({'x': [1.0], 'frac': [1.0]}))
    with pytest.raises(NotImplementedError, match="sampler='numpy'"):
        res.make_source_map(SMALL)


def run_inputs(ctx, n, size, seed, savepath=None):
    inputs = Input(INPUT, savepath=savepath)
    inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
    with quiet():
        inputs.run(n, packs_per_it=size, seed=seed, context=ctx)
        inputs.wait()
    return inputs


def x0_of(catalogue):
    out = []
    for run in catalogue:
        X0 = Output.upcast(run.X0)
        out.append({c: X0[c].values.astype(np.float64)
                    for c in ('longitude', 'latitude', 'v', 'altitude', 'azimuth', 'frac')})
    return out


def spacecraft(nspec, seed, **columns):
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2*np.pi, nspec, endpoint=False)
    r = 1.6 + 1.2*rng.random(nspec)
    pos = np.stack([0.3*r*np.cos(th), r*np.sin(th)*0.6 - 0.4, r*np.sin(th)*0.8], 1)
    look = -pos + 0.6*rng.normal(size=pos.shape)
    look /= np.linalg.norm(look, axis=1)[:, None]
    return SpacecraftData(*pos.T, *look.T, **columns)


def check_result(res, gp):
    with quiet():
        source, available = res.make_source_map(gp)
    outs = x0_of(res.inputs._catalogue)
    check(source, R.source_map(outs, res.unit_km, gp, 'source', True, float(res.sourcerate)))
    check(available, R.source_map(outs, res.unit_km, gp, 'available', True,
                                  float(res.sourcerate)))
    return source


@pytest.mark.parametrize('where', ['resident', 'restored'])
def test_end_to_end_unfitted_and_fitted(ctx, tmp_path, where):
    inputs = run_inputs(ctx, 30000, 8000, seed=5, savepath=str(tmp_path))
    if where == 'restored':
        restored = Input(INPUT)
        restored.options.endtime = inputs.options.endtime
        for k, f in enumerate(inputs.search()[1]):
            back = Output.restore(f)
            back.idnum = k + 1
            restored._catalogue.append(back)
        inputs = restored
    assert len(inputs._catalogue) >= 3
    sc0 = spacecraft(120, 3)
    probe = LOSResult(sc0, inputs, dphi=np.radians(3.0), context=ctx)
    with quiet():
        probe.simulate_data_from_inputs(sc0)
    rng = np.random.default_rng(8)
    radiance = probe.radiance.values*rng.uniform(0.5, 1.5, 120)
    sc = spacecraft(120, 3, radiance=radiance, sigma=0.05*np.abs(radiance) + 0.01)
    los = LOSResult(sc, inputs, dphi=np.radians(3.0), context=ctx, label='unfit')
    with quiet():
        los.simulate_data_from_inputs(sc)
    los.determine_source_rate(sc, use_weight=False)
    sc.add_model_result(los, 'unfit')
    gp = dict(nlonbins=60, nlatbins=30, nvelbins=40)
    unfit_map = check_result(los, gp)
    fitted = LOSResultFitted(sc, 'unfit', dphi=np.radians(2.0), context=ctx)
    with quiet():
        fitted.determine_source_from_data(sc, use_weight='dist')
    fitted_map = check_result(fitted, gp)
    # the multipliers reach the map
    assert not np.allclose(np.nan_to_num(fitted_map.abundance_uncor),
                           np.nan_to_num(unfit_map.abundance_uncor))


def test_full_size_default_grid(ctx):
    inputs = Input(INPUT)
    with quiet():
        inputs.run(1e6, seed=77, context=ctx)
    res = LOSResult.__new__(LOSResult)
    res.inputs, res.sourcerate, res._ctx = inputs, 1.0, ctx
    res.unit_km = inputs.geometry.planet.radius.value
    with quiet():
        source, _ = res.make_source_map(do_available=False)
    outs = x0_of(inputs._catalogue)
    check(source, R.source_map(outs, res.unit_km, None, 'source', True, 1.0))
    assert source.n_total.sum() > 1e6
