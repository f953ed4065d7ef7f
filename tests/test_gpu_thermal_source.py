"""Thermal launch speeds on the device (k_sample, speed_type 3) against the NumPy restatement
(tests/thermal_restatement.py), the law (the host sampler's, which defines it), the seeded host
stream (generator='pcg64'), and end to end.

Seeds and sizes of the statistical checks are those of tests/test_thermal_source_cpu.py, where
the host sampler's packets pass the same checks without a GPU."""
import contextlib
import io

import numpy as np
import pytest

from nexoclom_amd import Input, ModelImage, Output, hip_api
from nexoclom_amd.Output import n_output_steps
from nexoclom_amd.source_distribution import spot_density_map, surface_map_cells
from nexoclom_amd.surface import surface_temperature, thermal_launch_spline
from tests import thermal_restatement as R
from tests.test_thermal_source_cpu import (LAW_N, LAW_SEED, THERMAL_INPUT, bare_output, law_checks,
                                           thermal_input)

pytestmark = pytest.mark.gpu
STATE = ['time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac']


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def lon_lat(X, exobase=1.0):
    """Longitude and latitude of launch points given as columns (time, x, y, z, ...)."""
    return np.arctan2(X[1], -X[2]) % (2*np.pi), np.arcsin(np.clip(X[3]/exobase, -1, 1))


def smooth_map():
    """37 x 19 nodes, dayside-heavy, no zeros."""
    longitude = np.linspace(0, 2*np.pi, 37)
    latitude = np.linspace(-np.pi/2, np.pi/2, 19)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    return longitude, latitude, 1.2 + np.cos(lon)*np.cos(lat)


def with_spatial(src, kind):
    src = {k: v for k, v in src.items() if k != 'surface_map'}
    if kind == 'map':
        longitude, latitude, abundance = smooth_map()
        cdf, (lon0, lon1, s0, s1) = surface_map_cells(longitude, latitude, abundance)
        src.update(spatial_type=2, map_nodes=abundance, map_cdf=cdf, map_lon0=lon0, map_lon1=lon1,
                   map_s0=s0, map_s1=s1)
    elif kind == 'spot':
        _, _, density = spot_density_map(0.3, 0.2, 0.4)
        src.update(spatial_type=1, surface_map=density)
    return src


def speed_tolerance(src, seed):
    """4 x the largest relative change of v under 1-ulp moves of cos(lon), cos(lat) and the
    latitude (tests/thermal_restatement.py, speed_ulp_sensitivity), evaluated here on the CPU for
    this test's own packets: 1.66e-14 for the uniform source at seed 77."""
    lon, lat, u = R.launch(LAW_N, seed, **{k: v for k, v in src.items()
                                          if k in ('spatial_type', 'sinlat0', 'sinlat1', 'lon0',
                                                   'lon1', 'map_nodes', 'map_cdf', 'map_lon0',
                                                   'map_lon1', 'map_s0', 'map_s1')})
    return 4*R.speed_ulp_sensitivity(lon, lat, u, src['t0'], src['t1'], src['thermal_spline'])


# ---- 5. the device law, given the uniforms --------------------------------------------------------------
@pytest.mark.parametrize('spatial', ['uniform', 'map'])
@pytest.mark.parametrize('angular_type', [0, 1])
def test_device_thermal_speeds_equal_the_restatement(ctx, spatial, angular_type):
    src = with_spatial(bare_output(Input(THERMAL_INPUT)).source_desc(), spatial)
    src['angular_type'] = angular_type
    tol = speed_tolerance(src, 77)
    print(f'{spatial}, angular_type {angular_type}: speed tolerance {tol:.3e}')
    assert 0 < tol < 1e-12
    for first in (0, 3_000_001):
        X = ctx.sample_packets(LAW_N, 77, first_index=first, download=True, **src)
        ref = R.sample_x0(LAW_N, 77, first, **src).T
        np.testing.assert_allclose(X, ref, rtol=1e-11, atol=1e-14)
        v_dev, v_ref = np.linalg.norm(X[4:7], axis=0), np.linalg.norm(ref[4:7], axis=0)
        assert np.array_equal(v_dev == 0, v_ref == 0)
        live = v_ref > 0
        worst = float(np.max(np.abs(v_dev[live] - v_ref[live])/v_ref[live]))
        print(f'  first_index {first}: largest relative speed difference {worst:.3e}')
        assert worst <= tol


# ---- 6. the device law, statistically -------------------------------------------------------------------
@pytest.mark.parametrize('spatial', ['uniform', 'map', 'spot'])
def test_device_thermal_speeds_follow_the_law(ctx, spatial):
    inputs = Input(THERMAL_INPUT)
    src = with_spatial(bare_output(inputs).source_desc(), spatial)
    assert R.nondecreasing_in_p(thermal_launch_spline(inputs))
    X = ctx.sample_packets(LAW_N, LAW_SEED, download=True, **src)
    lon, lat = lon_lat(X)
    law_checks(inputs, lon, lat, np.linalg.norm(X[4:7], axis=0)*src['unit_km'])


# ---- 7. PCG64 follows the host stream ------------------------------------------------------------------
def test_pcg64_thermal_follows_the_seeded_host_stream(ctx):
    inputs = Input(THERMAL_INPUT)
    n, seed = 20000, 321
    got = ctx.pcg64_uniforms(seed, n, 0, n, 5)
    rng = np.random.default_rng(seed)
    for v in range(5):
        assert np.array_equal(got[v], rng.random(n))
    with quiet():
        host = Output(inputs, n, seed=seed, integrate=False, save=False, context=ctx)
        dev = Output(inputs, n, seed=seed, integrate=False, save=False, context=ctx,
                     sampler='device', generator='pcg64')
        part = Output(inputs, n, seed=seed, integrate=False, save=False, context=ctx,
                      sampler='device', generator='pcg64', window=(n, 777, 15001))
    eps = np.finfo(float).eps
    for c in ('x', 'y', 'z'):
        a, b = dev.X0[c].values, host.X0[c].values
        assert np.abs(a - b).max() <= 4*eps, (c, np.abs(a - b).max()/eps)
    for c in STATE:
        assert np.array_equal(part.X0[c].values, dev.X0[c].values[777:15001]), c
    # speeds: the bound of test 5 plus FITPACK's .ev against the de Boor sum (host, 1e6 points)
    src = bare_output(inputs).source_desc()
    lon, lat, u = R.launch(LAW_N, 77, spatial_type=0)
    tol = 4*R.speed_ulp_sensitivity(lon, lat, u, src['t0'], src['t1'], src['thermal_spline'])
    r = np.random.default_rng(6)
    T, p = 100 + r.random(1000000)*src['t1'], r.random(1000000)
    S = thermal_launch_spline(inputs)
    fit = np.abs(S.ev(T, p) - R.bispev3(*src['thermal_spline'], T, p))
    live = np.abs(S.ev(T, p)) > 1e-3
    bound = tol + float(np.max(fit[live]/np.abs(S.ev(T, p))[live]))
    v_dev = np.linalg.norm(dev.X0[['vx', 'vy', 'vz']].values, axis=1)
    v_host = host.X0.v.values
    keep = v_host > 0
    worst = float(np.max(np.abs(v_dev[keep] - v_host[keep])/v_host[keep]))
    print(f'PCG64: speed bound {bound:.3e}, largest relative difference {worst:.3e}')
    assert worst <= bound
    # the run: host-sampled against device-sampled packets through the streaming image
    params = {'quantity': 'radiance', 'dims': '128,128'}
    kw = dict(npackets=20000, seed=55, packs_per_it=8000, context=ctx)
    with quiet():
        host_img = ModelImage(inputs, params, sampler='numpy', **kw)
        dev_img = ModelImage(inputs, params, sampler='device', generator='pcg64', **kw)
    assert host_img.packet_image.sum() > 1e5
    assert np.array_equal(dev_img.packet_image, host_img.packet_image)
    np.testing.assert_allclose(dev_img.image, host_img.image, rtol=1e-9, atol=0)


def test_bad_thermal_descriptors_raise_and_leave_the_context_usable(ctx):
    good = bare_output(Input(THERMAL_INPUT)).source_desc()
    tx, ty, coef = good['thermal_spline']

    def spline(tx=tx, ty=ty, coef=coef):
        return dict(good, thermal_spline=(tx, ty, coef))

    def changed(a, k, value):
        a = a.copy()
        a[k] = value
        return a

    bad = {
        'nan coefficient': spline(coef=changed(coef, (3, 4), np.nan)),
        'inf coefficient': spline(coef=changed(coef, (0, 0), np.inf)),
        'decreasing tx': spline(tx=changed(tx, 50, tx[49] - 1.0)),
        'repeated interior ty': spline(ty=changed(ty, 50, ty[49])),
        'nan knot': spline(tx=changed(tx, 0, np.nan)),
        'too few knots': spline(tx=tx[:7], coef=coef[:3]),
        'coef of another shape': spline(coef=coef[:, :-1]),
        't0 = 0': dict(good, t0=0.0),
        't1 < 0': dict(good, t1=-1.0),
        'no spline': {k: v for k, v in good.items() if k != 'thermal_spline'},
        'PCG64 with a map': dict(with_spatial(good, 'map'), pcg64=(1000, 0)),
    }
    for what, src in bad.items():
        with pytest.raises((hip_api.HipError, ValueError)):
            ctx.sample_packets(1000, 5, download=True, **src)
            pytest.fail(f'{what}: accepted')
    X = ctx.sample_packets(1000, 5, download=True, **good)
    assert np.all(np.isfinite(X)) and np.all(X[7] == 1.0)
    X = ctx.sample_packets(1000, 5, download=True, pcg64=(1000, 0), **good)
    assert np.all(np.isfinite(X))


# ---- 8. end to end ----------------------------------------------------------------------------------
def test_thermal_runs_end_to_end(ctx, tmp_path):
    inputs = Input(THERMAL_INPUT)
    params = {'quantity': 'radiance', 'dims': '64,64'}
    with quiet():
        inputs.run(200000, seed=3, context=ctx, sampler='device')
        image = inputs.produce_image(params, context=ctx)
    assert image.packet_image.sum() > 1e5 and np.all(np.isfinite(image.image))
    variable = thermal_input(tmp_path, 'options.step_size = 0\noptions.resolution = 1e-4')
    with quiet():
        out = Output(variable, 20000, seed=4, context=ctx, sampler='device', save=False)
    assert len(out.X) > 0 and np.all(np.isfinite(out.X[STATE].values))
    # three shards of the streaming image sum to the whole
    kw = dict(npackets=30000, seed=12, packs_per_it=10000, context=ctx, sampler='device')
    with quiet():
        whole = ModelImage(inputs, params, **kw)
        shards = [ModelImage(inputs, params, finalize=False, shard=s, **kw)
                  for s in ((0, 7001), (7001, 21000), (21000, 30000))]
    assert np.array_equal(sum(s.packet_image for s in shards), whole.packet_image)


def test_no_night_side_packet_escapes(ctx):
    inputs = Input(THERMAL_INPUT)
    S = thermal_launch_spline(inputs)
    night_max = float(np.max(S.ev(np.full(10001, R.NIGHT_K), np.linspace(0, 1, 10001))))
    assert night_max < 0.82               # 3 v_th at 100 K, far below the 4.25 km/s escape speed
    n = 100000
    with quiet():
        out = Output(inputs, n, seed=9, integrate=False, save=False, context=ctx,
                     sampler='device')
    X0 = out.X0[STATE].values.T
    lon, lat = lon_lat(X0, inputs.spatialdist.exobase)
    night = surface_temperature(inputs.geometry, lon, lat) == R.NIGHT_K
    assert 0.3 < night.mean() < 0.7
    ctx.set_forces(**out.forces_kwargs())
    ctx.set_bounce(None)
    step = inputs.options.step_size
    _, n_iter = n_output_steps(inputs.options.endtime.value, step)
    outeredge = inputs.options.outeredge
    final = ctx.integrate_const(step, n_iter, outeredge, want_final=True)['final']
    r = np.linalg.norm(final[:, 1:4], axis=1)
    print(f'night-side launches: {night.sum()}, of them beyond the outer edge: '
          f'{(r[night] > outeredge).sum()}; all packets beyond it: {(r > outeredge).sum()}')
    assert not np.any(r[night] > outeredge)
