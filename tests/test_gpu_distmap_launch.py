"""Launching speeds and directions from a source map's per-point laws on the device (k_sample's
NXC_LAW_NODES instantiation: speed_type 4, angular_type 2) against the NumPy restatement
(tests/distmap_launch_restatement.py) and the analytic law, and end to end: run -> make_source_map
-> save -> inputfile with all three map types -> run / image.

Maps, seed and sizes of the statistical checks are those of tests/test_distmap_launch_cpu.py, where
the restatement passes them without a GPU."""
import contextlib
import io

import numpy as np
import pytest
from scipy import stats

from nexoclom_amd import Input, LOSResult, ModelImage, Output, SourceMap, hip_api
from nexoclom_amd.source_distribution import node_law_tables, surface_map_cells
from tests import distmap_launch_restatement as R
from tests.test_distmap_launch_cpu import (coded, coded_grids, descriptor, distmap_input,  # noqa: F401
                                           marginal_p_values, save_map, smooth)
from tests.test_gpu_sourcemap import SMALL
from tests.test_sourcemap_launch_cpu import BENCH_INPUT, LAW_N, LAW_SEED, P_MIN, bare_output
from tests.test_thermal_source_cpu import THERMAL_INPUT

pytestmark = pytest.mark.gpu
STATE = ['time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac']
NODE_KEYS = {'speeds': ('node_speed_table',),
             'angles': ('node_altitude_table', 'node_azimuth_table'),
             'both': ('node_speed_table', 'node_altitude_table', 'node_azimuth_table')}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def lon_s(X, exobase=1.0):
    return np.arctan2(X[1], -X[2]) % (2*np.pi), X[3]/exobase


def mode_of(src, mode):
    """``src`` (all three per-point laws) with only the speeds or only the directions from the
    map; the other comes from the bench input (flat speeds / isotropic directions)."""
    base = bare_output(Input(BENCH_INPUT)).source_desc()
    out = {k: v for k, v in src.items() if not k.startswith('node_')}
    out.update({k: src[k] for k in NODE_KEYS[mode]})
    if mode == 'speeds':
        out.update(angular_type=1)
    if mode == 'angles':
        out.update(speed_type=0, vprob=base['vprob'], vwidth=base['vwidth'])
    return out


# ---- parity with the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['speeds', 'angles', 'both'])
@pytest.mark.parametrize('which', ['coded', 'smooth'])
def test_device_equals_the_restatement(ctx, coded, smooth, which, mode):     # noqa: F811
    src = mode_of(coded[2] if which == 'coded' else smooth[2], mode)
    n = 100000
    X = ctx.sample_packets(n, 31, download=True, **src)
    ref = R.draw(n, 31, **src)['X']
    np.testing.assert_allclose(X.T, ref, rtol=1e-11, atol=1e-14)


def test_packets_are_counter_addressed(ctx, coded):                          # noqa: F811
    src = coded[2]
    a = ctx.sample_packets(700, 31, first_index=0, download=True, **src)
    b = ctx.sample_packets(300, 31, first_index=700, download=True, **src)
    c = ctx.sample_packets(1000, 31, first_index=0, download=True, **src)
    assert np.array_equal(np.concatenate([a, b], axis=1), c)


# ---- the law on device output --------------------------------------------------------------------------
def test_device_corner_choice_follows_the_node_law(ctx, coded):              # noqa: F811
    content, code, src = coded
    X = ctx.sample_packets(LAW_N, LAW_SEED, download=True, **src)
    speed, altitude, azimuth = R.launch_angles(X)
    decoded = R.decode_nodes(code, *coded_grids(src), speed*src['unit_km'], altitude, azimuth)
    assert np.all(decoded >= 0), 'a packet whose three draws belong to no single node'
    assert np.all(content['abundance'].ravel()[decoded] > 0)
    assert np.array_equal(decoded, R.draw(LAW_N, LAW_SEED, **src)['node'])
    p_nodes = R.node_goodness_of_fit(decoded, content['abundance'])
    print(f'device, coded map: nodes p={p_nodes:.4f}')
    assert p_nodes > P_MIN


def test_device_draw_follows_the_mixture_laws(ctx, smooth):                  # noqa: F811
    content, _, src = smooth
    X = ctx.sample_packets(LAW_N, LAW_SEED, download=True, **src)
    speed, altitude, azimuth = R.launch_angles(X)
    p = marginal_p_values(content, src, speed*src['unit_km'], altitude, azimuth)
    print('device, smooth map: KS speed p=%.4f altitude p=%.4f azimuth p=%.4f' % tuple(p))
    assert min(p) > P_MIN
    lon, s = lon_s(X, src['exobase'])
    limits = tuple(src[k] for k in ('map_lon0', 'map_lon1', 'map_s0', 'map_s1'))
    assert R.S.cell_goodness_of_fit(lon, s, content['abundance'], limits) > P_MIN


# ---- nodes without abundance ---------------------------------------------------------------------------
def peaked_map():
    """tests/test_gpu_sourcemap_launch.py's: 181 x 91 nodes, one sharp peak, 99 % of the cells
    without mass."""
    longitude = np.linspace(0, 2*np.pi, 181)
    latitude = np.linspace(-np.pi/2, np.pi/2, 91)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    abundance = np.exp(-0.5*(((lon - 2.0)/0.05)**2 + ((lat - 0.4)/0.05)**2))
    abundance[np.abs(lon - 2.0) > 0.17] = 0.0
    abundance[np.abs(lat - 0.4) > 0.17] = 0.0
    return longitude, latitude, abundance


def test_no_packet_from_a_node_without_abundance(ctx, tmp_path):
    """Nodes without abundance carry NaN rows in the file and the placeholder on the device,
    whose inversion gives the LAST grid value; the laws of the nodes with abundance leave the
    last bin empty, so a packet from a node without abundance would show."""
    longitude, latitude, abundance = peaked_map()
    live = abundance > 0
    assert live.mean() < 0.01
    laws = {}
    for name, n in (('speed_dist_map', 7), ('altitude_dist_map', 5), ('azimuth_dist_map', 6)):
        rows = np.full(abundance.shape + (n,), np.nan)
        rows[live] = np.r_[np.arange(1.0, n), 0.0]
        laws[name] = rows
    content = dict(longitude=longitude, latitude=latitude, abundance=abundance,
                   speed=np.linspace(0.5, 3.5, 7), **laws)
    src = descriptor(tmp_path, content)
    n = 1000000
    X = ctx.sample_packets(n, 606, download=True, **src)
    assert np.all(np.isfinite(X))
    speed, altitude, azimuth = R.launch_angles(X)
    for key, sample in (('node_speed_table', speed*src['unit_km']),
                        ('node_altitude_table', altitude), ('node_azimuth_table', azimuth)):
        grid = src[key][1]
        assert sample.max() <= grid[-2]*(1 + 1e-12), key
        assert sample.min() >= grid[0]*(1 - 1e-9), key
    ref = R.draw(20000, 606, **src)
    assert np.all(abundance.ravel()[ref['node']] > 0)
    np.testing.assert_allclose(X[:, :20000].T, ref['X'], rtol=1e-11, atol=1e-14)


# ---- bad descriptors ------------------------------------------------------------------------------------
def test_bad_descriptors_raise_and_leave_the_context_usable(ctx, coded):      # noqa: F811
    content, _, good = coded
    base = bare_output(Input(BENCH_INPUT)).source_desc()
    live = int(np.flatnonzero(content['abundance'].ravel() > 0)[5])

    def with_row(key, change):
        cdf, grid = good[key]
        cdf = cdf.copy()
        change(cdf[live])
        return dict(good, **{key: (cdf, grid)})

    def decreasing(row):
        row[-2] = 1.5

    def short(row):
        row *= 0.5

    def nan(row):
        row[1] = np.nan

    def zeros(row):
        row[:] = 0.0

    uniform = {k: v for k, v in good.items() if not k.startswith('map_')}
    bad = {}
    for key in NODE_KEYS['both']:
        bad[f'{key}: decreasing row'] = with_row(key, decreasing)
        bad[f'{key}: row that does not reach 1'] = with_row(key, short)
        bad[f'{key}: NaN in a row'] = with_row(key, nan)
        bad[f'{key}: placeholder at a node with abundance'] = with_row(key, zeros)
        cdf, grid = good[key]
        bad[f'{key}: one row too few'] = dict(good, **{key: (cdf[:-1], grid)})
        bad[f'{key}: axis of another length'] = dict(good, **{key: (cdf, grid[:-1])})
        bad[f'{key}: one entry per row'] = dict(good, **{key: (cdf[:, :1], grid[:1])})
        bad[f'{key}: infinite axis'] = dict(good, **{key: (cdf, np.r_[grid[:-1], np.inf])})
    bad['tables without a map'] = dict(uniform, spatial_type=0)
    bad['tables with spatial_type 0'] = dict(good, spatial_type=0)
    bad['speed_type 4 without its table'] = {k: v for k, v in good.items()
                                             if k != 'node_speed_table'}
    bad['angular_type 2 without its tables'] = {k: v for k, v in good.items()
                                                if k not in NODE_KEYS['angles']}
    bad['PCG64 stream'] = dict(good, pcg64=(1000, 0))
    # thermal speeds with per-node directions: no instantiation of k_sample holds both laws
    thermal = bare_output(Input(THERMAL_INPUT)).source_desc()
    bad['thermal speeds with per-node directions'] = dict(
        {k: v for k, v in good.items() if k != 'node_speed_table'}, speed_type=3,
        **{k: thermal[k] for k in ('t0', 't1', 'thermal_spline')})
    for what, src in bad.items():
        with pytest.raises((hip_api.HipError, ValueError)):
            ctx.sample_packets(1000, 5, download=True, **src)
            pytest.fail(f'{what}: accepted')
    # what nxc_packets_sample itself refuses, by its message
    by_the_library = {
        'node_speed_table: decreasing row': 'node_speed_cdf: row of node',
        'node_altitude_table: row that does not reach 1': 'node_alt_cdf: row of node',
        'node_azimuth_table: NaN in a row': 'node_az_cdf: row of node',
        'node_speed_table: placeholder at a node with abundance': 'node_speed_cdf: row of node',
        'node_azimuth_table: one entry per row': 'node_az needs 2..65536 entries',
        'node_altitude_table: infinite axis': 'node_alt: axis must be finite',
        'tables with spatial_type 0': 'spatial_type 2',
        'speed_type 4 without its table': 'node_speed needs 2..65536 entries',
        'angular_type 2 without its tables': 'node_alt needs 2..65536 entries',
        'PCG64 stream': 'PCG64',
        'thermal speeds with per-node directions': r'thermal speeds \(speed_type 3\) with per-node',
    }
    for what, message in by_the_library.items():
        with pytest.raises(hip_api.HipError, match=message):
            ctx.sample_packets(1000, 5, **bad[what])
    X = ctx.sample_packets(1000, 5, download=True, **good)
    assert np.all(np.isfinite(X))
    np.testing.assert_allclose(X.T, R.draw(1000, 5, **good)['X'], rtol=1e-11, atol=1e-14)
    X = ctx.sample_packets(1000, 5, download=True, **base)
    assert np.all(np.isfinite(X)) and np.all(X[7] == 1.0)


def test_pcg64_generator_is_refused_by_the_output(ctx, coded, tmp_path):     # noqa: F811
    inputs = distmap_input(tmp_path, save_map(tmp_path, coded[0]))
    with pytest.raises(hip_api.HipError), quiet():
        Output(inputs, 1000, seed=3, integrate=False, save=False, context=ctx, sampler='device',
               generator='pcg64')


# ---- closing the loop -----------------------------------------------------------------------------------
def test_run_to_map_to_file_to_run_with_per_point_laws(ctx, tmp_path):
    first = Input(BENCH_INPUT)
    first.options.endtime = type(first.options.endtime)(6000., 's')
    with quiet():
        first.run(300000, seed=17, context=ctx)              # host sampler: X0 kept
    res = LOSResult.__new__(LOSResult)
    res.inputs, res.sourcerate, res._ctx = first, 1.0, ctx
    res.unit_km = first.geometry.planet.radius.value
    with quiet():
        source, _ = res.make_source_map(SMALL, normalize=True, do_available=False)
    path = str(tmp_path / 'fitted_map.npz')
    source.save(path)
    back = SourceMap(path)
    assert back.speed_dist_map.shape == back.abundance.shape + (SMALL['nvelbins'],)

    inputs = distmap_input(tmp_path, path)
    n = 400000
    with quiet():
        out = Output(inputs, n, seed=23, integrate=False, save=False, context=ctx,
                     sampler='device')
    src = out.source_desc()
    assert (src['spatial_type'], src['speed_type'], src['angular_type']) == (2, 4, 2)
    X = out.X0[STATE].values.T
    lon, s = lon_s(X, inputs.spatialdist.exobase)
    _, limits = surface_map_cells(back.longitude, back.latitude, back.abundance)
    p_cells = R.S.cell_goodness_of_fit(lon, s, back.abundance, limits)
    speed, altitude, azimuth = R.launch_angles(X)
    tables = {law: node_law_tables(inputs.spatialdist, law)
              for law in ('speed', 'altitude', 'azimuth')}
    p = [stats.kstest(sample, R.mixture_cdf(back.abundance, tables[law])).pvalue
         for law, sample in (('speed', speed*out.unit_km), ('altitude', altitude),
                             ('azimuth', azimuth))]
    print('loop: cells p=%.4f KS speed p=%.4f altitude p=%.4f azimuth p=%.4f'
          % ((p_cells,) + tuple(p)))
    assert p_cells > P_MIN and min(p) > P_MIN

    # Input.run and the streaming image draw the same packets from the map and its laws
    params = {'quantity': 'radiance', 'dims': '64,64'}
    with quiet():
        inputs.run(200000, packs_per_it=100000, seed=29, context=ctx, sampler='device')
        two_stage = inputs.produce_image(params, context=ctx)
        streaming = ModelImage(inputs, params, npackets=200000, packs_per_it=100000, seed=29,
                               context=ctx, sampler='device')
    assert [len(o) for o in inputs._catalogue] == [100000, 100000]
    assert two_stage.totalsource == streaming.totalsource
    assert streaming.packet_image.sum() > 1e5
    np.testing.assert_allclose(two_stage.packet_image, streaming.packet_image, rtol=1e-11)
    np.testing.assert_allclose(two_stage.image, streaming.image, rtol=1e-11)
