"""Launching packets from a source map on the device (k_sample, spatial_type 2 / 3; user-defined
speeds as speed_type 2) against the NumPy restatement (tests/sourcemap_launch_restatement.py) and
the law it restates, and end to end: run -> make_source_map -> save -> inputfile -> run / image.

Seeds and sizes of the statistical checks are those of tests/test_sourcemap_launch_cpu.py, where
the restatement passes them without a GPU."""
import contextlib
import io
import os

import numpy as np
import pytest
from scipy import stats

from nexoclom_amd import Input, LOSResult, ModelImage, Output, SourceMap, hip_api
from nexoclom_amd.source_distribution import density_cdf, surface_map_cells
from tests import sourcemap_launch_restatement as R
from tests.test_gpu_sourcemap import SMALL
from tests.test_sourcemap_launch_cpu import (BENCH_INPUT, LAW_N, LAW_SEED, P_MIN, bare_output,
                                             golden, golden_map, map_input)    # noqa: F401

pytestmark = pytest.mark.gpu
STATE = ['time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac']


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def lon_s(X, exobase=1.0):
    """Longitude and sin(latitude) of launch points given as rows (.., x, y, z, ..) of STATE."""
    return np.arctan2(X[1], -X[2]) % (2*np.pi), X[3]/exobase


def peaked_map():
    """181 x 91 nodes, one sharp peak, 99 % of the cells without mass: what rejection is worst at
    (mean / max of the nodes = 8e-4)."""
    longitude = np.linspace(0, 2*np.pi, 181)
    latitude = np.linspace(-np.pi/2, np.pi/2, 91)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    abundance = np.exp(-0.5*(((lon - 2.0)/0.05)**2 + ((lat - 0.4)/0.05)**2))
    abundance[np.abs(lon - 2.0) > 0.17] = 0.0
    abundance[np.abs(lat - 0.4) > 0.17] = 0.0
    return longitude, latitude, abundance


def map_source(base, longitude, latitude, abundance):
    """``base`` (the descriptor of some other source) with its launch points taken from a map."""
    cdf, limits = surface_map_cells(longitude, latitude, abundance)
    src = {k: v for k, v in base.items() if k != 'surface_map'}
    src.update(spatial_type=2, map_nodes=abundance, map_cdf=cdf, map_lon0=limits[0],
               map_lon1=limits[1], map_s0=limits[2], map_s1=limits[3])
    return src, limits


# ---- 7. parity with the restatement ------------------------------------------------------------------
@pytest.mark.parametrize('one_d', [False, True])
def test_map_source_equals_the_restatement_and_is_counter_addressed(ctx, golden, tmp_path,   # noqa: F811
                                                                    one_d):
    path = golden_map(golden, tmp_path, one_d=one_d)
    inputs = map_input(tmp_path, mapfile=path, vdistfile=path)
    n = 100000
    with quiet():
        out = Output(inputs, n, seed=31, integrate=False, save=False, context=ctx,
                     sampler='device')
    src = out.source_desc()
    assert src['spatial_type'] == (3 if one_d else 2) and src['speed_type'] == 2
    X = out.X0[STATE].values
    ref = R.sample_x0(n, 31, **src)
    np.testing.assert_allclose(X, ref, rtol=1e-11, atol=1e-14)
    if one_d:
        assert np.all(X[:, 3] == 0)
    a = ctx.sample_packets(700, 31, first_index=0, download=True, **src)
    b = ctx.sample_packets(300, 31, first_index=700, download=True, **src)
    c = ctx.sample_packets(1000, 31, first_index=0, download=True, **src)
    assert np.array_equal(np.concatenate([a, b], axis=1), c)
    assert np.array_equal(c, X[:1000].T)
    # the device against the reference's deviates, at the restatement's seed and size
    big = ctx.sample_packets(LAW_N, LAW_SEED, download=True, **src)
    lon, s = lon_s(big, src['exobase'])
    p_lon = stats.ks_2samp(lon, golden['lon_1d' if one_d else 'lon_2d']).pvalue
    speed = np.linalg.norm(big[4:7], axis=0)*src['unit_km']
    p_speed = stats.ks_2samp(speed, golden['speed_2d']).pvalue
    print(f'one_d={one_d}: KS lon p={p_lon:.4f} speed p={p_speed:.4f}')
    assert p_lon > P_MIN and p_speed > P_MIN
    if not one_d:
        limits = tuple(src[k] for k in ('map_lon0', 'map_lon1', 'map_s0', 'map_s1'))
        p_s = stats.ks_2samp(s, golden['s_2d']).pvalue
        p_cells = R.cell_goodness_of_fit(lon, s, golden['abundance'], limits)
        print(f'KS s p={p_s:.4f} cells p={p_cells:.4f}')
        assert p_s > P_MIN and p_cells > P_MIN


# ---- 8. the map rejection is worst at ----------------------------------------------------------------
def test_sharp_peak_on_an_empty_map(ctx):
    longitude, latitude, abundance = peaked_map()
    prob = R.cell_probabilities(abundance)
    assert (prob == 0).mean() > 0.99
    base = bare_output(Input(BENCH_INPUT)).source_desc()
    src, limits = map_source(base, longitude, latitude, abundance)
    n = 1000000
    X = ctx.sample_packets(n, 606, download=True, **src)
    assert np.all(np.isfinite(X))
    np.testing.assert_allclose(np.linalg.norm(X[1:4], axis=0), 1.0, rtol=1e-14)
    lon, s = lon_s(X)
    # inside the closure of a cell with mass: the cell of the point itself, or -- for a point that
    # rounding put onto a cell's edge -- of a point 1e-9 cells away
    gx = (lon - limits[0])/((limits[1] - limits[0])/180)
    gy = (s - limits[2])/((limits[3] - limits[2])/90)
    inside = np.zeros(n, dtype=bool)
    for dx in (-1e-9, 1e-9):
        for dy in (-1e-9, 1e-9):
            i = np.clip(np.floor(gx + dx).astype(int), 0, 179)
            j = np.clip(np.floor(gy + dy).astype(int), 0, 89)
            inside |= prob[i, j] > 0
    assert inside.all(), f'{(~inside).sum()} launch points in cells without mass'
    p_cells = R.cell_goodness_of_fit(lon, s, abundance, limits)
    print(f'peaked map: cells p={p_cells:.4f}')
    assert p_cells > P_MIN
    ref = R.sample_x0(20000, 606, **src)
    np.testing.assert_allclose(X[:, :20000].T, ref, rtol=1e-11, atol=1e-14)


# ---- 9. bad descriptors ------------------------------------------------------------------------------
def test_bad_map_descriptors_raise_and_leave_the_context_usable(ctx, golden):   # noqa: F811
    base = bare_output(Input(BENCH_INPUT)).source_desc()
    good, _ = map_source(base, golden['longitude'], golden['latitude'], golden['abundance'])

    def changed(**changes):
        src = dict(good)
        src.update(changes)
        return src

    def with_node(value):
        nodes = golden['abundance'].copy()
        nodes[3, 4] = value
        return changed(map_nodes=nodes)

    decreasing = good['map_cdf'].copy()
    decreasing[100] = decreasing[99] - 1e-3
    short = good['map_cdf'].copy()
    short[-1] = 0.5
    grid_cdf, grid = density_cdf(golden['longitude'], golden['abundance_1d'])
    one_d = {k: v for k, v in good.items() if not k.startswith('map_')}
    bad = {
        'nan node': with_node(np.nan), 'inf node': with_node(np.inf),
        'negative node': with_node(-0.5),
        'all-zero map': changed(map_nodes=np.zeros_like(golden['abundance'])),
        'one longitude': changed(map_nodes=golden['abundance'][:1], map_cdf=np.empty(0)),
        'one latitude': changed(map_nodes=golden['abundance'][:, :1], map_cdf=np.empty(0)),
        'decreasing cdf': changed(map_cdf=decreasing),
        'cdf that does not reach 1': changed(map_cdf=short),
        'cdf of another size': changed(map_cdf=good['map_cdf'][:-1]),
        'limits out of order': changed(map_lon0=good['map_lon1'], map_lon1=good['map_lon0']),
        'sin(latitude) beyond 1': changed(map_s1=1.5),
        'nodes without cdf': {k: v for k, v in good.items() if k != 'map_cdf'},
        '1-D: flat cdf': dict(one_d, spatial_type=3, map_nodes=grid,
                              map_cdf=np.ones_like(grid_cdf)),
        '1-D: decreasing cdf': dict(one_d, spatial_type=3, map_nodes=grid,
                                    map_cdf=grid_cdf[::-1].copy()),
        'PCG64 stream': dict(good, pcg64=(1000, 0)),
    }
    for what, src in bad.items():
        with pytest.raises((hip_api.HipError, ValueError)):
            ctx.sample_packets(1000, 5, download=True, **src)
            pytest.fail(f'{what}: accepted')
    X = ctx.sample_packets(1000, 5, download=True, **base)
    assert np.all(np.isfinite(X)) and np.all(X[7] == 1.0)
    X = ctx.sample_packets(1000, 5, download=True, **good)
    assert np.all(np.isfinite(X))


# ---- 10. closing the loop ----------------------------------------------------------------------------
def test_run_to_map_to_file_to_run(ctx, tmp_path):
    first = Input(BENCH_INPUT)
    first.options.endtime = type(first.options.endtime)(6000., 's')
    with quiet():
        first.run(300000, seed=17, context=ctx)              # host sampler: X0 kept
    res = LOSResult.__new__(LOSResult)
    res.inputs, res.sourcerate, res._ctx = first, 1.0, ctx
    res.unit_km = first.geometry.planet.radius.value
    with quiet():
        source, _ = res.make_source_map(SMALL, normalize=True, do_available=False)
    assert np.all(np.isfinite(source.abundance)) and source.abundance.max() > 0
    path = str(tmp_path / 'fitted_map.npz')
    source.save(path)
    back = SourceMap(path)
    assert np.array_equal(back.abundance, source.abundance)

    inputs = map_input(tmp_path, mapfile=path, vdistfile=path)
    n = 400000
    with quiet():
        out = Output(inputs, n, seed=23, integrate=False, save=False, context=ctx,
                     sampler='device')
    X = out.X0[STATE].values.T
    lon, s = lon_s(X, inputs.spatialdist.exobase)
    _, limits = surface_map_cells(back.longitude, back.latitude, back.abundance)
    p_cells = R.cell_goodness_of_fit(lon, s, back.abundance, limits)
    cdf, grid = density_cdf(back.speed, back.speed_dist)
    speed = out.X0.v.values*out.unit_km
    p_speed = stats.kstest(speed, lambda v: np.interp(v, grid, cdf)).pvalue
    print(f'loop: cells p={p_cells:.4f} speeds p={p_speed:.4f}')
    assert p_cells > P_MIN and p_speed > P_MIN

    # Input.run and the streaming image draw the same packets from the map
    params = {'quantity': 'radiance', 'dims': '64,64'}
    with quiet():
        inputs.run(200000, packs_per_it=100000, seed=29, context=ctx, sampler='device')
        two_stage = inputs.produce_image(params, context=ctx)
        streaming = ModelImage(inputs, params, npackets=200000, packs_per_it=100000, seed=29,
                               context=ctx, sampler='device')
    assert [len(o) for o in inputs._catalogue] == [100000, 100000]
    assert two_stage.totalsource == streaming.totalsource
    assert streaming.packet_image.sum() > 1e5
    assert np.array_equal(two_stage.packet_image, streaming.packet_image)
    np.testing.assert_allclose(two_stage.image, streaming.image, rtol=1e-11)
    # ... and so does one Output of all of them, binned by create_image (saved, i.e. narrowed to
    # float32 as the catalogued Outputs are: the streaming image bins float32 samples as well)
    with quiet():
        whole = Output(inputs, 200000, seed=29, context=ctx, sampler='device')
        weighted, counted = streaming.create_image(whole)
    assert np.array_equal(counted.histogram, streaming.packet_image)
    np.testing.assert_allclose(weighted.histogram*streaming.atoms_per_packet, streaming.image,
                               rtol=1e-11)
