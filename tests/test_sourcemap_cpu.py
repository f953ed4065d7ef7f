"""Source maps without a GPU: the restatement's membership against sklearn's BallTree, the grid's
candidate cells against the restated membership, and the combination and normalisation quirks of
LOSResult.py:338-447 (sourcemap.combine_small / finish against the restatement and the literal
i, j loop), and make_source_map's driver -- one rank and two over gloo -- on a host stand-in for
the Context.source_map_* calls."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pandas as pd
import pytest

from nexoclom_amd import sourcemap as SM
from tests import sourcemap_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_packets(n, seed):
    rng = np.random.default_rng(seed)
    lat = np.arcsin(rng.uniform(-1, 1, n))
    lon = rng.uniform(0, 2*np.pi, n)
    lat[:8] = [np.pi/2 - 1e-7, -np.pi/2 + 1e-7, 0, 0.1, -0.2, 1.5, -1.5, 0.7]
    lon[:8] = [0, 2*np.pi, 0, 2*np.pi, 1e-9, 2*np.pi - 1e-9, 3, 0]
    return lat, lon


@pytest.mark.parametrize('grid', [dict(nlonbins=36, nlatbins=18),
                                  dict(nlonbins=20, nlatbins=11, smear_radius=np.radians(25))])
def test_membership_equals_balltree(grid):
    sk = pytest.importorskip('sklearn.neighbors')
    p = R.params(grid)
    lat, lon = random_packets(3000, 1)
    pt, pk = R.members(lat, lon, p)
    glon, glat = R.grid_points(p)
    glat2, glon2 = np.meshgrid(glat, glon)
    points = np.array([glat2.ravel(), glon2.ravel()]).T
    ind = sk.BallTree(np.stack([lat, lon], 1), metric='haversine').query_radius(
        points, p['smear_radius']*np.cos(points[:, 0]))
    for i, want in enumerate(ind):
        got = np.sort(pk[pt == i])
        assert np.array_equal(got, np.sort(want)), i


@pytest.mark.parametrize('grid', [None, dict(nlonbins=36, nlatbins=18),
                                  dict(nlonbins=7, nlatbins=5, smear_radius=np.radians(40)),
                                  dict(nlonbins=50, nlatbins=31, smear_radius=np.radians(3),
                                       nvelbins=3000)])
def test_tile_segments_hold_every_member(grid):
    """Every (point, packet) membership lies in a cell the point's tile walks."""
    g = SM.SourceMapGrid(grid, 2439.7)
    p = R.params(grid)
    lat, lon = random_packets(20000, 2)
    order, cell_start = g.bucket(lat, lon)
    cell_of = np.empty(len(lat), dtype=np.int64)
    for c in range(g.npoints):
        cell_of[order[cell_start[c]:cell_start[c + 1]]] = c
    pt, pk = R.members(lat, lon, p)
    assert len(pt) > 0
    tpr = -(-g.nlon // g.tile)
    i, j = pt // g.nlat, pt % g.nlat
    tile = j*tpr + i // g.tile
    for t in np.unique(tile):
        segs = g.seg[g.seg_off[t]:g.seg_off[t + 1]]
        cells = cell_of[pk[tile == t]]
        inside = np.zeros(len(cells), dtype=bool)
        for a, b in segs:
            inside |= (cells >= a) & (cells <= b)
        assert inside.all(), t
    assert cell_start[-1] == len(lat)


def test_bucket_puts_non_finite_packets_last():
    g = SM.SourceMapGrid(dict(nlonbins=8, nlatbins=4), 1.0)
    lat = np.array([0.1, np.nan, -0.3, 0.2])
    lon = np.array([1.0, 2.0, np.inf, 6.0])
    order, cell_start = g.bucket(lat, lon)
    assert cell_start[-1] == 2 and set(order[2:]) == {1, 2}


def hand_sources(rng, nlon=4, nlat=3, vmaxes=(7., 9., 9., 4.)):
    out = []
    for vmax in vmaxes:
        s = dict(longitude=R.axis(0, 2*np.pi, nlon), latitude=R.axis(-np.pi/2, np.pi/2, nlat),
                 speed=R.axis(0, vmax, 5), altitude=R.axis(0, np.pi/2, 3),
                 azimuth=R.axis(0, 2*np.pi, 4))
        s['abundance_uncor'] = rng.random((nlon, nlat))
        s['n_total'] = rng.integers(0, 5, (nlon, nlat)).astype(float)
        s['n_included'] = np.minimum(s['n_total'], rng.integers(0, 5, (nlon, nlat)))
        s['speed_dist'], s['altitude_dist'], s['azimuth_dist'] = (rng.random(n) for n in (5, 3, 4))
        s['speed_dist_map'] = rng.random((nlon, nlat, 5))
        s['altitude_dist_map'] = rng.random((nlon, nlat, 3))
        s['azimuth_dist_map'] = rng.random((nlon, nlat, 4))
        s['speed_dist_map'][0, 0] = 0                  # a point whose sum is 0 -> NaN map
        out.append(s)
    return out


def test_restated_broadcast_equals_the_literal_loop():
    sources = hand_sources(np.random.default_rng(3))
    got = R.combine(sources)
    vmax = max(s['speed'].max() for s in sources)
    want_map = np.zeros_like(sources[0]['speed_dist_map'])
    want = np.zeros(5)
    for s in sources:
        want_map += s['speed_dist_map']
        want += s['speed_dist']
        if s['speed'].max() == vmax:
            want_map += s['speed_dist_map']
            want += s['speed_dist']
        else:
            want += np.interp(got['speed'], s['speed'], s['speed_dist'])
            for i in range(want_map.shape[0]):
                for j in range(want_map.shape[1]):
                    want_map += np.interp(got['speed'], s['speed'], s['speed_dist_map'][i, j])
    np.testing.assert_allclose(got['speed_dist_map'], want_map, rtol=1e-13)
    np.testing.assert_allclose(got['speed_dist'], want, rtol=1e-14)
    assert got['speed'].max() == sources[1]['speed'].max()


def product_combine(sources):
    """sourcemap.combine_small + the map adds the device does (factor x speed map, broadcast)."""
    pieces = [dict(speed_dist=s['speed_dist'], altitude_dist=s['altitude_dist'],
                   azimuth_dist=s['azimuth_dist'],
                   speed_gridsum=s['speed_dist_map'].sum(axis=(0, 1))) for s in sources]
    vmaxes = [s['speed'][-1] + (s['speed'][1] - s['speed'][0])/2 for s in sources]
    small, factors = SM.combine_small(pieces, [float(round(v)) for v in vmaxes], 5)
    assert factors == [1.0, 2.0, 2.0, 1.0]
    d = dict(longitude=sources[0]['longitude'].copy(), latitude=sources[0]['latitude'].copy(),
             altitude=sources[0]['altitude'].copy(), azimuth=sources[0]['azimuth'].copy(),
             speed=small['speed'], speed_dist=small['speed_dist'],
             altitude_dist=small['altitude_dist'], azimuth_dist=small['azimuth_dist'])
    for key in ('abundance_uncor', 'n_total', 'n_included', 'altitude_dist_map',
                'azimuth_dist_map'):
        d[key] = sum(s[key] for s in sources)
    d['speed_dist_map'] = sum(f*s['speed_dist_map'] for f, s in zip(factors, sources)) + \
        small['broadcast']
    return d


@pytest.mark.parametrize('normalize', [True, False])
def test_combination_and_normalisation_quirks(normalize):
    sources = hand_sources(np.random.default_rng(4))
    for s in sources:
        s['n_total'][1, 1] = s['n_included'][1, 1] = 0     # 0/0: fraction 1 for the division, then 0
        s['n_total'][0, 2], s['n_included'][0, 2] = 2, 0   # uncor 0 over fraction 0: NaN -> 0
        s['abundance_uncor'][0, 2] = 0
        s['n_total'][2, 2], s['n_included'][2, 2] = 3, 0   # uncor > 0 over fraction 0: inf, kept
    want = R.normalise(R.combine(sources), normalize, 2.5, 2439.7)
    got = SM.finish(product_combine(sources), normalize, 2.5, 2439.7)
    assert (got['fraction_observed'][[1, 0, 2], [1, 2, 2]] == 0).all()
    if not normalize:
        uncor = sum(s['abundance_uncor'] for s in sources)
        assert got['abundance'][1, 1] == uncor[1, 1] and got['abundance'][0, 2] == 0
        assert np.isinf(got['abundance'][2, 2])
    for key in ('abundance', 'abundance_uncor', 'fraction_observed', 'speed_dist',
                'speed_dist_map', 'altitude_dist', 'altitude_dist_map', 'azimuth_dist',
                'azimuth_dist_map', 'altitude', 'azimuth', 'speed', 'n_total', 'n_included'):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, equal_nan=True, err_msg=key)
    raw = R.combine(sources)
    if normalize:
        # the axes altitude / azimuth are normalised, the *_dist arrays stay raw
        np.testing.assert_allclose(got['altitude_dist'], raw['altitude_dist'], rtol=1e-15)
        assert not np.allclose(got['altitude'], raw['altitude'])
        assert np.isnan(got['speed_dist_map'][0, 0]).all() or got['abundance'][0, 0] == 0


def test_source_map_object_holds_the_reference_attributes():
    m = SM.SourceMap(dict(abundance=np.ones((2, 2)), n_total=np.ones((2, 2))), normalized=True)
    for key in ('abundance', 'longitude', 'latitude', 'speed', 'speed_dist', 'azimuth',
                'azimuth_dist', 'altitude', 'altitude_dist', 'fraction_observed',
                'abundance_uncor', 'n_included', 'n_total', 'speed_dist_map',
                'altitude_dist_map', 'azimuth_dist_map'):
        assert hasattr(m, key)
    assert m.coordinate_system == 'solar-fixed' and m.units['abundance'] == '1/(cm2 s)'
    with pytest.raises(NotImplementedError):
        SM.SourceMap('map.pkl')


def test_device_sampled_outputs_raise():
    class Run:
        X0 = pd.DataFrame({'x': [1.0], 'frac': [1.0]})
    with pytest.raises(NotImplementedError, match="sampler='numpy'"):
        SM.x0_columns(Run())


class StandInContext:
    """The Context.source_map_* calls restated on the host (tests/sourcemap_restatement.py), so
    that make_source_map's driver and its cp= reductions run without a GPU."""

    def source_map_set(self, grid):
        self.grid = grid
        self.gp = dict(grid.params)
        stride = grid.nvel + grid.nalt + grid.naz + 3
        self.map = np.zeros((grid.npoints, stride))
        self.hist2d = np.zeros(grid.npoints)

    def source_map_accumulate(self, lat, lon, v, alt, az, frac, cell_start, vel_edges, available,
                              factor):
        g = self.grid
        X0 = dict(latitude=lat, longitude=lon, v=v, altitude=alt, azimuth=az, frac=frac)
        d = R.one_output(X0, g.r_km, self.gp, 'available' if available else 'source')
        assert d['speed'][-1] + (d['speed'][1] - d['speed'][0])/2 == vel_edges[-1]
        P = g.npoints
        cols = [factor*d['speed_dist_map'].reshape(P, -1), d['altitude_dist_map'].reshape(P, -1),
                d['azimuth_dist_map'].reshape(P, -1), d['n_total'].reshape(P, 1),
                d['n_included'].reshape(P, 1), d['abundance_uncor'].reshape(P, 1)]
        self.map += np.concatenate(cols, axis=1)
        w = frac if not available else np.ones_like(frac)
        inc = frac > 0
        self.hist2d += np.histogram2d(lon[inc], lat[inc], bins=(g.nlon, g.nlat), weights=w[inc],
                                      range=[[0, 2*np.pi], [-np.pi/2, np.pi/2]])[0].ravel()
        return dict(speed_dist=d['speed_dist'], altitude_dist=d['altitude_dist'],
                    azimuth_dist=d['azimuth_dist'],
                    speed_gridsum=d['speed_dist_map'].sum(axis=(0, 1)))

    def source_map_download(self):
        return self.map.copy(), self.hist2d.copy()


def stand_in_result(outs, ctx):
    from nexoclom_amd import LOSResult

    class Run:
        def __init__(self, X0):
            self.X0 = pd.DataFrame(X0)
    res = LOSResult.__new__(LOSResult)
    res.inputs = type('Inputs', (), {})()
    res.inputs._catalogue = [Run(X0) for X0 in outs]
    res.unit_km, res.sourcerate, res._ctx = 2439.7, 1.3, ctx
    return res


def hand_outputs(seed=5):
    rng = np.random.default_rng(seed)
    outs = []
    for k, n in enumerate((900, 700, 800, 600)):
        lat, lon = random_packets(n, seed + k)
        frac = rng.uniform(0, 1, n)
        frac[rng.random(n) < 0.3] = 0
        outs.append(dict(longitude=lon, latitude=lat, v=rng.uniform(0, (2. + k % 3)/2439.7, n),
                         altitude=rng.uniform(0, np.pi/2, n), azimuth=rng.uniform(0, 2*np.pi, n),
                         frac=frac))
    return outs


GP = dict(nlonbins=18, nlatbins=9, nvelbins=6, naltbins=4, nazbins=5, smear_radius=np.radians(25))


def test_driver_on_a_stand_in_context_equals_the_restatement():
    outs = hand_outputs()
    source, available = stand_in_result(outs, StandInContext()).make_source_map(GP)
    for todo, got in (('source', source), ('available', available)):
        want = R.source_map(outs, 2439.7, GP, todo, True, 1.3)
        for key in ('abundance', 'abundance_uncor', 'fraction_observed', 'speed_dist',
                    'speed_dist_map', 'altitude', 'azimuth', 'altitude_dist_map', 'n_total'):
            np.testing.assert_allclose(getattr(got, key), want[key], rtol=1e-12, equal_nan=True,
                                       err_msg=key)


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from nexoclom_amd.distributed import ControlPlane
    cp = ControlPlane(world, rank, timeout=120)
    outs = hand_outputs()
    mine = outs[rank::world]
    shared = stand_in_result(mine, StandInContext()).make_source_map(GP, cp=cp, reduce='host')
    if rank == 0:
        alone = stand_in_result(outs[0::2] + outs[1::2], StandInContext()).make_source_map(GP)
        for got, want in zip(shared, alone):
            for key in ('abundance', 'abundance_uncor', 'fraction_observed', 'speed_dist',
                        'speed_dist_map', 'altitude_dist_map', 'azimuth_dist_map', 'n_total',
                        'n_included', 'speed', 'altitude'):
                np.testing.assert_allclose(getattr(got, key), getattr(want, key), rtol=1e-12,
                                           equal_nan=True, err_msg=key)
        open(os.path.join(tmpdir, 'ok'), 'w').write('ok')
    cp.barrier()
    cp.close()


def test_two_ranks_equal_one_rank(tmp_path):
    port = 29450 + os.getpid() % 150
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / 'ok').exists()
