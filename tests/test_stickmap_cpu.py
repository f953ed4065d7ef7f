"""Sticking from a surface map on the CPU: the inputfile reaches the bounce configuration, the
host's stickcoef(lon, lat) is the documented interpolation, every refusal, and the libm spread the
GPU tolerance of tests/test_gpu_stickmap.py is built on.

Bound of stickcoef against an independent interpolator (scipy interpn on the padded table).  Both
evaluate the same bilinear form of exact data with values and weights in [0, 1], so nothing
cancels.  With u = 2^-53: wl = (lon - L[i]) / (L[i+1] - L[i]) carries 3 roundings (relative 3u,
and wl <= 1), wt the same; 1 - wl and 1 - wt one more each (absolute u); each of the two inner
sums is two products and a sum of terms <= 1 (3u on top of the 4u its weights bring), the outer
sum again two products and a sum (3u, plus 4u from wt): below 16u for a sum that is at most 1.
scipy's form (products of weights times values, summed) has as many operations: 16u again.  Where
the seam is involved there is one more source: lon + 2 pi and the padded nodes L[0] + 2 pi,
L[n-1] - 2 pi are each rounded to the doubles around 2 pi, 4.5e-16 away at most, which moves wl by
up to 2 x 4.5e-16 / (seam interval) and S by that times the step across the seam.  So
    |stickcoef - interpn| <= 32u + 9e-16 max|dS| / min(dL)
with max|dS| the largest step between longitude neighbours and min(dL) the narrowest interval:
3.6e-15 + 9e-16 x (at most 0.9 / 0.0175) for the maps here.
"""
import os
import types

import numpy as np
import pytest
from scipy.interpolate import interpn

from nexoclom_amd import Input, surface
from nexoclom_amd.input_classes import InputError
from nexoclom_amd.sourcemap import SourceMap
from tests import bounce_cases as B
from tests import stickmap_restatement as SR

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0**-53

TEMPLATE = """geometry.planet = Mercury
geometry.taa = 1.3
SurfaceInteraction.sticktype = surface map
SurfaceInteraction.stick_mapfile = {mapfile}
SurfaceInteraction.accomfactor = {accom}
{extra}
SpatialDist.type = uniform
SpeedDist.type = flat
SpeedDist.vprob = 2.
SpeedDist.delv = 1.5
AngularDist.type = isotropic
options.endtime = 9000.
options.lifetime = 0.
options.species = Na
options.outeredge = 15
options.step_size = 30.
"""


def write_map(path, stick_map, **more):
    lon, lat, coef = stick_map
    contents = dict(abundance=coef, longitude=lon, latitude=lat)
    contents.update(more)
    SourceMap({k: v for k, v in contents.items() if v is not None}).save(str(path))
    return str(path)


def map_inputs(tmp_path, mapfile, accom=0.2, extra=''):
    infile = tmp_path / 'stickmap.input'
    infile.write_text(TEMPLATE.format(mapfile=mapfile, accom=accom, extra=extra))
    return Input(str(infile))


# ---- the inputfile reaches the kernel's configuration: fails without the feature ----------------------
def test_an_output_of_a_surface_map_inputfile_carries_law_2_and_the_map(tmp_path):
    from nexoclom_amd.Output import Output
    lon, lat, coef = SR.smooth_map()
    inputs = map_inputs(tmp_path, write_map(tmp_path / 'stick.npz', (lon, lat, coef)))
    assert inputs.surfaceinteraction.sticktype == 'surface map'
    out = Output(inputs, 100, seed=5, integrate=False, save=False)
    cfg = out._bounce
    assert cfg['temp_dependent'] == 2 and cfg['stickcoef'] == 0.0 and cfg['accomfactor'] == 0.2
    got_lon, got_lat, got_coef = cfg['stick_map']
    assert np.array_equal(got_lon, lon) and np.array_equal(got_lat, lat) and np.array_equal(got_coef, coef)
    assert got_coef.flags['C_CONTIGUOUS'] and got_coef.dtype == np.float64
    assert cfg['tx'].any()                                       # accommodation: the v(T, p) spline
    probe = np.array([0.3, 3.0, 6.2]), np.array([-1.2, 0.1, 1.5])
    assert np.array_equal(cfg['surf'].stickcoef(*probe), surface.sticking_map_callable(lon, lat, coef)(*probe))
    # 1-D, without accommodation
    lon1, _, coef1 = SR.longitude_map()
    inputs = map_inputs(tmp_path, write_map(tmp_path / 'lon.npz', (lon1, None, coef1)), accom=0)
    cfg = surface.bounce_config(inputs, -1e-3, 2440., 7)
    assert cfg['temp_dependent'] == 2 and cfg['stick_map'][1] is None and not cfg['tx'].any()
    assert np.array_equal(cfg['stick_map'][2], coef1)


def test_the_example_inputfile_parses_and_names_its_map():
    example = os.path.join(os.path.dirname(HERE), 'nexoclom_amd', 'inputfiles', 'Na.mercury.stickmap.input')
    spec = Input(example).surfaceinteraction
    assert (spec.sticktype, spec.stick_mapfile, spec.accomfactor) == ('surface map', 'stickmap.npz', 0.2)


# ---- the interpolation ------------------------------------------------------------------------------
def reference_interp(stick_map, lon, lat):
    lon2, lat2, coef2 = SR.padded(*stick_map)
    lon = np.asarray(lon, dtype=float)
    if lat2 is None:
        return interpn((lon2,), coef2, lon[:, None], method='linear')
    return interpn((lon2, lat2), coef2, np.stack([lon, np.asarray(lat, dtype=float)], 1), method='linear')


def bound(stick_map):
    lon, _, coef = stick_map
    dL = np.diff(np.concatenate([lon, [lon[0] + 2*np.pi]]))
    dS = np.abs(np.diff(np.concatenate([coef, coef[:1]], axis=0), axis=0)).max()
    return 32*U + 9e-16*dS/dL.min()


@pytest.mark.parametrize('which', list(SR.MAPS) + ['one degree'])
def test_stickcoef_is_bilinear_periodic_and_clamped(which):
    if which == 'one degree':
        inputs = types.SimpleNamespace(geometry=B.geometry(1.3),
                                       surfaceinteraction=types.SimpleNamespace(A=B.DEFAULT_A))
        m = surface.sticking_map_from_law(inputs, np.radians(np.arange(360.)), np.radians(np.arange(-90., 91.)))
        stick_map = (m.longitude, m.latitude, m.abundance)
    else:
        stick_map = SR.MAPS[which]()
    L, T, S = surface.check_sticking_map(*stick_map)
    f = surface.sticking_map_callable(L, T, S)
    rng = np.random.default_rng(3)
    lat_nodes = np.array([-0.3, 0.4]) if T is None else T
    groups = {
        'random': (rng.uniform(0, 2*np.pi, 20000), np.arcsin(rng.uniform(-1, 1, 20000))),
        'nodes': (np.repeat(L, len(lat_nodes)), np.tile(lat_nodes, len(L))),
        'next to nodes': (np.nextafter(np.repeat(L, 2), np.tile([-1., 7.], len(L))).clip(0, None),
                          np.resize(lat_nodes, 2*len(L))),
        'seam': (np.concatenate([np.linspace(L[-1], np.nextafter(2*np.pi, 0), 300), np.linspace(0, L[0], 300),
                                 [0.0, np.nextafter(2*np.pi, 0), L[0], L[-1]]]),
                 np.resize(np.linspace(-1.5, 1.5, 41), 604)),
        'beyond the end latitudes': (rng.uniform(0, 2*np.pi, 600),
                                     np.concatenate([np.linspace(-np.pi/2, lat_nodes[0], 300),
                                                     np.linspace(lat_nodes[-1], np.pi/2, 300)])),
    }
    tol = bound((L, T, S))
    for what, (lon, lat) in groups.items():
        got = f(lon, lat)
        want = reference_interp((L, T, S), lon, lat)
        err = np.abs(got - want).max()
        print(f'{which} / {what}: {len(lon)} points, largest difference {err:.3g} (bound {tol:.3g})')
        assert got.shape == lon.shape and np.all((got >= 0) & (got <= 1))
        assert err <= tol, (which, what, err)
    # at a node the value is the node's, to the bit (weights 0 and 1 are exact)
    lon, lat = groups['nodes']
    node = S[np.searchsorted(L, lon)] if T is None else S[np.searchsorted(L, lon), np.searchsorted(T, lat)]
    assert np.array_equal(f(lon, lat), node)
    # beyond the end latitudes the value is the end row's
    if T is not None:
        lon = rng.uniform(0, 2*np.pi, 50)
        assert np.array_equal(f(lon, np.full(50, np.pi/2)), f(lon, np.full(50, T[-1])))
        assert np.array_equal(f(lon, np.full(50, -np.pi/2)), f(lon, np.full(50, T[0])))
    # scalars are taken too
    assert f(1.0, 0.2).shape == (1,)


def test_values_outside_0_1_cannot_leave_stickcoef():
    """Validation keeps such maps out; the clamp after the interpolation is the kernel's, and is
    there for the last bit of a map that touches 0 or 1."""
    lon, lat, _ = SR.smooth_map()
    f = surface.sticking_map_callable(lon, lat, np.full((36, 18), 1.0))
    assert np.all(f(np.linspace(0, 6.28, 500), np.linspace(-1.57, 1.57, 500)) == 1.0)
    f = surface.sticking_map_callable(lon, lat, np.zeros((36, 18)))
    assert np.all(f(np.linspace(0, 6.28, 500), np.linspace(-1.57, 1.57, 500)) == 0.0)


# ---- refusals ---------------------------------------------------------------------------------------
def changed(a, k, value):
    a = np.array(a, dtype=float)
    a[k] = value
    return a


def test_refusals(tmp_path):
    lon, lat, coef = SR.smooth_map()
    good = write_map(tmp_path / 'good.npz', (lon, lat, coef))
    surface.SurfaceInteraction(map_inputs(tmp_path, good))

    def refused(exc, match=None, **kw):
        with pytest.raises(exc, match=match):
            surface.bounce_config(map_inputs(tmp_path, **kw), -1e-3, 2440., 1)

    refused(InputError, mapfile='default')
    refused(InputError, mapfile=str(tmp_path / 'missing.npz'))
    # (the parser's own default is 'default' as well)
    text = TEMPLATE.format(mapfile='x', accom=0.2, extra='').replace('SurfaceInteraction.stick_mapfile = x\n', '')
    (tmp_path / 'nofile.input').write_text(text)
    with pytest.raises(InputError):
        surface.bounce_config(Input(str(tmp_path / 'nofile.input')), -1e-3, 2440., 1)
    for ending in ('.pkl', '.sav'):
        path = tmp_path / f'map{ending}'
        path.write_bytes(b'')
        refused(NotImplementedError, mapfile=str(path))
    bad = {
        'no abundance': dict(abundance=None, longitude=lon, latitude=lat),
        'no longitude': dict(abundance=coef, longitude=None, latitude=lat),
        'shape': dict(abundance=coef[:, :-1], longitude=lon, latitude=lat),
        'transposed': dict(abundance=coef.T, longitude=lon, latitude=lat),
        '2-D values, 1-D axes': dict(abundance=coef, longitude=lon, latitude=None),
        'one longitude': dict(abundance=coef[:1], longitude=lon[:1], latitude=lat),
        'one latitude': dict(abundance=coef[:, :1], longitude=lon, latitude=lat[:1]),
        'longitude repeats': dict(abundance=coef, longitude=changed(lon, 5, lon[4]), latitude=lat),
        'longitude decreases': dict(abundance=coef, longitude=lon[::-1], latitude=lat),
        'latitude repeats': dict(abundance=coef, longitude=lon, latitude=changed(lat, 5, lat[4])),
        'longitude 2 pi': dict(abundance=coef, longitude=changed(lon, 35, 2*np.pi), latitude=lat),
        'longitude below 0': dict(abundance=coef, longitude=changed(lon, 0, -1e-3), latitude=lat),
        'latitude above pi/2': dict(abundance=coef, longitude=lon, latitude=changed(lat, 17, 1.58)),
        'latitude below -pi/2': dict(abundance=coef, longitude=lon, latitude=changed(lat, 0, -1.58)),
        'longitude nan': dict(abundance=coef, longitude=changed(lon, 3, np.nan), latitude=lat),
    }
    for what, contents in bad.items():
        path = tmp_path / 'bad.npz'
        SourceMap({k: v for k, v in contents.items() if v is not None}).save(str(path))
        with pytest.raises(ValueError):
            surface.bounce_config(map_inputs(tmp_path, str(path)), -1e-3, 2440., 1)
            pytest.fail(f'{what}: accepted')
    # values: the first offending index and value are named
    for value, shown in ((np.nan, 'nan'), (np.inf, 'inf'), (-0.25, '-0.25'), (1.5, '1.5')):
        values = changed(coef, (7, 3), value)
        values[20, 11] = value
        path = write_map(tmp_path / 'bad.npz', (lon, lat, values))
        refused(ValueError, match=rf'abundance\[7, 3\] = {shown}', mapfile=path)
    path = write_map(tmp_path / 'bad.npz', (lon, None, changed(coef[:, 0], 9, 2.0)))
    refused(ValueError, match=r'abundance\[9\] = 2\.0', mapfile=path)
    # planet-fixed maps: as for source maps
    path = write_map(tmp_path / 'planet.npz', (lon, lat, coef), coordinate_system='planet-fixed')
    refused(ValueError, match='subsolarlon', mapfile=path)
    refused(NotImplementedError, match='planet-fixed', mapfile=path,
            extra='SurfaceInteraction.subsolarlon = 1.0')
    # nothing was uploaded or drawn on the way: an Output refuses in its constructor
    from nexoclom_amd.Output import Output
    with pytest.raises(NotImplementedError):
        Output(map_inputs(tmp_path, path, extra='SurfaceInteraction.subsolarlon = 1.0'), 10, seed=1,
               integrate=False, save=False)


# ---- the parser is as it was ------------------------------------------------------------------------
@pytest.mark.parametrize('number', ['05', '06'])
def test_parser_fixtures_still_parse_without_loading_a_map(number):
    """The expectations of tests/test_parser_fixtures.py for the two surface-map fixtures: the
    parser reads the parameters and leaves the file alone (05 names none, 06 one that is absent)."""
    from tests.test_parser_fixtures import EXPECTED, section_dict
    name = f'SurfaceInteraction.{number}.input'
    want = EXPECTED['surfaceinteraction_per_code'][name]
    got = section_dict(name, 'surfaceinteraction')
    assert set(want) >= {'sticktype', 'stick_mapfile', 'stick_map', 'subsolarlon', 'accomfactor'}
    assert got == want and got['sticktype'] == 'surface map' and got['stick_map'] is None


# ---- the law as a map -------------------------------------------------------------------------------
def test_sticking_map_from_law_equals_the_law_at_its_nodes(tmp_path):
    inputs = Input(os.path.join(HERE, 'inputfiles', 'Bounce.tempdep.input'))
    lon, lat = np.radians(np.arange(0., 360., 4.)), np.radians(np.arange(-90., 91., 3.))
    smap = surface.sticking_map_from_law(inputs, lon, lat)
    law = surface.SurfaceInteraction._sticking_law(inputs.geometry, inputs.surfaceinteraction.A)
    for i in (0, 7, 22, 23, 45, 67, 68, 89):
        assert np.array_equal(smap.abundance[i], law(np.full(len(lat), lon[i]), lat))
    assert smap.abundance.shape == (90, 61) and smap.abundance.min() >= 0 and smap.abundance.max() == 1.0
    assert smap.coordinate_system == 'solar-fixed'
    # and it goes through a file into a run's configuration unchanged
    path = tmp_path / 'law.npz'
    smap.save(str(path))
    cfg = surface.bounce_config(map_inputs(tmp_path, str(path)), -1e-3, 2440., 1)
    assert np.array_equal(cfg['stick_map'][2], smap.abundance)
    f = cfg['surf'].stickcoef
    grid_lon, grid_lat = np.meshgrid(lon, lat, indexing='ij')
    assert np.array_equal(f(grid_lon.ravel(), grid_lat.ravel()), smap.abundance.ravel())


# ---- the restatement and its libm spread ------------------------------------------------------------
def test_restatement_changes_frac_only_and_by_the_map():
    g = np.load(B.GOLDEN, allow_pickle=False)
    for name in ('tempdep', 'elastic'):
        taa, accom = float(g[f'{name}_scalars'][0]), float(g[f'{name}_scalars'][1])
        cfg = SR.map_config(taa, accom, SR.smooth_map(), float(g['GM']), float(g['unit_km']), int(g['seed']))
        X, ids, nb, hit = (g[f'{name}_{k}'] for k in ('X', 'ids', 'nb', 'hit'))
        got = SR.restate(X, cfg, ids, nb, hit)
        plain = B.restate(X, dict(cfg, temp_dependent=0, stickcoef=0.0), ids, nb, hit)
        assert np.array_equal(got[:, :7], plain[:, :7]) and np.array_equal(got[~hit], X[~hit])
        lon, lat = SR.impact_point(plain[hit])
        assert np.array_equal(got[hit, 7], plain[hit, 7]*(1 - cfg['surf'].stickcoef(lon, lat)))
        assert np.all(got[hit, 7] < plain[hit, 7])
        # laws 0 and 1 go through untouched
        law = B.golden_config(g, name)
        assert np.array_equal(SR.restate(X, law, ids, nb, hit), B.restate(X, law, ids, nb, hit))


def test_libm_spread_is_what_the_gpu_tolerance_was_derived_from():
    """The figures of test_gpu_stickmap's docstring: the recorded ones bound what is measured here
    and are not padded by more than 2x."""
    from tests.test_gpu_stickmap import STICKMAP_SPREAD, stickmap_spread
    g = np.load(B.GOLDEN, allow_pickle=False)
    for which, recorded in STICKMAP_SPREAD.items():
        measured = stickmap_spread(g, which)
        print(f'{which} map: libm spread of frac {measured:.3g} (recorded {recorded:.3g})')
        assert 0.5*recorded <= measured <= recorded, (which, measured)
