"""ModelDensity(spectrum=...) without a GPU: the restatement the GPU tests lean on against a plain
double loop, the host formulas (``spectrum_from_sums``) on known answers, every refusal of
``parse_spectrum``, the enable's argument check as a host program (plain and under the host
sanitizers), and a physics pin of the restatement on a Maxwellian.  The device is replaced by a
stand-in that answers the density calls with the restatement (SpectrumContext below)."""
import contextlib
import inspect
import io
import math
import os
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

from tests.density_spectrum_restatement import brute_force, frames_of, restate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
COLUMNS = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')


def _stand_in():
    from tests.oracle_context import OracleContext

    class SpectrumContext(OracleContext):
        """The density calls of hip_api.Context answered by the restatement over every sample
        handed in (host columns only)."""

        def density_set(self, points, cell_start, origin, h, dr, dims):
            self._dpoints, self._ddr = np.array(points, dtype=np.float64).reshape(-1, 3), float(dr)
            self._dcols, self._dspec = [], None

        def density_spectrum_enable(self, nv, s_lo=0.0, s_hi=0.0, cos_half=-1.0, all_sky=True,
                                    frames=None):
            self._dspec = (np.array(frames, dtype=np.float64), int(nv), float(s_lo), float(s_hi),
                           float(cos_half), bool(all_sky))

        def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
            zero = np.zeros(len(x))
            self._dcols.append((x, y, z, zero, zero, zero, frac))

        def density_spectrum_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                        frac=None, rows=None):
            assert self._dspec is not None, 'density_spectrum_enable has not been called'
            self._dcols.append((x, y, z, vx, vy, vz, frac))

        def _restated(self):
            spec = self._dspec or (np.zeros((len(self._dpoints), 8)), 1, 0., 1., -1., True)
            cols = [np.concatenate([np.asarray(c, dtype=np.float64) for c in col])
                    for col in zip(*self._dcols)] if self._dcols else [np.zeros(0)]*7
            return restate(self._dpoints, self._ddr, *spec, *cols)

        def density_download(self):
            got = self._restated()
            return got.s0.copy(), got.counts.copy()

        def density_spectrum_download(self):
            return self._restated().sums.copy()
    return SpectrumContext


def _fake_inputs(runs=()):
    from nexoclom_amd import Input
    inputs = Input(INPUT)
    inputs._catalogue = list(runs)
    return inputs


def _run(columns, totalsource=1000.):
    X = pd.DataFrame({c: np.asarray(v, dtype=np.float64) for c, v in zip(COLUMNS, columns)})
    return types.SimpleNamespace(X=X, totalsource=totalsource, npackets=len(X), idnum=1, filename='a')


def _model(runs, pts, dr=0.1, **kwargs):
    from nexoclom_amd import ModelDensity
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        return ModelDensity(_fake_inputs(runs), pts[:, 0], pts[:, 1], pts[:, 2], dr=dr,
                            context=_stand_in()(), **kwargs)


NEW_ATTRIBUTES = ('spectrum_sums', 'speed_edges', 'speed_axis', 'energy_edges', 'density_spectrum',
                  'density_below', 'density_above', 'density_in_view', 'flux_spectrum',
                  'flux_below', 'flux_above', 'flux', 'spectrum_effective_packets',
                  'flux_effective_packets')


def test_spectrum_keyword_exists():
    """The test that fails without the feature: ModelDensity takes ``spectrum``; without it the
    object has none of the new attributes."""
    from nexoclom_amd import ModelDensity
    assert 'spectrum' in inspect.signature(ModelDensity.__init__).parameters
    run = _run(([1.0], [0.], [0.], [1e-4], [0.], [0.], [0.5]))
    d = _model([run], [[1.0, 0., 0.]], spectrum=dict(speed=(0., 4., 8)))
    assert d.spectrum_sums.shape == (2, 1, 10, 2)
    assert all(hasattr(d, name) for name in NEW_ATTRIBUTES)
    plain = _model([run], [[1.0, 0., 0.]])
    assert not any(hasattr(plain, name) for name in NEW_ATTRIBUTES)
    assert np.array_equal(plain.density, d.density) and np.array_equal(plain.packets, d.packets)


def _cloud(rng, p, dtype=np.float32):
    cols = [rng.uniform(-1, 1, p) for _ in range(3)] + \
           [rng.normal(1e-4, 2e-4, p) for _ in range(3)] + [rng.uniform(0, 1, p)]
    return [c.astype(dtype) for c in cols]                  # widened, as stored rows are


@pytest.mark.parametrize('all_sky', [False, True])
def test_restatement_equals_a_double_loop(all_sky):
    """400 rows x 30 points, bit for bit: the NumPy steps and the Python-float steps give the same
    members, planes, seen rows and terms, and both add them in row order, so every sum of the two
    planes and S0 are equal."""
    rng = np.random.default_rng(41)
    dr, Q = 0.6, 30
    cols = _cloud(rng, 400)
    pts = np.concatenate([rng.uniform(-1, 1, (Q - 3, 3)),
                          np.stack(cols[:3], axis=1)[:3].astype(np.float64)])
    b = rng.normal(size=(Q, 3))
    b /= np.linalg.norm(b, axis=1)[:, None]
    frames = frames_of(rng.normal(0, 2e-4, (Q, 3)), b, Q)
    args = (pts, dr, frames, 6, 1e-4, 5e-4, math.cos(math.radians(70.)), all_sky)
    want = restate(*args, *cols)
    sums, s0, counts, seen = brute_force(*args, *cols)
    assert np.array_equal(counts, want.counts) and want.counts.sum() > 500
    assert np.array_equal(seen, want.seen)
    assert (want.seen[:, 0] > 0).any() and (want.seen[:, -1] > 0).any() and (want.seen[:, 1:-1] > 0).any()
    if all_sky:
        assert np.array_equal(want.seen.sum(axis=1), want.counts)
    else:
        assert 0 < want.seen.sum() < want.counts.sum()
    assert (want.seen >= 8).any() and (want.counts >= 8).all()           # past np.sum's pairing
    assert np.array_equal(sums, want.sums)
    assert np.array_equal(s0, want.s0)
    # a record with one term or none has a zero bound: equal
    assert not want.bound[:, want.seen <= 1].any()


def test_the_planes_sum_to_what_is_in_view_and_all_sky_to_s0():
    from nexoclom_amd.ModelDensity import spectrum_from_sums
    rng = np.random.default_rng(42)
    Q, nv = 25, 7
    cols = _cloud(rng, 4000)
    pts = rng.uniform(-1, 1, (Q, 3))
    frames = frames_of(rng.normal(0, 2e-4, (Q, 3)), [0., 1., 0.], Q)
    for all_sky in (False, True):
        want = restate(pts, 0.3, frames, nv, 1e-4, 4e-4, 0.5, all_sky, *cols)
        out = spectrum_from_sums(want.sums, 3.0, 2440., 0.244, 0.976, 3.8e-26)
        for name in ('density', 'flux'):
            total = out[name + '_below'] + out[name + '_spectrum'].sum(axis=1) + out[name + '_above']
            whole = out['density_in_view' if name == 'density' else name]
            # positive terms, nv + 2 additions and the scalings: a few roundings each way
            np.testing.assert_allclose(total, whole, rtol=(nv + 4) * 2.0**-52, atol=0)
        assert out['density_spectrum'].shape == (Q, nv) and out['density_in_view'].shape == (Q,)
        if all_sky:
            # the planes' sums added up are one more order of adding the point's n fracs
            in_view = want.sums[0, :, :, 0].sum(axis=1)
            assert want.counts.sum() > 1000
            assert np.all(np.abs(in_view - want.s0) <= want.bound_s0)
        else:
            assert np.all(want.sums[0, :, :, 0].sum(axis=1) <= want.s0 * (1 + 1e-12))


def test_units_on_a_hand_made_case():
    """Two points, each with rows of known speed; every factor written out."""
    from nexoclom_amd import Input, constants
    R = float(Input(INPUT).geometry.planet.radius.value)
    m = constants.ATOMIC_MASS['Na'] * constants.AMU
    a = 2.0**-12                                    # R/s
    # point 0 at x = 1: rows with c = v - u of 1.5 a (bin 1 of 2) and 0.5 a (bin 0), fracs 0.5, 0.25
    # point 1 at x = 3: one row at rest, seen from u = (2.5 a, 0, 0): above the range; frac 1
    cols = ([1.0, 1.01, 3.0], [0.]*3, [0.]*3, [0., 0., 0.], [1.5*a, 0., 0.], [0., 0.5*a, 0.],
            [0.5, 0.25, 1.0])
    spec = dict(speed=(0., 2*a*R, 2), velocity=[[0., 0., 0.], [2.5*a*R, 0., 0.]])
    d = _model([_run(cols, totalsource=1000.)], [[1.0, 0, 0], [3.0, 0, 0]], spectrum=spec)
    assert np.array_equal(d.packets, [2, 1])
    scale = d.atoms_per_packet / float(d.Vpix)
    np.testing.assert_allclose(d.speed_edges, [0., a*R, 2*a*R], rtol=1e-15)
    np.testing.assert_allclose(d.speed_axis, [0.5*a*R, 1.5*a*R], rtol=1e-15)
    np.testing.assert_allclose(d.energy_edges, 0.5*m*(d.speed_edges*1e3)**2/1.602176634e-19, rtol=1e-15)
    np.testing.assert_allclose(d.density_spectrum, [[0.25*scale, 0.5*scale], [0., 0.]], rtol=1e-15)
    np.testing.assert_allclose(d.density_above, [0., 1.0*scale], rtol=1e-15)
    assert not d.density_below.any()
    np.testing.assert_allclose(d.density_in_view, d.density, rtol=1e-15)
    cm = R*1e5                                      # R/s -> cm/s
    np.testing.assert_allclose(d.flux_spectrum, [[0.25*0.5*a*cm*scale, 0.5*1.5*a*cm*scale], [0., 0.]],
                               rtol=1e-14)
    np.testing.assert_allclose(d.flux_above, [0., 2.5*a*cm*scale], rtol=1e-14)
    np.testing.assert_allclose(d.flux, [(0.125 + 0.75)*a*cm*scale, 2.5*a*cm*scale], rtol=1e-14)
    # one row per bin: one effective packet; empty bins: 0, and nothing is NaN
    assert np.array_equal(d.spectrum_effective_packets, [[1., 1.], [0., 0.]])
    assert np.array_equal(d.flux_effective_packets, [[1., 1.], [0., 0.]])
    assert all(np.isfinite(getattr(d, n)).all() for n in NEW_ATTRIBUTES)
    # a 60 degree cone about +x at point 0 sees what arrives from +x: c along -x -- neither row
    spec.update(boresight=[1., 0., 0.], half_angle=60.)
    cone = _model([_run(cols)], [[1.0, 0, 0], [3.0, 0, 0]], spectrum=spec)
    assert np.array_equal(cone.packets, [2, 1]) and not cone.density_in_view[0]
    np.testing.assert_allclose(cone.density_in_view[1], 1.0*scale, rtol=1e-15)   # c = -u: from +x
    np.testing.assert_allclose(cone.density, d.density, rtol=1e-15)


def test_effective_packets_and_points_left_out():
    from nexoclom_amd.ModelDensity import spectrum_from_sums
    sums = np.zeros((2, 2, 5, 2))
    sums[0, 1, :, 0] = [1., 2., 0., 4., 8.]
    sums[0, 1, :, 1] = [1., 2., 0., 4., 16.]
    out = spectrum_from_sums(sums, 2.0, 10., 0., 3., 1e-26)
    assert np.array_equal(out['spectrum_effective_packets'], [[0., 0., 0.], [2., 0., 4.]])
    assert np.array_equal(out['density_spectrum'], [[0., 0., 0.], [4., 0., 8.]])
    assert np.array_equal(out['density_below'], [0., 2.]) and np.array_equal(out['density_above'], [0., 16.])
    assert np.array_equal(out['density_in_view'], [0., 30.])
    assert not out['flux_effective_packets'].any() and not out['flux'].any()
    # a point with a non-finite coordinate is left out of the index: zeros, and the others keep
    # their own frames (per-point velocities are permuted with the index)
    a = 2.0**-12
    cols = ([1.0, 3.0], [0.]*2, [0.]*2, [0., 0.], [0., 0.], [0., 0.], [1.0, 1.0])
    R = float(_fake_inputs().geometry.planet.radius.value)
    pts = [[3.0, 0, 0], [np.nan, 0, 0], [1.0, 0, 0]]
    spec = dict(speed=(0., 4*a*R, 4), velocity=[[3.5*a*R, 0, 0], [9., 9., 9.], [0.5*a*R, 0, 0]])
    d = _model([_run(cols)], pts, spectrum=spec)
    assert np.array_equal(d.packets, [1, 0, 1])
    assert np.array_equal(d.density_spectrum > 0, [[0, 0, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0]])
    assert not d.spectrum_sums[:, 1].any()


BAD = [
    ('not a dict', (0., 4., 8)),
    ('no speed', dict(velocity=(1., 0., 0.))),
    ('unknown key', dict(speed=(0., 4., 8), aperture=3.)),
    ('two numbers', dict(speed=(0., 4.))),
    ('empty range', dict(speed=(2., 2., 8))),
    ('reversed range', dict(speed=(4., 2., 8))),
    ('negative s_lo', dict(speed=(-0.5, 4., 8))),
    ('NaN s_hi', dict(speed=(0., np.nan, 8))),
    ('infinite s_hi', dict(speed=(0., np.inf, 8))),
    ('no bins', dict(speed=(0., 4., 0))),
    ('fractional bins', dict(speed=(0., 4., 2.5))),
    ('half_angle 0', dict(speed=(0., 4., 8), boresight=(1., 0., 0.), half_angle=0.)),
    ('half_angle negative', dict(speed=(0., 4., 8), boresight=(1., 0., 0.), half_angle=-10.)),
    ('half_angle above 180', dict(speed=(0., 4., 8), boresight=(1., 0., 0.), half_angle=180.5)),
    ('half_angle NaN', dict(speed=(0., 4., 8), boresight=(1., 0., 0.), half_angle=np.nan)),
    ('velocity shape', dict(speed=(0., 4., 8), velocity=np.zeros((2, 3)))),
    ('velocity of four', dict(speed=(0., 4., 8), velocity=(1., 0., 0., 0.))),
    ('boresight shape', dict(speed=(0., 4., 8), boresight=np.ones((4, 3)))),
    ('velocity NaN', dict(speed=(0., 4., 8), velocity=(np.nan, 0., 0.))),
    ('velocity infinite', dict(speed=(0., 4., 8), velocity=(np.inf, 0., 0.))),
    ('boresight NaN', dict(speed=(0., 4., 8), boresight=(0., np.nan, 1.))),
    ('boresight zero', dict(speed=(0., 4., 8), boresight=(0., 0., 0.))),
    ('boresight name', dict(speed=(0., 4., 8), velocity=(1., 0., 0.), boresight='wake')),
    ('ram at rest', dict(speed=(0., 4., 8), boresight='ram')),
    ('ram at rest at one point', dict(speed=(0., 4., 8), boresight='ram',
                                      velocity=[[1., 0., 0.], [0., 0., 0.], [0., 1., 0.]])),
]


@pytest.mark.parametrize('bad', [b[1] for b in BAD], ids=[b[0] for b in BAD])
def test_a_bad_spectrum_is_refused_before_a_context_is_opened(bad):
    """No context is given and this machine may have no device: a ValueError, nothing else."""
    from nexoclom_amd import ModelDensity
    from nexoclom_amd.ModelDensity import parse_spectrum
    with pytest.raises(ValueError, match='spectrum='):
        parse_spectrum(bad, 3)
    with pytest.raises(ValueError, match='spectrum='):
        ModelDensity(_fake_inputs(), [0., 1., 2.], [0., 0., 0.], [0., 0., 0.], spectrum=bad)


def test_parse_spectrum():
    from nexoclom_amd.ModelDensity import parse_spectrum
    got = parse_spectrum(dict(speed=(0, 4, np.int64(8))), 3)
    assert got['speed'] == (0.0, 4.0, 8) and got['all_sky'] and got['cos_half'] == -1.0
    assert got['velocity'].shape == (3, 3) and not got['velocity'].any() and not got['boresight'].any()
    u = np.array([[3., 0., 4.], [0., 2., 0.], [1., 1., 1.]])
    got = parse_spectrum(dict(speed=(0.5, 4, 8), velocity=u, boresight='ram', half_angle=30), 3)
    assert not got['all_sky'] and got['cos_half'] == np.cos(np.radians(30.))
    np.testing.assert_allclose(got['boresight'], u/np.linalg.norm(u, axis=1)[:, None], rtol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(got['boresight'], axis=1), 1., rtol=1e-15)
    got = parse_spectrum(dict(speed=(0.5, 4, 8), boresight=(0., 0., 5.), half_angle=180), 2)
    assert got['all_sky'] and np.array_equal(got['boresight'], [[0., 0., 1.]]*2)
    got = parse_spectrum(dict(speed=(0.5, 4, 8), half_angle=45), 2)     # no boresight: the whole sky
    assert got['all_sky']
    with pytest.raises(ValueError, match='2\\^31'):
        parse_spectrum(dict(speed=(0., 4., 2**20)), 2**11)


@pytest.mark.parametrize('kw', [dict(moments=True), dict(cp=object())], ids=['moments', 'cp'])
def test_model_density_refuses_spectrum_with(kw):
    from nexoclom_amd import ModelDensity
    with pytest.raises(NotImplementedError) as err:
        ModelDensity(_fake_inputs(), [0.], [0.], [0.], context=object(),
                     spectrum=dict(speed=(0., 4., 8)), **kw)
    assert 'spectrum=' in str(err.value) and next(iter(kw)) in str(err.value)


@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_argument_check_as_a_host_program(tmp_path, flags):
    """nxc_density_spectrum_enable's refusals are host-only code (nxc_spectrum_check.hpp);
    tests/tools/spectrum_check.cpp feeds it good arguments, one bad set per refusal, bad frame
    records and nv one below and at the 2^31 record limit.  Built plainly and with the host
    sanitizers; both runs must pass."""
    exe = tmp_path / 'spectrum_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'spectrum_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    assert sum(' refused: ' in line for line in lines) >= 30
    assert sum(line.endswith(' accepted') for line in lines) >= 11
    assert not done.stderr.strip()


def test_the_library_exports_the_five_entry_points():
    from nexoclom_amd import hip_api
    names = [f'nxc_density_spectrum_{what}'
             for what in ('enable', 'accumulate', 'accumulate_f32', 'accumulate_rows', 'download')]
    assert all(name in hip_api.EXPORTS for name in names)
    for what in ('enable', 'accumulate', 'download'):
        assert callable(getattr(hip_api.Context, f'density_spectrum_{what}'))
    header = open(os.path.join(ROOT, 'include', 'nexoclom_hip.h')).read()
    assert all(f'int {name}(' in header for name in names)


def test_maxwellian_seen_from_a_moving_spacecraft():
    """A physics pin on the restatement alone: 2e5 rows of equal frac of a Maxwellian at rest
    (sigma per axis) inside one ball, seen from a spacecraft of speed U.

    With all_sky the mean arrival speed, flux / density = sum(f s) / sum(f), is that of |v - u|:
        sigma sqrt(2/pi) exp(-U^2 / 2 sigma^2) + (U + sigma^2 / U) erf(U / (sigma sqrt 2)),
    and its standard error is the sample's own: std(s) / sqrt(N).  With a cone of 90 degrees about
    the ram direction a row is in view iff its velocity along u is below U (to the 6e-17 of
    cos(radians(90))): a fraction (1 + erf(U / (sigma sqrt 2))) / 2, a binomial proportion with
    the standard error sqrt(p (1 - p) / N) taken from the sample's own p.  Both within 4 standard
    errors; the seed is fixed (and was chosen so that the restatement passes)."""
    N, sigma, U = 200_000, 1.5e-4, 2.5e-4                     # R/s
    rng = np.random.default_rng(43)
    v = rng.normal(0, sigma, (N, 3))
    xyz = 2.0 + rng.uniform(-0.02, 0.02, (N, 3))
    u = U * np.array([2., -1., 2.]) / 3.
    frames = frames_of(u, u / U, 1)
    nv, s_lo, s_hi = 16, 1e-4, 6e-4
    args = (*xyz.T, *v.T, np.full(N, 0.25))
    sky = restate([[2., 2., 2.]], 0.1, frames, nv, s_lo, s_hi, -1.0, True, *args)
    assert sky.counts[0] == N and sky.seen.sum() == N
    assert sky.seen[0, 0] > 0 and sky.seen[0, -1] > 0 and (sky.seen[0, 1:-1] > 0).all()
    density, flux = sky.sums[0, 0, :, 0].sum(), sky.sums[1, 0, :, 0].sum()
    mean = flux / density
    # sum f = N f, sum f^2 s^2 = f^2 sum s^2: the sample variance of s from the sums themselves
    second = sky.sums[1, 0, :, 1].sum() / sky.sums[0, 0, :, 1].sum()
    stderr = math.sqrt((second - mean*mean) / N)
    want = sigma*math.sqrt(2/math.pi)*math.exp(-U*U/(2*sigma*sigma)) \
        + (U + sigma*sigma/U)*math.erf(U/(sigma*math.sqrt(2)))
    print(f'mean arrival speed {mean:.6e} want {want:.6e} ({(mean - want)/stderr:+.2f} standard errors)')
    assert abs(mean - want) <= 4*stderr
    ram = restate([[2., 2., 2.]], 0.1, frames, nv, s_lo, s_hi, math.cos(math.radians(90.)), False, *args)
    assert ram.counts[0] == N
    p = ram.sums[0, 0, :, 0].sum() / ram.s0[0]
    assert p == ram.seen.sum() / N                           # equal fracs of 1/4: exact sums
    want_p = 0.5*(1 + math.erf(U/(sigma*math.sqrt(2))))
    stderr_p = math.sqrt(p*(1 - p)/N)
    print(f'fraction in view {p:.6f} want {want_p:.6f} ({(p - want_p)/stderr_p:+.2f} standard errors)')
    assert abs(p - want_p) <= 4*stderr_p
