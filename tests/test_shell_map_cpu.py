"""ShellMap without a GPU: the definition (tests/shell_map_restatement.py, written from
include/nexoclom_hip.h) on hand cases; ShellMap's params, axes and refusals; the normalisation of
what it publishes against closed forms; the host-only check of nxc_shell_desc as a stand-alone
program, plain and under the host sanitizers; the ctypes mirror of the descriptor."""
import contextlib
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from tests.shell_map_restatement import shell_map

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
HEADER = os.path.join(ROOT, 'include', 'nexoclom_hip.h')
RTOL = 1e-11
G_TABLES = [(np.array([-5e-3, -1e-3, 2e-3, 6e-3]), np.array([3., 7., 5., 2.])),
            (np.array([-4e-3, 0., 4e-3]), np.array([1., 4., 2.]))]


def one(p, quantity='column', frac=0.37, vy=1e-3, grid=(8, 4), alt=(1.0, 3.0, 4)):
    return shell_map([p[0]], [p[1]], [p[2]], [vy], [frac], 2e-4, quantity, G_TABLES, *grid, *alt)


def cloud(n, seed, extent=4.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = d*rng.uniform(1.0, extent, n)[:, None]
    return p[:, 0], p[:, 1], p[:, 2], rng.uniform(-4e-3, 5e-3, n), rng.uniform(0.1, 1.0, n)


# ---- 1. hand cases ------------------------------------------------------------------------------
def test_longitude_is_local_time():
    """0 at the sub-solar point (-y), pi/2 at dusk (+x), pi at midnight, 3 pi/2 at dawn; eight
    bins of 45 degrees, so a point 10 degrees past each of them sits in bins 0, 2, 4, 6."""
    for k, angle in enumerate(np.radians([10., 100., 190., 280.])):
        res = one((2*np.sin(angle), -2*np.cos(angle), 0.3))
        assert res.binned == 1 and res.counts[2*k, 2] == 1 and res.counts.sum() == 1
    before_noon = one((-0.1, -2., 0.3))                           # just west of the seam
    assert before_noon.counts[7, 2] == 1
    assert 0 < before_noon.edge_guard < 0.05/(2*np.pi)


def test_latitude_bands_are_uniform_in_sine():
    for z, band in ((-1.9, 0), (-0.6, 1), (0.6, 2), (1.9, 3)):    # mu = z/2 with x^2 + y^2 + z^2 = 4
        rho = np.sqrt(4 - z*z)
        res = one((rho*np.sin(0.3), -rho*np.cos(0.3), z))
        assert res.counts[0, band] == 1 and res.counts.sum() == 1


def test_column_and_the_two_planes():
    p = (0.5, -2.0, 1.0)
    r2 = (0.5*0.5 + 2.0*2.0) + 1.0
    res = one(p)
    ix, iz = np.argwhere(res.counts)[0]
    assert res.column[ix, iz] == 0.37/r2
    k = 1 + int((np.sqrt(r2) - 1.0)*(4/2.0))
    assert k == 3
    assert list(res.sums[0, ix, iz, k]) == [0.37, 0.37*0.37]
    assert list(res.sums[1, ix, iz, k]) == [0.37/r2, (0.37/r2)*(0.37/r2)]
    assert np.count_nonzero(res.sums) == 4 and np.array_equal(res.sums, res.abs_sums)


def test_below_above_and_the_last_edge():
    below = one((0.5, -1.0, 0.2), alt=(1.5, 3.0, 4))
    assert below.binned == 1 and below.sums[:, :, :, 0, 0].sum() > 0
    assert not below.sums[:, :, :, 1:].any() and below.column.sum() > 0
    above = one((0.5, -4.0, 0.2))
    assert above.sums[:, :, :, 5, 0].sum() > 0 and not above.sums[:, :, :, :5].any()
    at_r_hi = one((0.0, -3.0, 0.0))                               # r = r_hi: t = (3 - 1) * 2 exactly
    assert at_r_hi.sums[:, :, :, 5, 0].sum() > 0                  # [r_lo, r_hi): r_hi is above
    assert at_r_hi.bin_guard == 0.0


def test_shadow_and_zero_weights_count_but_add_nothing():
    p = (0.5, 2., 0.3)                                            # inside the shadow cylinder
    dark = one(p, 'radiance')
    assert dark.binned == 1 and dark.counts.sum() == 1 and not dark.sums.any()
    assert dark.column.sum() == 0
    assert one(p, 'column').sums.any()
    assert one((1.5, 2., 0.3), 'radiance').sums[0].sum() > 0
    nothing = one((0.5, -2., 0.3), frac=0.0)
    assert nothing.binned == 1 and nothing.counts.sum() == 1 and not nothing.sums.any()


def test_nonfinite_samples():
    for kw in (dict(frac=np.nan), dict(frac=np.inf), dict(vy=np.nan)):
        res = one((0.5, -2., 0.3), 'radiance', **kw)
        assert res.binned == 0 and res.nonfinite == 1 and not res.counts.any() and not res.sums.any()
    centre = one((0., 0., 0.))                                   # mu is not a number: not binned
    assert centre.binned == 0 and centre.nonfinite == 0 and centre.samples == 1
    centre = one((0., 0., 0.), frac=np.nan)
    assert centre.binned == 0 and centre.nonfinite == 1


def test_plane_b_sums_to_the_column():
    cols = cloud(20000, 5)
    for quantity in ('column', 'radiance'):
        res = shell_map(*cols, 2e-4, quantity, G_TABLES, 12, 7, 1.5, 2.5, 9)
        assert res.binned == 20000 == res.counts.sum()
        np.testing.assert_allclose(res.sums[1, ..., 0].sum(-1), res.column, rtol=1e-12, atol=0)
        assert res.sums[0, :, :, 0, 0].sum() > 0 and res.sums[0, :, :, -1, 0].sum() > 0
        assert min(res.edge_guard, res.margin_guard, res.bin_guard) > 0


# ---- 2. ShellMap: params, axes and refusals -----------------------------------------------------------
def make_inputs():
    from nexoclom_amd import Input
    return Input(INPUT)


def build(params, **kw):
    from nexoclom_amd import ShellMap
    with contextlib.redirect_stdout(io.StringIO()):
        return ShellMap(make_inputs(), params, context=object(), **kw)


GOOD = dict(quantity='column', dims='8,6', altitude='0.5,2.5,4')


def test_params_make_the_axes():
    sm = build(GOOD)
    assert sm.column.shape == sm.packets.shape == (8, 6) and not sm.column.any()
    assert sm.density.shape == sm.column_profile.shape == (8, 6, 4)
    assert sm.column_below.shape == sm.column_above.shape == (8, 6)
    assert sm.density_effective_packets.shape == sm.column_effective_packets.shape == (8, 6, 4)
    assert sm.shell_sums.shape == (2, 8, 6, 6, 2) and not sm.shell_sums.any()
    assert np.array_equal(sm.lon_edges, np.linspace(0, 2*np.pi, 9))
    assert np.array_equal(sm.mu_edges, np.linspace(-1, 1, 7))
    np.testing.assert_allclose(sm.longitude, (np.arange(8) + 0.5)*np.pi/4, rtol=1e-15)
    np.testing.assert_allclose(sm.local_time, [13.5, 16.5, 19.5, 22.5, 1.5, 4.5, 7.5, 10.5], rtol=1e-14)
    np.testing.assert_allclose(np.sin(sm.latitude), (np.arange(6) + 0.5)/3 - 1, rtol=1e-15, atol=1e-16)
    np.testing.assert_allclose(sm.altitude_edges, [0.5, 1.0, 1.5, 2.0, 2.5], rtol=1e-15)
    np.testing.assert_allclose(sm.altitude_axis, [0.75, 1.25, 1.75, 2.25], rtol=1e-15)
    np.testing.assert_allclose(sm.altitude_axis_km, sm.altitude_axis*sm.unit_km, rtol=1e-15)
    np.testing.assert_allclose(sm.altitude_edges_km, sm.altitude_edges*sm.unit_km, rtol=1e-15)
    np.testing.assert_allclose(sm.solid_angle*8*6, 4*np.pi, rtol=1e-15)
    assert sm.totalsource == 0 and sm.atoms_per_packet == 0 and sm.counters == {}


def test_local_time_of_noon_and_dusk():
    from nexoclom_amd.ShellMap import shell_axes
    axes = shell_axes(24, 2, 0.0, 1.0, 1)
    np.testing.assert_allclose(axes['local_time'][0], 12.5, rtol=1e-14)     # longitude 7.5 degrees
    np.testing.assert_allclose(axes['local_time'][6], 18.5, rtol=1e-14)     # pi/2 + 7.5 degrees
    assert np.all((axes['local_time'] >= 0) & (axes['local_time'] < 24))
    assert axes['r_edges'][0] == 1.0 and axes['r_edges'][-1] == 2.0


def test_defaults():
    sm = build({k: v for k, v in GOOD.items() if k != 'dims'})
    assert sm.column.shape == (72, 36) and sm.density.shape == (72, 36, 4)
    sm = build(dict(GOOD, quantity='radiance', altitude='0,1,3'))
    assert sm.density.shape == (8, 6, 3) and sm.wavelength == (5891, 5897)


@pytest.mark.parametrize('change, text', [
    (dict(quantity='density'), 'quantity'),
    (dict(quantity=None), 'quantity'),
    (dict(dims='0,6'), 'dims'),
    (dict(dims='8,9000'), 'dims'),
    (dict(dims='8'), 'dims'),
    (dict(dims='8,6,4'), 'dims'),
    (dict(dims='a,b'), 'dims'),
    (dict(altitude=None), 'altitude'),
    (dict(altitude='0.5,2.5'), 'altitude'),
    (dict(altitude='0.5,2.5,4,1'), 'altitude'),
    (dict(altitude='0.5,2.5,4.5'), 'altitude'),
    (dict(altitude='a,2.5,4'), 'altitude'),
    (dict(altitude='-0.1,2.5,4'), '0 <= lo < hi'),
    (dict(altitude='2.5,2.5,4'), '0 <= lo < hi'),
    (dict(altitude='3,2.5,4'), '0 <= lo < hi'),
    (dict(altitude='0.5,inf,4'), 'finite'),
    (dict(altitude='nan,2.5,4'), 'finite'),
    (dict(altitude='0.5,2.5,0'), 'nbins'),
    (dict(altitude='0.5,2.5,-3'), 'nbins'),
    (dict(dims='8192,8192', altitude='0,1,30'), '2^31'),
])
def test_refused_params(change, text):
    from nexoclom_amd import InputError
    params = {k: v for k, v in dict(GOOD, **change).items() if v is not None}
    with pytest.raises(InputError) as err:
        build(params)
    assert text in str(err.value)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(cp=object()), dict(shard=(0, 10))])
def test_out_of_scope_keywords_are_refused(kw):
    with pytest.raises(NotImplementedError) as err:
        build(GOOD, **kw)
    assert 'ShellMap' in str(err.value) or 'npackets' in str(err.value)
    with pytest.raises(TypeError):
        build(GOOD, no_such_keyword=1)
    with pytest.raises(NotImplementedError):
        build(dict(GOOD, origin='Io'))


def test_the_package_exports_the_class():
    import nexoclom_amd
    from nexoclom_amd.ShellMap import ShellMap
    assert nexoclom_amd.ShellMap is ShellMap


# ---- 3. normalisation against closed forms --------------------------------------------------------------
@pytest.mark.parametrize('quantity', ['column', 'radiance'])
def test_normalisation(quantity):
    """What ShellMap publishes from the sums (shell_from_sums), with the sums of the restatement:
    density times shell volume over all cells is the content of the altitude range, the shell
    volumes fill the range's spherical shell, and column times cell area is the sum of w / r^2."""
    from nexoclom_amd.ShellMap import shell_axes, shell_from_sums
    nlon, nlat, alt = 12, 7, (0.5, 1.5, 9)
    R_cm, app = 2440.53e5, 3.7e21
    x, y, z, vy, frac = cloud(20000, 11)
    axes = shell_axes(nlon, nlat, *alt)
    r_lo, r_hi = axes['r_edges'][0], axes['r_edges'][-1]
    assert (r_lo, r_hi) == (1.5, 2.5)
    res = shell_map(x, y, z, vy, frac, 2e-4, quantity, G_TABLES, nlon, nlat, r_lo, r_hi, alt[2])
    out = shell_from_sums(res.column, res.sums, app, axes['solid_angle'], axes['volume'], R_cm)

    # the closed forms, from the samples themselves
    r2 = (x*x + y*y) + z*z
    r = np.sqrt(r2)
    w = frac
    if quantity == 'radiance':
        sunlit = (x*x + z*z > 1.0 + 2.0**-52) | (y < 0)
        g = np.interp(vy + 2e-4, *G_TABLES[0]) + np.interp(vy + 2e-4, *G_TABLES[1])
        w = np.where(sunlit, frac, 0.0)*g/1e6
    inside = (r >= r_lo) & (r < r_hi)
    assert 3000 < inside.sum() < 17000

    V = axes['volume']*R_cm**3                                    # cm^3 per cell of a shell
    assert V.shape == (alt[2],)
    np.testing.assert_allclose((out['density']*V).sum(), app*w[inside].sum(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(V.sum()*nlon*nlat, 4*np.pi/3*(r_hi**3 - r_lo**3)*R_cm**3, rtol=RTOL,
                               atol=0)
    area = axes['solid_angle']*R_cm**2
    np.testing.assert_allclose((out['column']*area).sum(), app*(w/r2).sum(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(out['column_profile'].sum(-1) + out['column_below'] + out['column_above'],
                               out['column'], rtol=RTOL, atol=0)
    np.testing.assert_allclose((out['column_profile']*area).sum(), app*(w/r2)[inside].sum(),
                               rtol=RTOL, atol=0)
    # effective packets: (sum a)^2 / sum a^2, between 1 and the count where a shell holds samples
    for name, plane in (('density_effective_packets', 0), ('column_effective_packets', 1)):
        S, ww = res.sums[plane, ..., 1:-1, 0], res.sums[plane, ..., 1:-1, 1]
        filled = ww != 0
        assert filled.sum() > 300 and not out[name][~filled].any()
        assert np.array_equal(out[name][filled], S[filled]**2/ww[filled])
        assert np.all(out[name][filled] >= 1 - 1e-12)
        assert np.all(out[name] <= res.counts[..., None] + 1e-9)


def test_uniform_density_comes_out_uniform():
    """Samples uniform in volume between two spheres, weight 1 each: every cell of every shell has
    the same expected density n/V_total; with about 800 samples a cell the scatter is Poisson."""
    from nexoclom_amd.ShellMap import shell_axes, shell_from_sums
    rng = np.random.default_rng(3)
    n = 200_000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = (1.0 + rng.uniform(size=n)*(3.0**3 - 1.0))**(1/3)
    p = d*r[:, None]
    res = shell_map(p[:, 0], p[:, 1], p[:, 2], np.zeros(n), np.ones(n), 0.0, 'column', (), 8, 6, 1.0,
                    3.0, 5)
    axes = shell_axes(8, 6, 0.0, 2.0, 5)
    out = shell_from_sums(res.column, res.sums, 1.0, axes['solid_angle'], axes['volume'], 1.0)
    expected = n/(4*np.pi/3*(27.0 - 1.0))
    per_cell = n/(8*6*5)
    assert np.all(np.abs(out['density']/expected - 1) < 6/np.sqrt(per_cell))
    # and the zenith column of a uniform shell: n0 (r_hi - r_lo) ... of 1/r^2-weighted volume
    np.testing.assert_allclose(out['column'].mean(), expected*2.0, rtol=0.01)


# ---- 4. the C side's refusals, as a host program --------------------------------------------------------
@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_descriptor_check_as_a_host_program(tmp_path, flags):
    """nxc_shell_set's refusals are host-only code (nxc_shell_check.hpp);
    tests/tools/shell_check.cpp feeds it good descriptions, one bad one per refusal and the record
    limit one below and at the bound.  Built plainly and with the host sanitizers; both runs must
    pass."""
    exe = tmp_path / 'shell_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'shell_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    assert not done.stderr.strip()
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 35 and sum(' accepted' in line for line in lines) >= 13
    for word in ('1..8192', 'nalt must be at least 1', 'finite', 'at least 1 (the surface)',
                 'below r_hi', '2^31', 'null edges', 'increase', 'span', 'n_lines', 'g-value table',
                 '160 KiB', 'vrplanet', 'quantity', 'null description'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('1 cell, 2^31 - 1 records accepted') for line in lines)
    assert any(line.startswith('1 cell, 2^31 records refused') for line in lines)


# ---- 5. ABI ---------------------------------------------------------------------------------------------
def test_shell_desc_mirror_matches_the_compiled_header(tmp_path):
    from nexoclom_amd import hip_api
    ct = hip_api.nxc_shell_desc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("%zu", sizeof(nxc_shell_desc));']
    lines += [f'printf(" %zu", offsetof(nxc_shell_desc, {field}));' for field, *_ in ct._fields_]
    lines.append('printf("\\n"); return 0;}')
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    size, *offsets = subprocess.check_output([str(exe)], text=True).split()
    assert int(size) == C.sizeof(ct) == 3*8 + 2*4 + 3*8 + 2*8 + 4*8 + 8*8
    assert [int(v) for v in offsets] == [getattr(ct, f).offset for f, *_ in ct._fields_]
    names = ('nxc_shell_set', 'nxc_shell_accumulate', 'nxc_shell_accumulate_f32',
             'nxc_shell_accumulate_rows', 'nxc_shell_download')
    assert all(name in hip_api.EXPORTS for name in names)
    lib = hip_api.load_library()
    assert all(hasattr(lib, name) for name in names)
    assert lib.nxc_abi_version() == hip_api.ABI_VERSION == 3
    with open(HEADER) as f:
        header = f.read()
    assert 'ShellMap' in header and all(f'int {name}(' in header for name in names)
