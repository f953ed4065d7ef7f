"""ShellMap moments without a GPU: the definition (tests/shell_moments_restatement.py, written from
include/nexoclom_hip.h, "ShellMap moments") on flows with closed forms; what ShellMap publishes from
the sums (shell_moments_from_sums) against hand calculations; the ``moments=`` keyword and the
unchanged refusals; the ctypes signatures of the new exports; the host-only checks of the new
entries as a stand-alone program, plain and under the host sanitizers."""
import contextlib
import io
import os
import subprocess

import numpy as np
import pytest

from nexoclom_amd import constants as const
from nexoclom_amd.ModelDensity import moments_from_sums
from nexoclom_amd.ShellMap import SHELL_MOMENT_COLUMNS, shell_axes, shell_moments_from_sums
from tests import shell_moments_restatement as R
from tests.shell_moments_restatement import local_velocity, shell_moments
from tests.test_shell_map_cpu import GOOD, HEADER, HERE, cloud, make_inputs

MASS_NA = 22.98976928*const.AMU
GRID, ALT = (12, 7), (1.0, 4.5, 5)              # cloud() reaches from 1 to 4 radii: all inside


def restate(cols7, grid=GRID, alt=ALT, quantity='column'):
    return shell_moments(*cols7, 2e-4, quantity, [], *grid, *alt)


def flow(n, seed, velocity):
    """cloud()'s positions and fractions with the velocity field ``velocity(x, y, z)`` [R/s]"""
    x, y, z, _, frac = cloud(n, seed)
    vx, vy, vz = velocity(x, y, z)
    return x, y, z, vx, vy, vz, frac


def published(res, grid=GRID, alt=ALT, app=1.0, unit_km=1.0, quantity='column'):
    axes = shell_axes(*grid, alt[0] - 1.0, alt[1] - 1.0, alt[2])
    return shell_moments_from_sums(res.sums, res.moments, app, axes['volume'], axes['r_edges'],
                                   unit_km, MASS_NA, quantity), axes


def column(res, name):
    """The sum ``name`` of SHELL_MOMENT_COLUMNS per cell and altitude record"""
    k = SHELL_MOMENT_COLUMNS.index(name)
    return res.moments[k // 2, ..., k % 2]


def test_the_columns_are_the_planes_in_order():
    assert SHELL_MOMENT_COLUMNS == R.SHELL_MOMENT_COLUMNS and len(SHELL_MOMENT_COLUMNS) == 12
    assert SHELL_MOMENT_COLUMNS[:2] == ('ur', 'ue') and SHELL_MOMENT_COLUMNS[-3:] == ('up', 'upup', 'dndn')


# ---- 1. flows with closed forms ---------------------------------------------------------------------
def test_radial_outflow():
    """v = v0 r^: no east or north component, everything goes up, and no spread within a cell."""
    v0 = 2.0/2440.53

    def radial(x, y, z):
        r = np.sqrt(x*x + y*y + z*z)
        return v0*x/r, v0*y/r, v0*z/r
    cols = flow(20000, 3, radial)
    res = restate(cols)
    sw = res.sums[0, ..., 0].sum()
    assert res.binned == 20000 and sw > 5000
    assert abs(column(res, 'ue').sum()) <= 1e-12*v0*sw and abs(column(res, 'un').sum()) <= 1e-12*v0*sw
    assert np.abs(column(res, 'ue')).max() <= 1e-12*v0*sw
    assert np.array_equal(column(res, 'up'), column(res, 'ur'))
    assert not column(res, 'dndn').any()
    np.testing.assert_allclose(column(res, 'ur').sum(), v0*sw, rtol=1e-12)
    out, _ = published(res, unit_km=2440.53)
    filled = res.sums[0, ..., 1:-1, 0] > 0
    assert filled.sum() > 300
    np.testing.assert_allclose(out['velocity'][filled][:, 0], 2.0, rtol=1e-12)
    thermal = MASS_NA*2.0**2*1e6/(3*const.K_B)                  # m v0^2 / (3 k_B) [K]
    assert thermal > 1000 and np.abs(out['temperature'][filled]).max() <= 1e-11*thermal
    assert np.isnan(out['temperature'][~filled]).all() and np.isnan(out['velocity'][~filled]).all()


def test_rigid_rotation():
    """v = Omega z^ x x: v_e = Omega rho, nothing radial or northward."""
    omega = 3e-4
    x, y, z, vx, vy, vz, _ = flow(5000, 4, lambda x, y, z: (-omega*y, omega*x, 0.0*z))
    v_r, v_e, v_n, p2 = local_velocity(x, y, z, vx, vy, vz)
    r = np.sqrt(p2 + z*z)
    np.testing.assert_allclose(v_e, omega*np.sqrt(p2), rtol=1e-14)
    assert np.abs(v_r).max() <= 1e-15*omega*r.max() and np.abs(v_n).max() <= 1e-15*omega*r.max()


def random_flow(n, seed):
    rng = np.random.default_rng(seed + 1000)
    return flow(n, seed, lambda x, y, z: tuple(rng.normal(size=len(x))*1e-3 + b
                                               for b in (2e-4, -5e-4, 3e-4)))


def test_the_basis_is_orthonormal():
    """v_r^2 + v_e^2 + v_n^2 = |v|^2 per sample, and the diagonal sums of planes 1 and 2 total
    sum w |v|^2."""
    cols = random_flow(20000, 5)
    x, y, z, vx, vy, vz, frac = cols
    v_r, v_e, v_n, _ = local_velocity(x, y, z, vx, vy, vz)
    speed2 = vx*vx + vy*vy + vz*vz
    np.testing.assert_allclose(v_r*v_r + v_e*v_e + v_n*v_n, speed2, rtol=1e-14)
    res = restate(cols)
    assert res.binned == 20000
    diagonal = column(res, 'urr').sum() + column(res, 'uee').sum() + column(res, 'unn').sum()
    np.testing.assert_allclose(diagonal, (frac*speed2).sum(), rtol=1e-12)


def test_up_less_down_is_net():
    """sum up - sum dn = sum u_r, sample by sample: one sample on a 1 x 1 x 1 grid each, where the
    sum of dn is the root of the sum of dn^2."""
    cols = random_flow(64, 6)
    signs = set()
    for k in range(64):
        res = restate(tuple(c[k:k + 1] for c in cols), grid=(1, 1), alt=(1.0, 4.5, 1))
        assert res.binned == 1
        ur, up, dn = (column(res, n)[0, 0, 1] for n in ('ur', 'up', 'dndn'))
        dn = np.sqrt(dn)
        np.testing.assert_allclose(up - dn, ur, rtol=1e-15)
        assert (up == 0) != (dn == 0) and column(res, 'upup')[0, 0, 1] == up*up
        signs.add(ur > 0)
    assert signs == {True, False}


def test_temperature_is_the_cartesian_one():
    """A cell whose samples share one direction shares one basis, and the trace of the covariance
    does not depend on the basis: the temperature equals ModelDensity.moments_from_sums' on the
    Cartesian sums of the same samples.  (Samples of different directions have different bases: for
    them the two differ by design -- radial outflow is cold here and hot in Cartesian terms.)"""
    rng = np.random.default_rng(7)
    n, grid, alt = 400, (4, 2), (1.0, 4.5, 1)
    lon, mu = np.array([0.3, 2.0, 3.5, 5.5]), np.array([-0.4, 0.6, 0.2, -0.7])
    which = rng.integers(0, 4, n)
    r = rng.uniform(1.1, 4.4, n)
    rho = np.sqrt(1 - mu*mu)
    d = np.stack([rho*np.sin(lon), -rho*np.cos(lon), mu], axis=1)[which]
    x, y, z = (r*d[:, k] for k in range(3))
    v = rng.normal(size=(n, 3))*1e-3 + np.array([2e-4, -5e-4, 3e-4])
    w = rng.uniform(0.1, 1.0, n)
    res = restate((x, y, z, v[:, 0], v[:, 1], v[:, 2], w), grid, alt)
    out, _ = published(res, grid, alt, unit_km=2440.53)
    assert res.binned == n and np.count_nonzero(res.counts) == 4
    for k in range(4):
        m = which == k
        ix, iz = int(lon[k]//(np.pi/2)), int(mu[k] > 0)
        assert res.counts[ix, iz] == m.sum() > 50
        pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
        ten = [(w[m]*v[m, a]).sum() for a in range(3)] + \
              [(w[m]*v[m, a]*v[m, b]).sum() for a, b in pairs] + [(w[m]*w[m]).sum()]
        _, _, want, _ = moments_from_sums([w[m].sum()], [ten], 2440.53, MASS_NA)
        assert want[0] > 100
        np.testing.assert_allclose(out['temperature'][ix, iz, 0], want[0], rtol=1e-9)


def test_samples_on_the_axis_add_no_moments():
    """x = y = 0 exactly: east and north are 0/0.  The sample is in plane A and in no moment plane."""
    cols = [c.copy() for c in random_flow(500, 8)]
    on_axis = np.arange(0, 500, 5)
    cols[0][on_axis] = cols[1][on_axis] = 0.0
    res = restate(tuple(cols))
    rest = restate(tuple(np.delete(c, on_axis) for c in cols))
    assert res.binned == 500 and rest.binned == 400
    assert res.sums[0, ..., 0].sum() > rest.sums[0, ..., 0].sum()
    assert np.array_equal(res.moments, rest.moments) and np.isfinite(res.moments).all()
    assert np.array_equal(res.abs_moments, rest.abs_moments)
    alone = restate(tuple(c[:1] for c in cols), grid=(1, 1), alt=(1.0, 4.5, 1))
    assert alone.sums[0, 0, 0, 1, 0] == cols[6][0] and not alone.moments.any()


def test_nonfinite_velocities_reach_their_record():
    cols = [c.copy() for c in random_flow(300, 9)]
    cols[3][17] = np.nan                                          # vx
    cols[5][40] = np.inf                                          # vz
    res = restate(tuple(cols))
    assert res.nonfinite == 0 and res.binned == 300
    assert np.isnan(column(res, 'ur')).sum() == 1 and np.isinf(column(res, 'ur')).sum() == 1
    assert np.isfinite(res.sums).all()
    cols[4][17] = np.nan                                          # vy: dropped through radvel
    again = restate(tuple(cols))
    assert again.nonfinite == 1 and not np.isnan(again.moments).any()


# ---- 2. what ShellMap publishes ------------------------------------------------------------------------
def test_flux_and_rate_of_one_sample():
    """One packet of weight w moving up at v: the hand calculation of the flux through its cell and
    of the rate through its shell."""
    w, v_kms, unit_km, app = 0.37, 1.5, 2440.53, 3.7e21
    grid, alt = (8, 4), (1.0, 3.0, 4)
    v = v_kms/unit_km                                              # R/s
    pos = np.array([0.5, -2.0, 1.0])
    r = np.sqrt((pos*pos).sum())
    vel = v*pos/r
    res = restate(tuple(np.array([c]) for c in (*pos, *vel, w)), grid, alt)
    out, axes = published(res, grid, alt, app, unit_km)
    ix, iz = np.argwhere(res.counts)[0]
    k = int((r - 1.0)*2.0)
    R_cm = unit_km*1e5
    volume_R3 = axes['solid_angle']*(axes['r_edges'][k + 1]**3 - axes['r_edges'][k]**3)/3
    # density [cm^-3] times speed [cm/s]
    want = app*w/(volume_R3*R_cm**3)*(v_kms*1e5)
    np.testing.assert_allclose(out['flux_up'][ix, iz, k], want, rtol=1e-13)
    np.testing.assert_allclose(out['flux_net'][ix, iz, k], want, rtol=1e-13)
    assert out['flux_down'][ix, iz, k] == 0 and np.count_nonzero(out['flux_up']) == 1
    np.testing.assert_allclose(out['flux_up_effective_packets'][ix, iz, k], 1.0, rtol=1e-14)
    assert not out['flux_down_effective_packets'].any()
    # atoms crossing the shell per second: the packet's atoms spend dr / v seconds in it
    dr_cm = 0.5*R_cm
    np.testing.assert_allclose(out['shell_rate_up'][k], app*w*(v_kms*1e5)/dr_cm, rtol=1e-13)
    np.testing.assert_allclose(out['shell_rate_net'], out['shell_rate_up'] - out['shell_rate_down'],
                               rtol=1e-13)
    assert np.count_nonzero(out['shell_rate_up']) == 1 and not out['shell_rate_down'].any()
    np.testing.assert_allclose(out['velocity'][ix, iz, k], [v_kms, 0, 0], rtol=1e-13, atol=1e-13)
    # and falling: the same numbers in flux_down
    res = restate(tuple(np.array([c]) for c in (*pos, *(-vel), w)), grid, alt)
    out, _ = published(res, grid, alt, app, unit_km)
    np.testing.assert_allclose(out['flux_down'][ix, iz, k], want, rtol=1e-13)
    np.testing.assert_allclose(out['flux_net'][ix, iz, k], -want, rtol=1e-13)
    assert not out['flux_up'].any()
    np.testing.assert_allclose(out['flux_down_effective_packets'][ix, iz, k], 1.0, rtol=1e-14)


def test_shell_rate_of_a_radial_wind():
    """Unit weights moving out at v0: the rate through shell k is atoms_per_packet n_k v0 / dr."""
    v0, app = 1e-3, 2.5e20

    def radial(x, y, z):
        r = np.sqrt(x*x + y*y + z*z)
        return v0*x/r, v0*y/r, v0*z/r
    cols = list(flow(20000, 10, radial))
    cols[6] = np.ones(20000)
    res = restate(tuple(cols))
    out, axes = published(res, app=app)
    n_k = res.sums[0, ..., 1:-1, 0].sum(axis=(0, 1))
    assert n_k.sum() == 20000 and n_k.min() > 1000
    np.testing.assert_allclose(out['shell_rate_up'], app*n_k*v0/np.diff(axes['r_edges']), rtol=1e-12)
    assert not out['shell_rate_down'].any()
    np.testing.assert_allclose(out['flux_up_effective_packets'], res.sums[0, ..., 1:-1, 0], rtol=1e-12)


def test_radiance_publishes_no_fluxes():
    res = restate(random_flow(2000, 11))
    out, _ = published(res, quantity='radiance')
    assert out['velocity'].shape == GRID + (ALT[2], 3)
    assert out['velocity_covariance'].shape == GRID + (ALT[2], 3, 3)
    for name in ('flux_up', 'flux_down', 'flux_net', 'flux_up_effective_packets',
                 'flux_down_effective_packets', 'shell_rate_up', 'shell_rate_down', 'shell_rate_net'):
        assert out[name] is None
    column_out, _ = published(res)
    assert column_out['flux_up'].shape == GRID + (ALT[2],) and column_out['shell_rate_up'].shape == (ALT[2],)
    cov = column_out['velocity_covariance']
    filled = res.sums[0, ..., 1:-1, 0] > 0
    assert np.array_equal(cov[filled], np.swapaxes(cov, -1, -2)[filled])


# ---- 3. the class ------------------------------------------------------------------------------------------
def build(params, **kw):
    from nexoclom_amd import ShellMap
    with contextlib.redirect_stdout(io.StringIO()):
        return ShellMap(make_inputs(), params, context=object(), **kw)


def test_the_moments_keyword():
    plain = build(GOOD)
    assert plain.moments is False and not hasattr(plain, 'shell_moment_sums')
    assert not hasattr(plain, 'velocity')
    sm = build(GOOD, moments=True)
    assert sm.moments is True and sm.shell_moment_sums.shape == (6, 8, 6, 6, 2)
    assert sm.velocity.shape == (8, 6, 4, 3) and np.isnan(sm.velocity).all()
    assert sm.velocity_covariance.shape == (8, 6, 4, 3, 3) and sm.temperature.shape == (8, 6, 4)
    assert sm.flux_up.shape == sm.flux_down.shape == sm.flux_net.shape == (8, 6, 4)
    assert sm.shell_rate_up.shape == sm.shell_rate_down.shape == sm.shell_rate_net.shape == (4,)
    assert not sm.flux_up_effective_packets.any() and not sm.flux_down_effective_packets.any()
    assert np.array_equal(sm.density, plain.density) and np.array_equal(sm.shell_sums, plain.shell_sums)
    emission = build(dict(GOOD, quantity='radiance'), moments=True)
    assert emission.flux_up is None and emission.shell_rate_net is None
    assert emission.temperature.shape == (8, 6, 4)


@pytest.mark.parametrize('kw', [dict(npackets=1000), dict(cp=object()), dict(shard=(0, 10))])
def test_the_refusals_stay(kw):
    with pytest.raises(NotImplementedError):
        build(GOOD, moments=True, **kw)
    with pytest.raises(TypeError):
        build(GOOD, moments=True, no_such_keyword=1)
    with pytest.raises(NotImplementedError):
        build(dict(GOOD, origin='Io'), moments=True)       # Io takes no part in this run


# ---- 4. the C side ---------------------------------------------------------------------------------------
def test_signatures_of_the_new_exports():
    import ctypes as C

    from nexoclom_amd import hip_api
    from tests.test_abi import header_signatures
    header = header_signatures(open(HEADER).read())
    names = ['nxc_shell_moments_enable', 'nxc_shell_moments_accumulate',
             'nxc_shell_moments_accumulate_f32', 'nxc_shell_moments_accumulate_rows',
             'nxc_shell_moments_download']
    for name in names:
        assert header[name] == (C.c_int, hip_api.SIGNATURES[name]), name
        assert name in hip_api.EXPORTS
    assert len(hip_api.SIGNATURES['nxc_shell_moments_accumulate']) == 9
    for method in ('shell_moments_enable', 'shell_moments_accumulate', 'shell_moments_download'):
        assert callable(getattr(hip_api.Context, method))


@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_entry_checks_as_a_host_program(tmp_path, flags):
    """The refusals of the shell moments' entries are host-only code
    (nxc_shell_moments_check.hpp); tests/tools/shell_moments_check.cpp feeds it a good state per
    entry and one bad one per refusal.  Built plainly and with the host sanitizers; both runs must
    pass."""
    exe = tmp_path / 'shell_moments_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'shell_moments_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    assert not done.stderr.strip()
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused (' in line]
    assert len(refused) >= 16 and sum(' accepted' in line for line in lines) >= 6
    for word in ('nxc_shell_set has not been called', 'moments not enabled', 'bad arguments', '2^31'):
        assert any(word in line for line in refused), word
    # the set is named before the enable
    stale = [line for line in refused if line.startswith('accumulate, set after an enable')]
    assert len(stale) == 1 and 'nxc_shell_set' in stale[0]
