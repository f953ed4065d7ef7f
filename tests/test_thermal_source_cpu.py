"""Thermal launch speeds on the host ('maxwellian' at temperature 0: a Maxwellian flux at the local
surface temperature): the host sampler by construction, the v(T, p) table independent of the
surface interaction, the surface temperature pinned to the reference
(tests/golden/g11_surface_temperature.npz, made by tests/tools/make_surface_temperature_golden.py),
refusals, and the statistical law at the seeds the GPU tests use."""
import os

import numpy as np
import pytest
from scipy import stats

from nexoclom_amd import Input, Output
from nexoclom_amd.source_distribution import WindowGenerator
from nexoclom_amd.surface import (SurfaceInteraction, day_side_t1, spline_tables,
                                  surface_temperature, thermal_launch_spline)

from . import thermal_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THERMAL_INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.thermal.input')
IO_INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.io.torus.input')
GOLDEN = os.path.join(HERE, 'golden', 'g11_surface_temperature.npz')
P_MIN = 1e-3
ESCAPE_KMS = 4.25             # Mercury's escape speed at the surface

# seeds and size of the statistical tests (the GPU tests draw the device's packets with these)
LAW_SEED, LAW_N = 8080, 200000


def thermal_input(tmp_path, extra=''):
    """The thermal example input with lines appended (later lines override earlier ones)."""
    path = tmp_path / f'thermal{len(list(tmp_path.iterdir()))}.input'
    path.write_text(open(THERMAL_INPUT).read() + '\n' + extra + '\n')
    return Input(str(path))


def bare_output(inputs):
    """An Output as far as source_desc() needs one (the descriptor is built before any GPU call)."""
    run = Output.__new__(Output)
    run.inputs, run.unit_km, run.planet = inputs, 2440.53, inputs.geometry.planet
    return run


def host_x0(inputs, n, seed, **kw):
    return Output(inputs, n, seed=seed, integrate=False, save=False, **kw).X0


# ---- 1. the host sampler, by construction -------------------------------------------------------------
@pytest.mark.parametrize('step_size', [30, 0])
def test_host_sampler_draws_thermal_speeds_by_construction(tmp_path, step_size):
    """X0.v equals max(S(T, u), 0) / unit_km bit for bit, S built here the reference's way, T the
    surface temperature at the drawn point and u the seeded vector in the speed slot: the draw
    order is [time] sin(latitude), longitude, speed, sin(altitude), azimuth, each a whole vector."""
    inputs = thermal_input(tmp_path, f'options.step_size = {step_size}')
    n, seed = 5000, 91
    X0 = host_x0(inputs, n, seed)
    rng = np.random.default_rng(seed)
    draws = rng.random((6 if step_size == 0 else 5, n))
    if step_size == 0:
        np.testing.assert_array_equal(X0.time.values, draws[0]*inputs.options.endtime.value)
        draws = draws[1:]
    u_lat, u_lon, u_speed, u_alt, u_az = draws
    np.testing.assert_array_equal(X0.latitude.values, np.arcsin(-1.0 + 2.0*u_lat))
    np.testing.assert_array_equal(X0.longitude.values, (0.0 + 2*np.pi*u_lon) % (2*np.pi))
    np.testing.assert_array_equal(X0.altitude.values, np.arcsin(u_alt*1.0))
    np.testing.assert_array_equal(X0.azimuth.values, 2*np.pi*u_az)
    S = R.reference_spline(float(inputs.geometry.taa), 'Na')
    T = surface_temperature(inputs.geometry, X0.longitude.values, X0.latitude.values)
    unit_km = inputs.geometry.planet.radius.value
    expected = np.maximum(S.ev(T, u_speed), 0.0)
    assert np.array_equal(X0.v.values, expected/unit_km)
    assert (T == 100.).any() and (T > 600.).any()


def test_a_window_equals_the_slice_of_the_whole_draw(tmp_path):
    inputs = thermal_input(tmp_path)
    assert WindowGenerator.windowable(inputs)
    n, a, b = 3000, 1234, 2500
    whole = host_x0(inputs, n, 5)
    part = host_x0(inputs, n, 5, window=(n, a, b))
    cols = ['x', 'y', 'z', 'vx', 'vy', 'vz', 'v', 'longitude', 'latitude']
    assert np.array_equal(part[cols].values, whole[cols].values[a:b])


# ---- 2. the table does not depend on the surface interaction ------------------------------------------
@pytest.mark.parametrize('interaction', [
    'surfaceinteraction.stickcoef = 1.',
    'surfaceinteraction.stickcoef = 0.5\nsurfaceinteraction.accomfactor = 0',
    'surfaceinteraction.sticktype = temperature dependent\nsurfaceinteraction.accomfactor = 0.2'])
def test_thermal_speeds_do_not_depend_on_the_surface_interaction(tmp_path, interaction):
    plain = host_x0(thermal_input(tmp_path), 4000, 17)
    other = host_x0(thermal_input(tmp_path, interaction), 4000, 17)
    assert np.array_equal(plain.v.values, other.v.values)


@pytest.mark.parametrize('infile', ['Bounce.const.input', 'Bounce.tempdep.input'])
def test_re_emission_spline_is_the_reference_construction_bit_for_bit(infile):
    inputs = Input(os.path.join(HERE, 'inputfiles', infile))
    assert inputs.surfaceinteraction.accomfactor != 0
    surf = SurfaceInteraction(inputs)
    ref = R.reference_spline(float(inputs.geometry.taa), inputs.options.species)
    for mine, theirs in zip(surf.spline.tck, ref.tck):
        assert np.array_equal(mine, theirs)
    for mine, theirs in zip(surf.bounce_tables(), R.tables(ref)):
        assert np.array_equal(mine, theirs)
    # and the launch source's table is the same spline
    for mine, theirs in zip(spline_tables(thermal_launch_spline(inputs)), R.tables(ref)):
        assert np.array_equal(mine, theirs)


def test_the_table_is_built_once_per_input(tmp_path):
    inputs = thermal_input(tmp_path)
    first = thermal_launch_spline(inputs)
    host_x0(inputs, 100, 1)
    bare_output(inputs).source_desc()
    assert thermal_launch_spline(inputs) is first


# ---- 3. the surface temperature, pinned to the reference -----------------------------------------------
def test_surface_temperature_equals_the_reference_bit_for_bit():
    with np.load(GOLDEN) as g:
        golden = {k: g[k] for k in g.files}
    inputs = Input(THERMAL_INPUT)
    lon, lat = golden['longitude'], golden['latitude']
    for taa, expected in zip(golden['taa'], golden['temperature']):
        inputs.geometry.taa = type(inputs.geometry.taa)(float(taa), 'rad')
        assert float(inputs.geometry.taa) == taa
        got = surface_temperature(inputs.geometry, lon, lat)
        assert np.array_equal(got, expected)
        assert np.array_equal(R.reference_temperature(taa, lon, lat), expected)
    for edge in (np.pi/2, 3*np.pi/2, 0.0, 2*np.pi):
        assert np.any(lon == edge)
    assert np.any(lat == np.pi/2) and np.any(lat == -np.pi/2)


# ---- 4. refusals ------------------------------------------------------------------------------------
def io_thermal(tmp_path):
    lines = [line for line in open(IO_INPUT) if not line.casefold().startswith('speeddist.')]
    lines += ['SpeedDist.type = maxwellian\n', 'SpeedDist.temperature = 0\n']
    path = tmp_path / 'io_thermal.input'
    path.write_text(''.join(lines))
    return Input(str(path))


def test_no_surface_temperature_off_mercury(tmp_path):
    inputs = io_thermal(tmp_path)
    with pytest.raises(NotImplementedError):
        Output(inputs, 100, seed=1, integrate=False, save=False)
    with pytest.raises(NotImplementedError):
        bare_output(inputs).source_desc()


def test_source_desc_of_the_thermal_source():
    inputs = Input(THERMAL_INPUT)
    src = bare_output(inputs).source_desc()
    assert src['speed_type'] == 3 and src['spatial_type'] == 0
    assert src['t0'] == 100. and src['t1'] == day_side_t1(inputs.geometry)
    tx, ty, coef = src['thermal_spline']
    assert len(tx) == 205 and len(ty) == 105 and coef.shape == (201, 101)
    assert 'speed_table' not in src


# ---- 6. the law, at the GPU tests' seeds -----------------------------------------------------------------
def test_the_table_is_monotone_in_p_and_bounded():
    inputs = Input(THERMAL_INPUT)
    S = thermal_launch_spline(inputs)
    assert R.nondecreasing_in_p(S)
    _, _, coef = spline_tables(S)
    # the night row tops out at 3 v_th(100 K), far below the escape speed
    night_max = float(np.max(S.ev(np.full(10001, 100.), np.linspace(0, 1, 10001))))
    print(f'S(100 K, 1) = {night_max:.4f} km/s, max |coef| = {np.abs(coef).max():.4f} km/s')
    assert 0.80 < night_max < 0.82 and night_max < ESCAPE_KMS
    assert np.abs(coef).max() < 2.1


def law_checks(inputs, lon, lat, speed):
    """The five KS tests of the recovered uniforms, and the two checks of the law's shape; used
    for the host's packets here and the device's in tests/test_gpu_thermal_source.py."""
    S = thermal_launch_spline(inputs)
    T = surface_temperature(inputs.geometry, lon, lat)
    pvalues, groups = R.law_pvalues(S, R.NIGHT_K, T, speed)
    print('KS p-values of the recovered uniforms:', pvalues)
    for name, p in pvalues.items():
        assert p >= P_MIN, f'{name}: p = {p}'
    means = [speed[groups[k]].mean() for k in ('night', 'day low', 'day mid', 'day high')]
    print('mean speeds night / day terciles [km/s]:', means)
    assert means[0] < means[1] < means[2] < means[3]
    night = speed[groups['night']]
    fresh = np.maximum(S.ev(np.full(len(night), R.NIGHT_K),
                            np.random.default_rng(1).random(len(night))), 0.0)
    p_row = stats.ks_2samp(night, fresh).pvalue
    lag = np.corrcoef(night[:-1], night[1:])[0, 1]
    print(f'night side: KS against the T = t0 row p = {p_row:.4f}, lag-1 correlation {lag:.2e}')
    assert p_row >= P_MIN
    assert abs(lag) < 4/np.sqrt(len(night))


def test_host_packets_follow_the_law_at_the_gpu_seeds():
    inputs = Input(THERMAL_INPUT)
    X0 = host_x0(inputs, LAW_N, LAW_SEED)
    law_checks(inputs, X0.longitude.values, X0.latitude.values,
               X0.v.values*inputs.geometry.planet.radius.value)


def test_restatement_sensitivity_bound():
    """The tolerance of the device speeds against tests/thermal_restatement.py (GPU test 5): the
    largest relative change of v when cos(lon), cos(lat) or the latitude move by one ulp, over the
    GPU test's packets, times 4.  Measured: 4.15e-15 at seed 77 (2e5 uniform packets), so the
    bound is 1.66e-14.  FITPACK's .ev and the de Boor restatement agree exactly (0.0) over 1e6
    random (T, p); the host's x**0.25 against the device's sqrt(sqrt(x)) moves v by 9.7e-16."""
    inputs = Input(THERMAL_INPUT)
    src = bare_output(inputs).source_desc()
    lon, lat, u = R.launch(LAW_N, 77, spatial_type=0)
    sens = R.speed_ulp_sensitivity(lon, lat, u, src['t0'], src['t1'], src['thermal_spline'])
    print(f'1-ulp sensitivity of v: {sens:.3e}')
    assert 0 < sens < 1e-13
    rng = np.random.default_rng(6)
    T = 100 + rng.random(1000000)*src['t1']
    p = rng.random(1000000)
    S = thermal_launch_spline(inputs)
    diff = np.max(np.abs(S.ev(T, p) - R.bispev3(*src['thermal_spline'], T, p)))
    print(f'FITPACK against de Boor: {diff:.3e} km/s')
    assert diff <= 1e-15
