"""k_shell_moments and ShellMap(moments=True) on the GPU against tests/shell_moments_restatement.py
(the "ShellMap moments" definition of include/nexoclom_hip.h restated with NumPy).  Sample generators,
the row stores and the comparison of the pair and of planes A and B are those of
tests/test_gpu_shell_map.py and tests/test_gpu_pixel_moments.py.

Comparison rule, everywhere, that of tests/test_gpu_shell_map.py: the restatement's three guards are
asserted first (>= 1e-9), then counts and counters must be equal exactly, the column to rtol 1e-11,
every entry of planes A and B and every one of the twelve moment sums to |got - want| <= 1e-11 *
sum |term| per (plane, cell, record, half), and an entry that is NaN in the restatement must be NaN
on the device and no other.  The samples put exactly on the polar axis (x = y = 0) have sin(latitude)
= z / sqrt(z z) = +-1 exactly on either side -- a pole is an edge of the axis, so they are left out
of the guards, and the grid of their case has an odd number of longitude bins, which puts their
longitude pi in the middle of one.

Every case's inputs come from CASES, so that the guards of all of them can be checked without a GPU:
``python -m tests.test_gpu_shell_moments`` restates every case and prints its guards.  The
thresholds themselves, which the guards keep away from, are covered by
tests/test_gpu_shell_thresholds.py, which runs the inputs of tests/threshold_cases.py through
shell_located<ShellHit> as well."""
import contextlib
import io

import numpy as np
import pytest

from nexoclom_amd import Input, Output, ShellMap, hip_api
from nexoclom_amd import constants as const
from nexoclom_amd.atomicdata import atomicmass
from nexoclom_amd.ShellMap import SHELL_MOMENT_COLUMNS, shell_axes, shell_moments_from_sums
from tests import helpers as H
from tests import test_gpu_shell_map as S
from tests.shell_moments_restatement import shell_moments
from tests.test_gpu_pixel_moments import (GUARD, INPUT, R_KM, ROWS_RTOL, RTOL, cloud,  # noqa: F401
                                          forces, store, tables)

pytestmark = pytest.mark.gpu
GRID, ALT = S.GRID, S.ALT


def five(cols):
    return S.five(cols)


def seven(cols5, seed, dtype=np.float64):
    """x y z vx vy vz frac from the five columns of tests/test_gpu_shell_map.py's generators: seeded
    vx and vz of a few km/s"""
    rng = np.random.default_rng(seed)
    x, y, z, vy, frac = cols5
    vx, vz = (np.ascontiguousarray((rng.normal(size=len(x))*2.0/R_KM).astype(dtype)) for _ in range(2))
    return x, y, z, vx, vy, vz, frac


def on_axis(seed, n=192):
    """64 of 192 samples exactly on the polar axis, north and south, mixed into every wave"""
    cols = [c.copy() for c in cloud(n, seed)]
    axis = np.arange(1, n, 3)
    cols[0][axis] = cols[1][axis] = 0.0
    cols[2][axis] = np.where(axis % 2 == 0, 1.0, -1.0)*np.linspace(1.6, 3.9, len(axis))
    return tuple(cols)


def half_zero(seed, n=3001):
    cols = [c.copy() for c in cloud(n, seed)]
    cols[6][::2] = 0.0
    return tuple(cols)


def poisoned(seed, n=2001):
    """A NaN vx, a NaN vz and an infinite vx inside the grid (they reach the sums of their records);
    a NaN vy, a NaN frac and a sample at the centre (dropped, as by k_shell)"""
    cols = [c.copy() for c in cloud(n, seed)]
    cols[3][5] = np.nan
    cols[5][400] = np.nan
    cols[3][900] = np.inf
    cols[4][700] = np.nan
    cols[6][10] = np.nan
    cols[0][1300] = cols[1][1300] = cols[2][1300] = 0.0
    return tuple(cols)


def radial(seed, n=20011, v0=2.0/R_KM):
    x, y, z, _, _, _, frac = cloud(n, seed)
    r = np.sqrt(x*x + y*y + z*z)
    return x, y, z, v0*x/r, v0*y/r, v0*z/r, frac


# name -> (seven columns, g-value tables' kind, (nlon, nlat), (r_lo, r_hi, nalt))
CASES = {f'p{p}': (lambda p=p: (cloud(p, 200 + p), 'two', GRID, ALT))
         for p in (0, 1, 63, 64, 65, 1023, 1025)}
CASES.update({
    'second_trip': lambda: (cloud(1_200_001, 9, np.float32), 'two', (9, 4), (1.5, 4.0, 33)),
    'grid_1x1': lambda: (cloud(5003, 21), 'column', (1, 1), (1.5, 4.0, 1)),
    'grid_37x11': lambda: (cloud(30011, 24), 'two', (37, 11), (1.5, 4.0, 5)),
    'all_below': lambda: (cloud(5003, 31), 'column', GRID, (7.0, 9.0, 4)),
    'all_above': lambda: (seven(S.far_cloud(5003, 32, 2.0, 6.0), 132), 'column', GRID, (1.0, 1.5, 4)),
    'seam_and_poles': lambda: (seven(S.seam_and_poles(41), 141), 'constant', GRID, ALT),
    'one_record': lambda: (seven(S.one_record(42), 142), 'constant', GRID, ALT),
    'on_axis': lambda: (on_axis(43), 'column', (11, 7), ALT),
    'half_zero': lambda: (half_zero(56), 'two', GRID, ALT),
    'poisoned_column': lambda: (poisoned(57), 'column', GRID, ALT),
    'poisoned_radiance': lambda: (poisoned(58), 'two', GRID, ALT),
    'float32': lambda: (cloud(40009, 59, np.float32), 'two', GRID, ALT),
    'first_call': lambda: (cloud(9001, 61), 'two', GRID, ALT),
    'second_call': lambda: (cloud(7001, 62), 'two', GRID, ALT),
    'radial': lambda: (radial(63), 'column', GRID, ALT),
})


def off_axis(cols):
    return (np.asarray(cols[0]) != 0) | (np.asarray(cols[1]) != 0) | (np.asarray(cols[2]) == 0)


def restate(forces, cols, kind, grid, alt, name=''):
    quantity, gt = tables(forces, kind)
    want = shell_moments(*cols, forces.vrplanet, quantity, gt, *grid, *alt)
    guards = want
    keep = off_axis(cols)
    if not keep.all():          # x = y = 0 exactly: sin(latitude) is +-1 exactly, on either side
        x, y, z = (np.asarray(c, dtype=np.float64)[~keep] for c in cols[:3])
        assert np.array_equal(np.abs(z/np.sqrt((x*x + y*y) + z*z)), np.ones(len(z)))
        guards = shell_moments(*(c[keep] for c in cols), forces.vrplanet, quantity, gt, *grid, *alt)
    print(f'{name} guards: edge {guards.edge_guard:.3e} margin {guards.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e}; {want.samples} samples, {want.binned} binned, '
          f'{want.nonfinite} nonfinite, {np.count_nonzero(want.abs_moments[0, ..., 0])} records with moments')
    assert guards.edge_guard >= GUARD and guards.margin_guard >= GUARD and want.bin_guard >= GUARD
    return want


def shell_set(ctx, forces, kind, grid, alt, enable=True):
    S.shell_set(ctx, forces, kind, grid, alt)
    if enable:
        ctx.shell_moments_enable()


def compare_moments(got, want, rtol=RTOL, reference=None):
    """|got - want| <= rtol * sum |term| per entry, NaN where the restatement has NaN and nowhere
    else; the worst ratio per sum is printed."""
    reference = want.moments if reference is None else reference
    assert got.shape == want.moments.shape == (6,) + want.sums.shape[1:]
    assert np.array_equal(np.isnan(got), np.isnan(want.moments))
    assert np.array_equal(np.isnan(reference), np.isnan(want.moments))
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(got - reference)
        same = (got == reference) | np.isnan(want.moments)         # equal infinities included
        ratio = np.where(same, 0.0, np.where(want.abs_moments > 0, err/want.abs_moments, np.inf))
    print('worst |got - want| / sum|term|:',
          {name: float(ratio[k // 2, ..., k % 2].max()) if ratio.size else 0.0
           for k, name in enumerate(SHELL_MOMENT_COLUMNS)})
    assert np.all(same | (err <= rtol*want.abs_moments))


def compare(ctx, want, counters=None):
    S.compare(ctx, want.base, counters)
    moments = ctx.shell_moments_download()
    compare_moments(moments, want)
    return moments


def check(ctx, forces, name):
    cols, kind, grid, alt = CASES[name]()
    want = restate(forces, cols, kind, grid, alt, name)
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_moments_accumulate(*cols)
    compare(ctx, want, ctx.counters())
    return want


def column(moments, name):
    k = SHELL_MOMENT_COLUMNS.index(name)
    return moments[k // 2, ..., k % 2]


# ---- 1. ragged waves and blocks ----------------------------------------------------------------------
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, p):
    want = check(ctx, forces, f'p{p}')
    assert want.binned == p
    if p >= 1023:
        assert np.count_nonzero(column(want.moments, 'un')) > 300


def test_second_trip_of_the_grid_stride_loop(ctx, forces):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    want = check(ctx, forces, 'second_trip')
    assert want.binned == 1_200_001 and np.count_nonzero(column(want.moments, 'ur')) > 1000


# ---- 2. the pairing of lanes, the seam, the axis --------------------------------------------------------
def test_a_whole_wave_in_one_record(ctx, forces):
    """64 samples in one record: lanes l and l + 32 add to the same 16 bytes of all eight planes."""
    want = check(ctx, forces, 'one_record')
    assert want.counts[2, 5] == 64 and want.binned == 64
    assert np.count_nonzero(want.abs_moments[..., 0]) == 6 and want.abs_moments[0, 2, 5, 3, 0] > 0


def test_seam_and_polar_bands(ctx, forces):
    want = check(ctx, forces, 'seam_and_poles')
    assert want.binned == 256 and np.count_nonzero(want.counts) == 4
    assert np.count_nonzero(want.abs_moments[0, ..., 0].sum(-1)) == 4


def test_samples_on_the_axis_add_no_moments(ctx, forces):
    """64 samples with x = y = 0 exactly, spread over the lanes of three waves: they are in the pair
    and in planes A and B, and the moment planes hold what the other 128 samples add."""
    cols, kind, grid, alt = CASES['on_axis']()
    want = check(ctx, forces, 'on_axis')
    keep = off_axis(cols)
    assert (~keep).sum() == 64 and want.binned == 192
    rest = shell_moments(*(c[keep] for c in cols), forces.vrplanet, 'column', [], *grid, *alt)
    assert np.array_equal(want.moments, rest.moments) and np.isfinite(want.moments).all()
    assert want.sums[0, ..., 0].sum() > rest.sums[0, ..., 0].sum()
    assert np.isfinite(ctx.shell_moments_download()).all()


def test_zero_weights_add_nothing(ctx, forces):
    """Every second frac zero: those lanes are counted and add to no plane; the sums are those of
    the other samples alone."""
    cols = CASES['half_zero']()[0]
    want = check(ctx, forces, 'half_zero')
    lit = shell_moments(*(c[1::2] for c in cols), forces.vrplanet, *tables(forces, 'two'), *GRID, *ALT)
    assert np.array_equal(want.moments, lit.moments) and want.counts.sum() == 2*lit.binned + 1
    # and a pass in which no lane of any wave files anything leaves the planes as they are
    before = ctx.shell_moments_download()
    dark = tuple(c[::2][:640] for c in cols)
    ctx.shell_moments_accumulate(*dark)
    assert ctx.counters()['samples_binned'] == 640
    assert np.array_equal(ctx.shell_moments_download(), before)


@pytest.mark.parametrize('name', ['poisoned_column', 'poisoned_radiance'])
def test_poisoned_inputs(ctx, forces, name):
    """NaN and infinite vx and vz reach the sums of their records and no other; a NaN vy, a NaN frac
    and a sample at the centre are dropped as k_shell drops them."""
    cols = CASES[name]()[0]
    want = check(ctx, forces, name)
    assert want.nonfinite == 2 and want.binned == len(cols[0]) - 3
    assert np.isfinite(want.sums).all()
    if name == 'poisoned_column':
        assert np.isnan(column(want.moments, 'ur')).any() and np.isinf(column(want.moments, 'ur')).any()
        assert np.isnan(column(want.moments, 'up')).sum() == 0


# ---- 3. grids, the altitude axis, widths ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['grid_1x1', 'grid_37x11'])
def test_grids(ctx, forces, name):
    want = check(ctx, forces, name)
    assert want.counts.all() and want.binned == want.samples


@pytest.mark.parametrize('name', ['all_below', 'all_above'])
def test_altitude_axis(ctx, forces, name):
    want = check(ctx, forces, name)
    filled = want.abs_moments[0, ..., 0] > 0
    record = 0 if name == 'all_below' else -1
    assert filled[..., record].all() and filled.sum() == filled[..., record].sum()


def test_float32_columns(ctx, forces):
    want = check(ctx, forces, 'float32')
    assert want.binned == want.samples and np.count_nonzero(column(want.moments, 'uen')) > 300


@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, forces, store, part):
    """Rows in HBM (float32 and 64-bit stores) against the same rows sent from the host and against
    the restatement."""
    st, rows = store
    first, count = (0, st.total) if part == 'whole' else (777, st.total - 777 - 999)
    cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (1, 2, 3, 4, 5, 6, 7))
    alt = (1.25, 7.25, 12)
    want = restate(forces, cols, 'two', GRID, alt, f'rows {part}')
    assert want.binned > 1000
    shell_set(ctx, forces, 'two', GRID, alt)
    ctx.shell_moments_accumulate(*cols)
    host = compare(ctx, want, ctx.counters())
    shell_set(ctx, forces, 'two', GRID, alt)
    ctx.shell_moments_accumulate(rows=(st, first, count))
    got = compare(ctx, want, ctx.counters())
    compare_moments(got, want, rtol=ROWS_RTOL, reference=host)


# ---- 4. state ---------------------------------------------------------------------------------------------
def test_two_calls_sum_an_enable_zeroes_and_a_set_switches_off(ctx, forces):
    a, kind, grid, alt = CASES['first_call']()
    b = CASES['second_call']()[0]
    want_a = restate(forces, a, kind, grid, alt, 'first')
    want = restate(forces, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), kind, grid, alt, 'both')
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_moments_accumulate(*a)
    compare(ctx, want_a, ctx.counters())
    ctx.shell_moments_accumulate(*b)
    compare(ctx, want)
    ctx.shell_moments_accumulate(*(c[:0] for c in a))            # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0
    compare(ctx, want)
    ctx.shell_moments_enable()                                   # an enable zeroes the six planes only
    assert not ctx.shell_moments_download().any()
    S.compare(ctx, want.base)
    shell_set(ctx, forces, kind, grid, alt, enable=False)        # a set switches the moments off
    for call in (ctx.shell_moments_download, lambda: ctx.shell_moments_accumulate(*a)):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'moments not enabled' in str(err.value)
    assert not any(part.any() for part in ctx.shell_download())  # the refused call added nothing
    ctx.shell_moments_enable()
    ctx.shell_moments_accumulate(*a)
    compare(ctx, want_a, ctx.counters())
    ctx.shell_moments_enable(False)
    with pytest.raises(hip_api.HipError, match='moments not enabled'):
        ctx.shell_moments_download()


def test_before_the_set_the_set_is_named():
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for call in (fresh.shell_moments_enable, fresh.shell_moments_download,
                     lambda: fresh.shell_moments_accumulate(x, x, x, x, x, x, x)):
            with pytest.raises(hip_api.HipError) as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE and 'nxc_shell_set' in str(err.value)


def test_bad_arguments(ctx, forces):
    import ctypes as C
    shell_set(ctx, forces, 'column', (5, 3), (1.0, 3.0, 4))
    ctx.shell_moments_accumulate(*cloud(2001, 71))
    before = ctx.shell_moments_download()
    assert before.any() and before.shape == (6, 5, 3, 6, 2)
    entry = ctx.lib.nxc_shell_moments_accumulate
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), *[p]*7) == hip_api.NXC_ERR_ARG
    for hole in range(7):
        args = [p]*7
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*7) == 0
    assert ctx.lib.nxc_shell_moments_download(ctx._h, None) == hip_api.NXC_ERR_ARG
    assert np.array_equal(ctx.shell_moments_download(), before)


def test_the_plain_pass_on_the_same_handle(ctx, forces):
    """With the moments enabled, nxc_shell_accumulate still gives k_shell's result and leaves the
    six planes alone; the two passes give the same pair and planes A and B."""
    cols, kind, grid, alt = CASES['first_call']()
    want = restate(forces, cols, kind, grid, alt, 'plain pass')
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_accumulate(*five(cols))
    plain = S.compare(ctx, want.base, ctx.counters())
    assert not ctx.shell_moments_download().any()
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_moments_accumulate(*cols)
    compare(ctx, want, ctx.counters())
    both = ctx.shell_download()
    assert np.array_equal(both[1], plain[1])
    np.testing.assert_allclose(both[0], plain[0], rtol=RTOL, atol=0)
    S.compare_planes(both[2], want.base, reference=plain[2])


# ---- 5. a flow with a closed form, through the kernel ------------------------------------------------------
def test_radial_outflow(ctx, forces):
    """v = v0 r^: nothing east or north, everything goes up, no spread within a cell."""
    v0 = 2.0/R_KM
    want = check(ctx, forces, 'radial')
    got = ctx.shell_moments_download()
    _, _, sums = ctx.shell_download()
    sw = sums[0, ..., 0].sum()
    assert want.binned == 20011 and sw > 5000
    for name in ('ue', 'un'):
        assert abs(column(got, name).sum()) <= 1e-12*v0*sw
    np.testing.assert_allclose(column(got, 'ur').sum(), v0*sw, rtol=1e-12)
    assert not column(got, 'dndn').any()
    assert np.all(np.abs(column(got, 'up') - column(got, 'ur')) <= RTOL*column(want.abs_moments, 'ur'))
    axes = shell_axes(*GRID, ALT[0] - 1, ALT[1] - 1, ALT[2])
    mass = atomicmass('Na').value*const.AMU
    out = shell_moments_from_sums(sums, got, 1.0, axes['volume'], axes['r_edges'], R_KM, mass)
    filled = sums[0, ..., 1:-1, 0] > 0
    thermal = mass*2.0**2*1e6/(3*const.K_B)
    assert filled.sum() > 300 and np.abs(out['temperature'][filled]).max() <= 1e-11*thermal
    np.testing.assert_allclose(out['velocity'][filled][:, 0], 2.0, rtol=1e-12)
    assert np.array_equal(out['flux_down_effective_packets'], np.zeros(GRID + (ALT[2],)))


# ---- 6. the public class ------------------------------------------------------------------------------------
def restate_outputs(outs, sm, quantity, grid, alt_edges, nalt, columns):
    """The restatement over the samples ``columns(out)`` of every Output, summed: (moments, sum |term|
    of the moments, the ShellResult of the sums)"""
    total = None
    for out in outs:
        vr, gt = float(out.vrplanet)/sm.unit_km, sm.g_tables(float(out.aplanet))
        res = shell_moments(*columns(out), vr, quantity, gt, *grid, alt_edges[0], alt_edges[-1], nalt)
        print(f'ShellMap guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e} '
              f'bin {res.bin_guard:.3e}; {res.binned} binned')
        assert min(res.edge_guard, res.margin_guard, res.bin_guard) >= GUARD and res.nonfinite == 0
        parts = [res.moments, res.abs_moments, res.counts, res.column, res.sums, res.abs_sums]
        total = parts if total is None else [a + b for a, b in zip(total, parts)]
    moments, mags, counts, column_sum, sums, abs_sums = total
    return moments, mags, S.ShellResult(counts, column_sum, sums, abs_sums, 0, 0, 0, 0, 0, 0)


def check_published(sm, want_moments, mags, base):
    assert sm.moments and np.array_equal(sm.packets, base.counts)
    assert sm.counters['samples_binned'] == base.counts.sum() and sm.counters['nonfinite'] == 0
    S.compare_planes(sm.shell_sums, base)
    assert np.all(np.abs(sm.shell_moment_sums - want_moments) <= RTOL*mags)
    mass = atomicmass('Na').value*const.AMU
    out = shell_moments_from_sums(sm.shell_sums, sm.shell_moment_sums, sm.atoms_per_packet, sm._volume,
                                  sm.r_edges, sm.unit_km, mass, sm.quantity)
    for name, value in out.items():
        if value is None:
            assert getattr(sm, name) is None and sm.quantity == 'radiance'
        else:
            np.testing.assert_allclose(getattr(sm, name), value, rtol=1e-13, atol=0, equal_nan=True)
    filled = sm.shell_sums[0, ..., 1:-1, 0] > 0
    assert filled.sum() > 300 and np.isfinite(sm.velocity[filled]).all()
    assert np.isnan(sm.velocity[~filled]).all() and np.isnan(sm.temperature[~filled]).all()
    assert np.all(np.abs(sm.velocity[filled]) < 100)                    # km/s, not R/s or cm/s
    if sm.quantity == 'column':
        np.testing.assert_allclose(sm.flux_net, sm.flux_up - sm.flux_down, rtol=1e-13, atol=0)
        assert np.all(sm.flux_up >= 0) and np.all(sm.shell_rate_up >= 0) and sm.shell_rate_up[0] > 0
        np.testing.assert_allclose(sm.shell_rate_net, sm.shell_rate_up - sm.shell_rate_down, rtol=1e-12)


def test_shell_map_moments_resident_restored_and_restatement(ctx, tmp_path):
    inputs = Input(INPUT, savepath=str(tmp_path))
    inputs.options.endtime = type(inputs.options.endtime)(3000., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2000, packs_per_it=1000, seed=81, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 2 and all(o.resident_rows(ctx) is not None for o in outs)
    restored = Input(INPUT)
    restored.options.endtime = inputs.options.endtime
    for k, f in enumerate(inputs.search()[1]):
        back = Output.restore(f)
        back.idnum = k + 1
        restored._catalogue.append(back)

    def columns(out):
        X = Output.restore(out).X
        return tuple(X[c].values for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'))

    for quantity in ('column', 'radiance'):
        params = dict(quantity=quantity, dims='24,12', altitude='0.25,3.25,12')
        with contextlib.redirect_stdout(io.StringIO()):
            resident = ShellMap(inputs, params, context=ctx, moments=True)
            host = ShellMap(restored, params, context=ctx, moments=True)
            plain = ShellMap(inputs, params, context=ctx)
        assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
        want, mags, base = restate_outputs(outs, resident, quantity, (24, 12), resident.r_edges, 12,
                                           columns)
        assert base.counts.sum() > 10000 and np.count_nonzero(mags[0, ..., 1:-1, 0]) > 500
        for sm in (resident, host):
            check_published(sm, want, mags, base)
        assert np.all(np.abs(host.shell_moment_sums - resident.shell_moment_sums) <= 2*RTOL*mags)
        # the keyword changes nothing of what the plain map publishes
        assert np.array_equal(plain.packets, resident.packets)
        np.testing.assert_allclose(plain.density, resident.density, rtol=RTOL, atol=0)
        np.testing.assert_allclose(plain.column, resident.column, rtol=RTOL, atol=0)


def test_shell_map_moments_around_io(ctx, tmp_path):
    """origin = a moon: the rows are moved into the moon's frame first, and the velocities are
    relative to the moon."""
    from tests.test_gpu_moon_frame import IoRun, quiet
    run = IoRun(ctx, savepath=str(tmp_path))
    params = dict(quantity='column', origin='Io', dims='12,6', altitude='0,4,4')
    sm = quiet(ShellMap, run.inputs, params, context=ctx, moments=True)
    want = shell_moments(*run.seven, run.vr, 'column', [], 12, 6, 1.0, 5.0, 4)
    print(f'Io guards: edge {want.edge_guard:.3e} bin {want.bin_guard:.3e}; {want.binned} binned')
    assert min(want.edge_guard, want.bin_guard) >= GUARD and want.binned > 1000
    assert np.array_equal(sm.packets, want.counts.astype(float))
    S.compare_planes(sm.shell_sums, want.base)
    assert np.all(np.abs(sm.shell_moment_sums - want.moments) <= RTOL*want.abs_moments)
    assert sm.unit == 'R_Io' and sm.unit_km == run.io_km
    filled = sm.shell_sums[0, ..., 1:-1, 0] > 0
    # launched at 0.5 - 4.5 km/s from Io (read in Jupiter's frame they would carry Io's 17 km/s)
    assert filled.sum() > 50 and np.all(np.abs(sm.velocity[filled]) < 6)
    assert sm.shell_rate_up[0] > 0 and np.all(sm.flux_up >= 0)


if __name__ == '__main__':                   # the guards of every case, without a GPU
    mercury = H.mercury_forces('Na', 1.3)
    for case in CASES:
        restate(mercury, *CASES[case](), case)
    a, b = CASES['first_call']()[0], CASES['second_call']()[0]
    restate(mercury, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), 'two', GRID, ALT, 'both calls')
