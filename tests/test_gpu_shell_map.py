"""k_shell and ShellMap on the GPU against tests/shell_map_restatement.py (the "ShellMap" definition
of include/nexoclom_hip.h restated with NumPy).  Sample generators, the row stores and the image and
camera scenes are those of tests/test_gpu_pixel_moments.py.

Comparison rule, everywhere, that of tests/test_gpu_pixel_cube.py: the restatement's three guards
are asserted first (>= 1e-9: no located longitude or sin(latitude) that close to an edge -- the seam
and the poles are edges --, no sunlit decision that close to its threshold, no t that close to an
integer -- a condition on the inputs, met by the seeds below, which is what makes the exact
comparison of counts and the per-record comparison legitimate); then counts and counters must be
equal exactly, the column to rtol 1e-11, every plane entry to |got - want| <= 1e-11 * sum |term|
per (plane, cell, record, half), and on the downloaded result plane B summed over the records of a
cell must equal its column at rtol 1e-11.

Every case's inputs come from CASES, so that the guards of all of them can be checked without a
GPU: ``python -m tests.test_gpu_shell_map`` restates every case and prints its guards.  The
thresholds themselves, which the guards keep away from, are covered by
tests/test_gpu_shell_thresholds.py on the inputs of tests/threshold_cases.py."""
import contextlib
import io

import numpy as np
import pytest

from nexoclom_amd import Input, Output, ShellMap, hip_api
from nexoclom_amd.ShellMap import shell_axes, shell_from_sums
from tests import helpers as H
from tests.shell_map_restatement import ShellResult, edges, shell_map
from tests.test_gpu_pixel_moments import (GUARD, INPUT, ROWS_RTOL, RTOL, CameraScene,  # noqa: F401
                                          ImageScene, cloud, forces, store, tables)

pytestmark = pytest.mark.gpu
GRID = (12, 7)
ALT = (1.5, 4.0, 7)             # [R from the centre]: cloud() reaches from 1 to 6, so both ends fill


def five(cols):
    """x y z vy frac of cloud()'s seven columns"""
    return tuple(cols[k] for k in (0, 1, 2, 4, 6))


def place(lon, mu, r, rng, frac=None, dtype=np.float64):
    """Samples at solar-fixed longitude lon, sin(latitude) mu and distance r"""
    rho = np.sqrt(1 - mu*mu)
    n = len(lon)
    frac = rng.uniform(0.1, 1.0, n) if frac is None else frac
    cols = (r*rho*np.sin(lon), -r*rho*np.cos(lon), r*mu, rng.uniform(-0.02, 0.02, n), frac)
    return tuple(np.ascontiguousarray(np.asarray(c).astype(dtype)) for c in cols)


def far_cloud(p, seed, r_lo, r_hi):
    rng = np.random.default_rng(seed)
    return place(rng.uniform(0.01, 2*np.pi - 0.01, p), rng.uniform(-0.99, 0.99, p),
                 rng.uniform(r_lo, r_hi, p), rng)


def seam_and_poles(seed, n=256):
    """Longitudes 1e-7 .. 1e-2 on either side of the seam, in the first and the last mu band"""
    rng = np.random.default_rng(seed)
    delta = 10.0**rng.uniform(-7, -2, n)
    lon = np.where(np.arange(n) % 2 == 0, delta, 2*np.pi - delta)
    mu = np.where(np.arange(n) % 4 < 2, 1.0, -1.0)*rng.uniform(0.75, 0.999, n)
    return place(lon, mu, rng.uniform(1.2, 5.0, n), rng)


def one_record(seed, n=64):
    """A whole wave in cell (2, 5) (sunlit, near dusk), altitude bin 2 of GRID and ALT"""
    rng = np.random.default_rng(seed)
    lon = (2 + rng.uniform(0.2, 0.8, n))*2*np.pi/GRID[0]
    mu = -1 + (5 + rng.uniform(0.2, 0.8, n))*2/GRID[1]
    dr = (ALT[1] - ALT[0])/ALT[2]
    return place(lon, mu, ALT[0] + (2 + rng.uniform(0.2, 0.8, n))*dr, rng)


def shadow(seed, n=300):
    """Everything inside the shadow cylinder behind the planet"""
    rng = np.random.default_rng(seed)
    rho, phi = rng.uniform(0.05, 0.9, n), rng.uniform(0, 2*np.pi, n)
    cols = (rho*np.cos(phi), rng.uniform(1.2, 4.0, n), rho*np.sin(phi), rng.uniform(-0.02, 0.02, n),
            rng.uniform(0.1, 1.0, n))
    return tuple(np.ascontiguousarray(c) for c in cols)


def half_zero(seed, n=3001):
    cols = [c.copy() for c in five(cloud(n, seed))]
    cols[4][::2] = 0.0
    return tuple(cols)


def poisoned(seed, n=2001):
    """A NaN frac inside the grid, a NaN vy, a sample at the centre, and one there with a NaN frac"""
    cols = [c.copy() for c in five(cloud(n, seed))]
    cols[4][10] = np.nan
    cols[3][700] = np.nan
    for k in (1300, 1900):
        cols[0][k] = cols[1][k] = cols[2][k] = 0.0
    cols[4][1900] = np.nan
    return tuple(cols)


# name -> (columns, g-value tables' kind, (nlon, nlat), (r_lo, r_hi, nalt))
CASES = {f'p{p}': (lambda p=p: (five(cloud(p, 100 + p)), 'two', GRID, ALT))
         for p in (0, 1, 63, 64, 65, 1023, 1025)}
CASES.update({
    'second_trip': lambda: (five(cloud(1_200_001, 9, np.float32)), 'two', (9, 4), (1.5, 4.0, 33)),
    'grid_1x1': lambda: (five(cloud(5003, 21)), 'column', (1, 1), (1.5, 4.0, 1)),
    'grid_1x2': lambda: (five(cloud(5003, 22)), 'column', (1, 2), (1.5, 4.0, 3)),
    'grid_3x5': lambda: (five(cloud(5003, 23)), 'column', (3, 5), (1.5, 4.0, 7)),
    'grid_37x11': lambda: (five(cloud(30011, 24)), 'two', (37, 11), (1.5, 4.0, 5)),
    'all_below': lambda: (five(cloud(5003, 31)), 'column', GRID, (7.0, 9.0, 4)),
    'all_above': lambda: (far_cloud(5003, 32, 2.0, 6.0), 'column', GRID, (1.0, 1.5, 4)),
    'narrow': lambda: (five(cloud(20011, 33)), 'two', GRID, (2.0, 2.0625, 4)),
    'seam_and_poles': lambda: (seam_and_poles(41), 'constant', GRID, ALT),
    'one_record': lambda: (one_record(42), 'constant', GRID, ALT),
    'column': lambda: (five(cloud(30011, 51)), 'column', GRID, ALT),
    'one_line': lambda: (five(cloud(30011, 52)), 'constant', GRID, ALT),
    'two_lines': lambda: (five(cloud(30011, 53)), 'two', GRID, ALT),
    'shadow_one_line': lambda: (shadow(54), 'constant', GRID, ALT),
    'shadow_two_lines': lambda: (shadow(55), 'two', GRID, ALT),
    'half_zero': lambda: (half_zero(56), 'two', GRID, ALT),
    'poisoned_column': lambda: (poisoned(57), 'column', GRID, ALT),
    'poisoned_radiance': lambda: (poisoned(58), 'two', GRID, ALT),
    'float32': lambda: (five(cloud(40009, 59, np.float32)), 'two', GRID, ALT),
    'first_call': lambda: (five(cloud(9001, 61)), 'two', GRID, ALT),
    'second_call': lambda: (five(cloud(7001, 62)), 'two', GRID, ALT),
})


def restate(forces, cols, kind, grid, alt, name=''):
    quantity, gt = tables(forces, kind)
    want = shell_map(*cols, forces.vrplanet, quantity, gt, *grid, *alt)
    print(f'{name} guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e}; {want.samples} samples, {want.binned} binned, '
          f'{want.nonfinite} nonfinite')
    assert want.edge_guard >= GUARD and want.margin_guard >= GUARD and want.bin_guard >= GUARD
    return want


def shell_set(ctx, forces, kind, grid, alt):
    quantity, gt = tables(forces, kind)
    ctx.shell_set(forces.vrplanet, quantity, *edges(*grid), alt[0], alt[1], alt[2], gt)


def compare_planes(got, want, rtol=RTOL, reference=None):
    """|got - want| <= rtol * sum |term| per entry; the worst ratio per plane and half is printed."""
    reference = want.sums if reference is None else reference
    assert got.shape == want.sums.shape
    err = np.abs(got - reference)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(want.abs_sums > 0, err/want.abs_sums, np.where(err > 0, np.inf, 0.0))
    print('worst |got - want| / sum|term| (A: w, ww; B: c, cc):',
          [ratio[plane, ..., half].max() if ratio.size else 0 for plane in (0, 1) for half in (0, 1)])
    assert np.all(err <= rtol*want.abs_sums)


def compare(ctx, want, counters=None):
    column, counts, sums = ctx.shell_download()
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(column, want.column, rtol=RTOL, atol=0)
    compare_planes(sums, want)
    np.testing.assert_allclose(sums[1, ..., 0].sum(-1), column, rtol=RTOL, atol=0)
    if counters is not None:
        assert counters['samples'] == want.samples
        assert counters['samples_binned'] == want.binned == want.counts.sum()
        assert counters['nonfinite'] == want.nonfinite
    return column, counts, sums


def check(ctx, forces, name):
    cols, kind, grid, alt = CASES[name]()
    want = restate(forces, cols, kind, grid, alt, name)
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_accumulate(*cols)
    compare(ctx, want, ctx.counters())
    return want


# ---- 1. ragged waves and blocks ----------------------------------------------------------------------
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, p):
    want = check(ctx, forces, f'p{p}')
    assert want.binned == p
    if p >= 1023:
        assert np.count_nonzero(want.sums[0, ..., 1:-1, 0]) > 300


def test_second_trip_of_the_grid_stride_loop(ctx, forces):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    want = check(ctx, forces, 'second_trip')
    assert want.binned == 1_200_001 and np.count_nonzero(want.sums[0, ..., 1:-1, 0]) > 1000


# ---- 2. the grid --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['grid_1x1', 'grid_1x2', 'grid_3x5', 'grid_37x11'])
def test_grids(ctx, forces, name):
    """1 x 1 with one altitude bin, 1 x 2, 3 x 5 (2 pi / 3 is not representable) and a grid that is
    not square: with the cell index transposed its counts would not be the restatement's."""
    want = check(ctx, forces, name)
    assert want.counts.all() and want.binned == want.samples
    if name == 'grid_37x11':
        flat = want.counts.reshape(-1)
        assert not np.array_equal(flat, want.counts.T.reshape(-1))


@pytest.mark.parametrize('name', ['all_below', 'all_above', 'narrow'])
def test_altitude_axis(ctx, forces, name):
    want = check(ctx, forces, name)
    A = want.sums[0, ..., 0]
    if name == 'all_below':
        assert A[..., 0].sum() > 0 and not A[..., 1:].any()
    elif name == 'all_above':
        assert A[..., -1].sum() > 0 and not A[..., :-1].any()
    else:
        inside = A[..., 1:-1].sum()
        assert 0 < inside < 0.05*A.sum() and A[..., 0].sum() > inside and A[..., -1].sum() > inside
    assert want.binned == want.samples and want.column.all()


def test_seam_and_polar_bands(ctx, forces):
    """Longitudes just above 0 and just below 2 pi land in the first and the last longitude bin,
    sin(latitude) near -1 and 1 in the first and the last band."""
    want = check(ctx, forces, 'seam_and_poles')
    assert want.binned == 256
    assert np.count_nonzero(want.counts) == 4
    assert all(want.counts[ix, iz] == 64 for ix in (0, GRID[0] - 1) for iz in (0, GRID[1] - 1))


def test_a_whole_wave_in_one_record(ctx, forces):
    """64 samples in one record: lanes l and l + 32 add to the same 16 bytes of either plane."""
    want = check(ctx, forces, 'one_record')
    assert want.counts[2, 5] == 64 and want.binned == 64
    assert np.count_nonzero(want.sums[..., 0]) == 2 and want.sums[0, 2, 5, 3, 0] > 0


# ---- 3. inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['column', 'one_line', 'two_lines', 'float32'])
def test_quantities_and_widths(ctx, forces, name):
    want = check(ctx, forces, name)
    assert want.binned == want.samples and np.count_nonzero(want.sums[0, ..., 0]) > 500
    if name != 'column':                        # part of the cloud is in the planet's shadow
        assert 0 < np.count_nonzero(want.sums[0, ..., 1]) < np.count_nonzero(
            shell_map(*CASES[name]()[0], forces.vrplanet, 'column', [], *GRID, *ALT).sums[0, ..., 1])


@pytest.mark.parametrize('name', ['shadow_one_line', 'shadow_two_lines', 'half_zero'])
def test_zero_weights_count_and_add_nothing(ctx, forces, name):
    """Samples in the shadow cylinder (radiance) and samples with frac = 0 are counted in packets
    and add nothing to the column or to either plane."""
    cols = CASES[name]()[0]
    want = check(ctx, forces, name)
    assert want.binned == len(cols[0]) == want.counts.sum()
    _, counts, sums = ctx.shell_download()
    if name == 'half_zero':
        lit = shell_map(*(c[1::2] for c in cols), forces.vrplanet, *tables(forces, 'two'), *GRID, *ALT)
        assert np.array_equal(want.sums, lit.sums) and counts.sum() == 2*lit.binned + 1
    else:
        assert not want.sums.any() and not sums.any() and counts.sum() == 300


@pytest.mark.parametrize('name', ['poisoned_column', 'poisoned_radiance'])
def test_nonfinite_samples_are_counted_and_dropped(ctx, forces, name):
    cols = CASES[name]()[0]
    want = check(ctx, forces, name)
    assert want.nonfinite == 3 and want.binned == len(cols[0]) - 4
    column, _, sums = ctx.shell_download()
    assert np.isfinite(column).all() and np.isfinite(sums).all()


# ---- 4. state -----------------------------------------------------------------------------------------
def test_two_calls_sum_and_a_set_zeroes(ctx, forces):
    a, kind, grid, alt = CASES['first_call']()
    b = CASES['second_call']()[0]
    want_a = restate(forces, a, kind, grid, alt, 'first')
    want = restate(forces, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), kind, grid, alt, 'both')
    shell_set(ctx, forces, kind, grid, alt)
    ctx.shell_accumulate(*a)
    compare(ctx, want_a, ctx.counters())
    ctx.shell_accumulate(*b)
    compare(ctx, want)
    ctx.shell_accumulate(*(c[:0] for c in a))                    # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0 and ctx.counters()['samples_binned'] == 0
    compare(ctx, want)
    shell_set(ctx, forces, kind, grid, alt)                      # a set zeroes
    column, counts, sums = ctx.shell_download()
    assert not column.any() and not counts.any() and not sums.any()
    ctx.shell_accumulate(*a)
    compare(ctx, want_a, ctx.counters())
    shell_set(ctx, forces, kind, (5, 3), (1.0, 2.0, 2))          # another shape: new, zeroed sums
    column, counts, sums = ctx.shell_download()
    assert column.shape == (5, 3) and sums.shape == (2, 5, 3, 4, 2) and not sums.any()


def test_before_the_set_the_set_is_named():
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for call in (fresh.shell_download, lambda: fresh.shell_accumulate(x, x, x, x, x)):
            with pytest.raises(hip_api.HipError) as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE and 'nxc_shell_set' in str(err.value)
        assert fresh.lib.nxc_shell_download(fresh._h, None, None, None) == hip_api.NXC_ERR_STATE


def test_bad_arguments(ctx, forces):
    import ctypes as C
    shell_set(ctx, forces, 'column', (5, 3), (1.0, 3.0, 4))
    cols = five(cloud(2001, 71))
    ctx.shell_accumulate(*cols)
    before = ctx.shell_download()
    assert before[2].any()
    lon_e, mu_e = edges(5, 3)
    for bad, text in ((dict(r_lo=0.5), 'at least 1'), (dict(r_lo=3.0), 'below r_hi'),
                      (dict(nalt=0), 'nalt'), (dict(r_hi=np.inf), 'finite'),
                      (dict(lon=lon_e*0.5), 'span'), (dict(mu=mu_e[::-1].copy()), 'increase'),
                      (dict(nalt=2**31 // 15), '2^31')):
        args = dict(dict(lon=lon_e, mu=mu_e, r_lo=1.0, r_hi=3.0, nalt=4), **bad)
        with pytest.raises(hip_api.HipError) as err:
            ctx.shell_set(forces.vrplanet, 'column', args['lon'], args['mu'], args['r_lo'],
                          args['r_hi'], args['nalt'])
        assert err.value.code == hip_api.NXC_ERR_ARG and text in str(err.value)
    for got, was in zip(ctx.shell_download(), before):            # a refused set leaves the map alone
        assert np.array_equal(got, was)
    entry = ctx.lib.nxc_shell_accumulate
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), p, p, p, p, p) == hip_api.NXC_ERR_ARG
    for hole in range(5):
        args = [p]*5
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*5) == 0
    for got, was in zip(ctx.shell_download(), before):
        assert np.array_equal(got, was)
    # each output of the download is optional
    column = np.zeros((5, 3))
    assert ctx.lib.nxc_shell_download(ctx._h, column.ctypes.data_as(C.POINTER(C.c_double)), None,
                                      None) == 0
    assert np.array_equal(column, before[0])
    assert ctx.lib.nxc_shell_download(ctx._h, None, None, None) == 0


def test_image_camera_and_shell_map_never_touch(ctx, forces):
    """An image and a camera set on the same handle download unchanged after a shell accumulate, and
    the shell map downloads unchanged after an image and a camera accumulate and after their sets."""
    image, cam = ImageScene(forces, dims=(40, 24)), CameraScene(forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    a, b, c = cloud(9001, 81), cloud(7001, 82), cloud(8001, 83)
    want = restate(forces, five(c), 'two', GRID, ALT, 'shell')
    image.set(ctx, quantity, gt, enable=False)
    cam.set(ctx, quantity, gt, enable=False)
    shell_set(ctx, forces, 'two', GRID, ALT)
    image.plain(ctx, *a)
    cam.plain(ctx, *b)
    image_before, cam_before = image.pair(ctx), cam.pair(ctx)
    assert image_before[1].sum() > 1000 and cam_before[1].sum() > 500
    assert not any(part.any() for part in ctx.shell_download())
    ctx.shell_accumulate(*five(c))
    shell_before = compare(ctx, want, ctx.counters())
    for got, was in zip(image.pair(ctx) + cam.pair(ctx), image_before + cam_before):
        assert np.array_equal(got, was)
    image.plain(ctx, *b)
    cam.plain(ctx, *a)
    image.set(ctx, quantity, gt, enable=False)
    cam.set(ctx, quantity, gt, enable=False)
    for got, was in zip(ctx.shell_download(), shell_before):
        assert np.array_equal(got, was)
    image.plain(ctx, *a)
    cam.plain(ctx, *b)
    shell_set(ctx, forces, 'two', GRID, ALT)                     # and its set touches only its own
    assert not any(part.any() for part in ctx.shell_download())
    assert np.array_equal(image.pair(ctx)[1], image_before[1])
    assert np.array_equal(cam.pair(ctx)[1], cam_before[1])


# ---- 5. row stores ------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, forces, store, part):
    """Rows in HBM (float32 and 64-bit stores), whole and as a slice with first > 0 that ends inside
    the store, against the same rows sent from the host and against the restatement."""
    st, rows = store
    first, count = (0, st.total) if part == 'whole' else (777, st.total - 777 - 999)
    cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (1, 2, 3, 5, 7))
    alt = (1.25, 7.25, 12)          # the rows launched at the surface (r = 1 to rounding) lie below
    want = restate(forces, cols, 'two', GRID, alt, f'rows {part}')
    assert want.binned > 1000
    shell_set(ctx, forces, 'two', GRID, alt)
    ctx.shell_accumulate(*cols)
    host, host_counts, host_sums = compare(ctx, want, ctx.counters())
    shell_set(ctx, forces, 'two', GRID, alt)
    ctx.shell_accumulate(rows=(st, first, count))
    got, got_counts, got_sums = compare(ctx, want, ctx.counters())
    assert np.array_equal(got_counts, host_counts)
    np.testing.assert_allclose(got, host, rtol=ROWS_RTOL, atol=0)
    compare_planes(got_sums, want, rtol=ROWS_RTOL, reference=host_sums)


# ---- 6. the public class ------------------------------------------------------------------------------
def test_shell_map_resident_restored_and_restatement(ctx, tmp_path):
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
    params = dict(quantity='radiance', dims='24,12', altitude='0.25,3.25,12')     # r = 1 to rounding lies below
    with contextlib.redirect_stdout(io.StringIO()):
        resident = ShellMap(inputs, params, context=ctx)
        host = ShellMap(restored, params, context=ctx)
    assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
    nlon, nlat, nalt = 24, 12, 12
    r_lo, r_hi = resident.r_edges[0], resident.r_edges[-1]
    assert (r_lo, r_hi) == (1.25, 4.25)
    shape = (2, nlon, nlat, nalt + 2, 2)
    counts, column = np.zeros((nlon, nlat)), np.zeros((nlon, nlat))
    sums, mags = np.zeros(shape), np.zeros(shape)
    totalsource = 0.
    for out in outs:
        X = Output.restore(out).X
        cols = tuple(X[c].values for c in ('x', 'y', 'z', 'vy', 'frac'))
        vr, gt = float(out.vrplanet)/resident.unit_km, resident.g_tables(float(out.aplanet))
        res = shell_map(*cols, vr, 'radiance', gt, nlon, nlat, r_lo, r_hi, nalt)
        print(f'ShellMap guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e} '
              f'bin {res.bin_guard:.3e}; {res.binned} binned')
        assert min(res.edge_guard, res.margin_guard, res.bin_guard) >= GUARD and res.nonfinite == 0
        counts += res.counts
        column += res.column
        sums += res.sums
        mags += res.abs_sums
        totalsource += out.totalsource
    assert counts.sum() > 10000 and np.count_nonzero(sums[0, ..., 1:-1, 0]) > 500
    want = ShellResult(counts, column, sums, mags, 0, 0, 0, 0, 0, 0)
    app = 1e23/(totalsource/inputs.options.endtime.value)
    R_cm = resident.unit_km*1e5
    axes = shell_axes(nlon, nlat, 0.25, 3.25, nalt)
    V, area = axes['volume']*R_cm**3, axes['solid_angle']*R_cm**2
    for obj in (resident, host):
        assert np.array_equal(obj.packets, counts) and obj.counters['samples_binned'] == counts.sum()
        assert obj.counters['nonfinite'] == 0
        np.testing.assert_allclose(obj.atoms_per_packet, app, rtol=1e-14)
        compare_planes(obj.shell_sums, want)
        np.testing.assert_allclose(obj.column, column*app/area, rtol=RTOL, atol=0)
        products = shell_from_sums(column, obj.shell_sums, obj.atoms_per_packet, obj.solid_angle,
                                   axes['volume'], R_cm)
        assert np.array_equal(obj.density, products['density'])
        assert np.array_equal(obj.column_profile, products['column_profile'])
        assert obj.density.shape == (nlon, nlat, nalt) == obj.column_profile.shape
        # the conservation identities
        np.testing.assert_allclose((obj.density*V).sum(), app*sums[0, ..., 1:-1, 0].sum(), rtol=RTOL,
                                   atol=0)
        np.testing.assert_allclose((obj.column*area).sum(), app*column.sum(), rtol=RTOL, atol=0)
        np.testing.assert_allclose(obj.column_profile.sum(-1) + obj.column_below + obj.column_above,
                                   obj.column, rtol=RTOL, atol=0)
        S, ww = obj.shell_sums[0, ..., 1:-1, 0], obj.shell_sums[0, ..., 1:-1, 1]
        filled = ww != 0
        assert filled.sum() > 500 and not obj.density_effective_packets[~filled].any()
        assert np.all(obj.density_effective_packets[filled] >= 1 - 1e-12)
    assert np.all(np.abs(host.shell_sums - resident.shell_sums) <= 2*RTOL*mags)


if __name__ == '__main__':                   # the guards of every case, without a GPU
    mercury = H.mercury_forces('Na', 1.3)
    for case in CASES:
        restate(mercury, *CASES[case](), case)
    a, b = CASES['first_call']()[0], CASES['second_call']()[0]
    restate(mercury, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), 'two', GRID, ALT, 'both calls')
    restate(mercury, five(cloud(8001, 83)), 'two', GRID, ALT, 'independence')
