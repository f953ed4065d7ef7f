"""k_shell_ages, nxc_shell_ages_* and ShellMap(ages=...) on the GPU against
tests/shell_ages_restatement.py (the "ShellMap ages" definition of include/nexoclom_hip.h restated
with NumPy).  Scenes are those of tests/test_gpu_shell_map.py with row times in multiples of 30 s
over [0, 600] and fractions in sixteenths; the axis is 8 bins of 30 s from 60 s at t0 = 600 s.

Comparison rule, everywhere:
* the restatement's three guards (edge, sunlit margin, altitude bin) are asserted first, >= 1e-9,
  with no sample left out; ``python -m tests.test_gpu_shell_ages`` restates every case and prints
  them without a GPU.  The age plane has no guard: it is a fixed sequence of fp64 operations.
* column, packets, planes A and B and the counters are held to k_shell's own rule
  (tests/test_gpu_shell_map.compare); counts and counters are exact.
* quantity 'column': age plane A is ``np.array_equal`` -- sums of dyadic w and w w are exact in any
  order -- and so is the identity "the age planes of a record sum to plane A's record".
* age plane B, and both planes for radiance: |got - want| <= (n - 1) 2^-52 sum |term| per record,
  the bound derived in tests/density_spectrum_restatement.py, with n the rows per record of a second
  pass over the same samples at frac = 1 (which files a superset of the rows: the zeros too).  That
  second pass is restated, and for quantity 'column' it is also run on the device, where every
  record of age plane A then holds {n, n}: equal exactly.  Nothing is measured."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from nexoclom_amd import Input, ShellMap, hip_api
from nexoclom_amd.transient import response_matrix
from tests import helpers as H
from tests import test_gpu_shell_map as S
from tests.age_cube_restatement import apply_ordered, apply_plan
from tests.shell_ages_restatement import bound, guards_hold, shell_ages
from tests.test_gpu_pixel_moments import INPUT, cloud, forces, store, tables  # noqa: F401

pytestmark = pytest.mark.gpu
GRID, ALT = S.GRID, S.ALT
T0 = 600.0
AXIS = (8, T0, 60.0, 300.0)            # 8 bins of 30 s from 60 s: inv_da = 1/30, edges on row ages
EPS = 2.0**-52


def aged(cols5, seed, times=None, nan_every=0):
    """Six columns time x y z vy frac of a scene's five: times in multiples of 30 s over [0, T0]
    (or ``times``) and every fraction that is finite and not zero replaced by a multiple of 1/16 in
    (0, 1]; zeros and NaNs stay where the scene has them."""
    x, y, z, vy, frac = cols5
    n, dtype = len(x), x.dtype
    rng = np.random.default_rng(seed + 7000)
    t = 30.*rng.integers(0, 21, n) if times is None else np.asarray(times, dtype=np.float64)
    if nan_every:
        t[::nan_every] = np.nan
    f = rng.integers(1, 17, n)/16
    f = np.where(np.isfinite(frac) & (frac != 0), f, frac)
    return (np.ascontiguousarray(t.astype(dtype)), x, y, z, vy, np.ascontiguousarray(f.astype(dtype)))


def at_one(cols6):
    """The same samples at frac = 1 (a NaN stays: it is dropped either way)."""
    f = cols6[5]
    return (*cols6[:5], np.where(np.isnan(f), f, 1.0).astype(f.dtype))


def half_waves(n):
    """Age 90 s (plane 2) for lanes 0..31 of every wave, 210 s (plane 6) for lanes 32..63"""
    return np.where((np.arange(n) % 64) < 32, 510., 390.)


def every_plane(n):
    """Ages 30, 60 .. 300 s in turn: planes 0 .. 9 of AXIS, lane after lane"""
    return T0 - 30.*(1 + np.arange(n) % 10)


def scene(name, seed, **kw):
    """A case of tests/test_gpu_shell_map.py with times: (columns, kind, grid, altitude)"""
    cols, kind, grid, alt = S.CASES[name]()
    return aged(cols, seed, **kw), kind, grid, alt


# name -> (six columns, g-value tables' kind, (nlon, nlat), (r_lo, r_hi, nalt), axis)
CASES = {f'p{p}_{kind}': (lambda p=p, kind=kind: (aged(S.five(cloud(p, 100 + p)), p), kind, GRID, ALT, AXIS))
         for p in (0, 1, 63, 64, 65, 1023, 1025) for kind in ('column', 'two')}
CASES.update({
    'one_record_same_bin': lambda: (aged(S.one_record(42), 1, times=np.full(64, 510.)), 'column', GRID, ALT, AXIS),
    'one_record_half_waves': lambda: (aged(S.one_record(42), 2, times=half_waves(64)), 'column', GRID, ALT, AXIS),
    'one_record_all_bins': lambda: (aged(S.one_record(42), 3, times=every_plane(64)), 'column', GRID, ALT, AXIS),
    'one_record_radiance': lambda: (aged(S.one_record(42), 4, times=every_plane(64)), 'constant', GRID, ALT, AXIS),
    'grid_1x1': lambda: (*scene('grid_1x1', 5), (1, T0, 60.0, 300.0)),
    'grid_37x11': lambda: (*scene('grid_37x11', 6), AXIS),
    'ages_below': lambda: (aged(S.five(cloud(5003, 31)), 7, times=np.where(np.arange(5003) % 2, 570., 600.)),
                           'column', GRID, ALT, AXIS),
    'ages_above': lambda: (aged(S.five(cloud(5003, 32)), 8, times=30.*(np.arange(5003) % 11)),
                           'column', GRID, ALT, AXIS),
    'nan_times': lambda: (aged(S.five(cloud(5003, 33)), 9, nan_every=7), 'column', GRID, ALT, AXIS),
    'half_zero': lambda: (*scene('half_zero', 10), AXIS),
    'half_zero_column': lambda: (aged(S.half_zero(56), 11), 'column', GRID, ALT, AXIS),
    'poisoned_column': lambda: (*scene('poisoned_column', 12), AXIS),
    'poisoned_radiance': lambda: (*scene('poisoned_radiance', 13), AXIS),
    'seam_and_poles': lambda: (*scene('seam_and_poles', 14), AXIS),
    'seam_and_poles_column': lambda: (aged(S.seam_and_poles(41), 15), 'column', GRID, ALT, AXIS),
    'float32': lambda: (*scene('float32', 16), AXIS),
    'float32_column': lambda: (aged(S.five(cloud(40009, 59, np.float32)), 17), 'column', GRID, ALT, AXIS),
    'second_trip': lambda: (aged(S.five(cloud(1_200_001, 9, np.float32)), 18), 'column', (9, 4),
                            (1.5, 4.0, 33), AXIS),
    'first_call': lambda: (aged(S.five(cloud(9001, 61)), 19), 'column', GRID, ALT, AXIS),
    'second_call': lambda: (aged(S.five(cloud(7001, 62)), 20), 'column', GRID, ALT, AXIS),
})


def restate(forces, cols, kind, grid, alt, axis, name=''):
    """(the restatement, the rows per record of its second pass at frac = 1)"""
    quantity, gt = tables(forces, kind)
    want = shell_ages(*cols, forces.vrplanet, quantity, gt, *grid, *alt, *axis)
    ones = shell_ages(*at_one(cols), forces.vrplanet, quantity, gt, *grid, *alt, *axis)
    print(f'{name} guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e} (frac = 1: {ones.bin_guard:.3e}); {want.base.samples} samples, '
          f'{want.base.binned} binned, {int(want.rows.sum())} filed, {want.base.nonfinite} nonfinite')
    assert guards_hold(want) and guards_hold(ones)
    assert np.all(ones.rows >= want.rows)
    return want, ones.rows


def set_map(ctx, forces, kind, grid, alt, axis=None):
    S.shell_set(ctx, forces, kind, grid, alt)
    if axis is not None:
        ctx.shell_ages_enable(*axis)


def compare_block(block, want, n, kind, label=''):
    assert block.shape == want.block.shape
    assert not block[:, want.rows == 0].any(), label              # an empty record holds exact zeros
    limit = bound(want, n)
    err = np.abs(block - want.block)
    with np.errstate(divide='ignore', invalid='ignore'):
        worst = np.max(np.where(limit > 0, err/limit, 0.), initial=0.)
    print(f'{label} filed {int(want.rows.sum())} worst error / bound {worst:.3f}')
    if kind == 'column':
        assert np.array_equal(block[0], want.block[0]), label
    assert np.all(err <= limit), label


def compare(ctx, want, n, kind, counters=None, label=''):
    column, counts, sums = S.compare(ctx, want.base, counters)
    block = ctx.shell_ages_download()
    compare_block(block, want, n, kind, label)
    if kind == 'column':                 # dyadic: the age planes of a record sum to plane A's record
        assert np.array_equal(block[0].sum(axis=-2), sums[0]), label
        assert np.array_equal(sums[0], want.base.sums[0]), label
    return block


def check(ctx, forces, name):
    cols, kind, grid, alt, axis = CASES[name]()
    want, n = restate(forces, cols, kind, grid, alt, axis, name)
    set_map(ctx, forces, kind, grid, alt, axis)
    ctx.shell_ages_accumulate(*cols)
    compare(ctx, want, n, kind, ctx.counters(), name)
    if kind == 'column':                 # the rows per record, from the device
        set_map(ctx, forces, kind, grid, alt, axis)
        ctx.shell_ages_accumulate(*at_one(cols))
        A = ctx.shell_ages_download()[0]
        assert np.array_equal(A[..., 0], n) and np.array_equal(A[..., 1], n)
    return want


# ---- 1. ragged waves and blocks ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['column', 'two'])
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, p, kind):
    want = check(ctx, forces, f'p{p}_{kind}')
    assert want.base.binned == p
    if p >= 1023:
        assert np.count_nonzero(want.rows) > 300 and np.all(want.rows.sum(axis=(0, 1, 2)) > 0)


def test_second_trip_of_the_grid_stride_loop(ctx, forces):
    """More samples than one full grid of workgroups holds, as float32 host columns with times."""
    want = check(ctx, forces, 'second_trip')
    assert want.base.binned == 1_200_001 and np.count_nonzero(want.rows) > 5000


# ---- 2. the wave-cooperative adds ---------------------------------------------------------------------
@pytest.mark.parametrize('bins', ['same_bin', 'half_waves', 'all_bins', 'radiance'])
def test_a_whole_wave_in_one_record(ctx, forces, bins):
    """64 samples in one record of the planes: lanes l and l + 32 add to the same 16 bytes of the
    block (one age bin), to two records (a bin per half wave), or to all ten planes in turn."""
    want = check(ctx, forces, f'one_record_{bins}')
    assert want.base.counts[2, 5] == 64 and want.rows.sum() == 64
    per_age = want.rows[2, 5, 3]
    assert per_age.sum() == 64
    if bins == 'same_bin':
        assert per_age[2] == 64
    elif bins == 'half_waves':
        assert per_age[2] == 32 and per_age[6] == 32
    else:
        assert per_age.tolist() == [7, 7, 7, 7, 6, 6, 6, 6, 6, 6]


# ---- 3. grids and the axis ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['grid_1x1', 'grid_37x11'])
def test_grids(ctx, forces, name):
    """1 x 1 with one altitude bin and one age bin (nine records in all), and a grid that is not
    square on the radiance tables."""
    want = check(ctx, forces, name)
    assert want.base.counts.all() and want.base.binned == want.base.samples
    if name == 'grid_1x1':
        assert want.block.shape == (2, 1, 1, 3, 3, 2) and np.all(want.rows > 0)


@pytest.mark.parametrize('name', ['ages_below', 'ages_above', 'nan_times'])
def test_ages_outside_the_range_and_times_that_are_no_number(ctx, forces, name):
    want = check(ctx, forces, name)
    per_plane = want.rows.sum(axis=(0, 1, 2))
    if name == 'ages_below':             # ages 0 and 30 s
        assert per_plane[0] == want.rows.sum() > 4000 and not per_plane[1:].any()
    elif name == 'ages_above':           # ages 300 .. 600 s: a_hi itself lands in the top plane
        assert per_plane[-1] == want.rows.sum() > 4000 and not per_plane[:-1].any()
    else:
        nan = np.isnan(CASES[name]()[0][0])
        assert nan.sum() == 715 and per_plane[-1] >= nan.sum() and np.all(per_plane > 0)


# ---- 4. inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['half_zero', 'half_zero_column'])
def test_zeros_are_not_filed(ctx, forces, name):
    """Samples with frac = 0 are counted in packets and add nothing to the block: the block is that
    of the other half alone, and no record counts them (age plane A's w w would show a zero as a
    row only in the frac = 1 pass)."""
    cols, kind, grid, alt, axis = CASES[name]()
    want = check(ctx, forces, name)
    assert want.base.binned == len(cols[0]) == 3001
    quantity, gt = tables(forces, kind)
    lit = shell_ages(*(c[1::2] for c in cols), forces.vrplanet, quantity, gt, *grid, *alt, *axis)
    assert np.array_equal(want.block, lit.block) and np.array_equal(want.rows, lit.rows)
    assert want.rows.sum() <= 1500 < want.base.counts.sum()
    block = ctx.shell_ages_download() if kind != 'column' else None
    if block is not None:
        assert np.array_equal(block != 0, np.broadcast_to((want.rows != 0)[None, ..., None], block.shape))


@pytest.mark.parametrize('name', ['poisoned_column', 'poisoned_radiance'])
def test_nonfinite_samples_are_counted_and_dropped(ctx, forces, name):
    cols = CASES[name]()[0]
    want = check(ctx, forces, name)
    assert want.base.nonfinite == 3 and want.base.binned == len(cols[0]) - 4
    assert np.isfinite(want.block).all()


@pytest.mark.parametrize('name', ['seam_and_poles', 'seam_and_poles_column'])
def test_seam_and_polar_bands(ctx, forces, name):
    want = check(ctx, forces, name)
    assert want.base.binned == 256 and np.count_nonzero(want.base.counts) == 4


@pytest.mark.parametrize('name', ['float32', 'float32_column'])
def test_float32_columns(ctx, forces, name):
    cols = CASES[name]()[0]
    assert all(c.dtype == np.float32 for c in cols)
    want = check(ctx, forces, name)
    assert want.base.binned == want.base.samples == 40009 and np.count_nonzero(want.rows) > 2000


# ---- 5. state -----------------------------------------------------------------------------------------
def test_two_calls_sum_an_enable_zeroes_and_a_set_switches_off(ctx, forces):
    a, kind, grid, alt, axis = CASES['first_call']()
    b = CASES['second_call']()[0]
    both = tuple(np.concatenate([u, v]) for u, v in zip(a, b))
    want_a, n_a = restate(forces, a, kind, grid, alt, axis, 'first')
    want, n = restate(forces, both, kind, grid, alt, axis, 'both')
    set_map(ctx, forces, kind, grid, alt, axis)
    ctx.shell_ages_accumulate(*a)
    compare(ctx, want_a, n_a, kind, ctx.counters(), 'first')
    ctx.shell_ages_accumulate(*b)
    block = compare(ctx, want, n, kind, label='both')
    ctx.shell_ages_accumulate(*(c[:0] for c in a))               # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0
    assert np.array_equal(ctx.shell_ages_download(), block)
    # the plain pass on the same handle: k_shell's sums for the same samples, the block untouched
    shell = ctx.shell_download()
    ctx.shell_accumulate(*both[1:])
    again = ctx.shell_download()
    assert np.array_equal(again[1], 2*shell[1]) and np.array_equal(again[2][0], 2*shell[2][0])
    assert np.array_equal(ctx.shell_ages_download(), block)
    ctx.shell_ages_enable(*axis)                                 # an enable zeroes the block only
    assert not ctx.shell_ages_download().any()
    assert np.array_equal(ctx.shell_download()[1], again[1])
    S.shell_set(ctx, forces, kind, grid, alt)                    # a set switches the block off
    for call in (ctx.shell_ages_download, lambda: ctx.shell_ages_accumulate(*a),
                 lambda: ctx.shell_ages_upload(block), lambda: ctx.shell_ages_apply(np.ones((10, 1)))):
        with pytest.raises((hip_api.HipError, ValueError)) as err:
            call()
        if isinstance(err.value, hip_api.HipError):
            assert err.value.code == hip_api.NXC_ERR_STATE
            assert 'nxc_shell_ages_enable has not been called' in str(err.value)
    assert ctx.lib.nxc_shell_ages_download(ctx._h, block.ctypes.data_as(C.POINTER(C.c_double))) \
        == hip_api.NXC_ERR_STATE
    assert not any(part.any() for part in ctx.shell_download())  # the refused call added nothing
    ctx.shell_ages_enable(*axis)
    ctx.shell_ages_accumulate(*a)
    block = compare(ctx, want_a, n_a, kind, ctx.counters(), 'after the set')
    ctx.shell_moments_enable()                                   # the moments are another state
    assert np.array_equal(ctx.shell_ages_download(), block)
    assert not ctx.shell_moments_download().any()
    ctx.shell_ages_enable(0)                                     # na = 0 frees
    with pytest.raises(hip_api.HipError, match='nxc_shell_ages_enable has not'):
        ctx.shell_ages_download()
    S.compare(ctx, want_a.base)


def test_before_the_set_the_set_is_named():
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for call in (lambda: fresh.shell_ages_enable(*AXIS), fresh.shell_ages_download,
                     lambda: fresh.shell_ages_accumulate(x, x, x, x, x, x)):
            with pytest.raises(hip_api.HipError) as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE and 'nxc_shell_set' in str(err.value)
        out = np.zeros(8)
        p = out.ctypes.data_as(C.POINTER(C.c_double))
        for entry in ('upload', 'download'):
            assert getattr(fresh.lib, 'nxc_shell_ages_' + entry)(fresh._h, p) == hip_api.NXC_ERR_STATE
        assert fresh.lib.nxc_shell_ages_apply(fresh._h, 1, p, p) == hip_api.NXC_ERR_STATE


def test_bad_arguments(ctx, forces):
    set_map(ctx, forces, 'column', (5, 3), (1.0, 3.0, 4), AXIS)
    cols = aged(S.five(cloud(2001, 71)), 21)
    ctx.shell_ages_accumulate(*cols)
    before = ctx.shell_ages_download()
    assert before.any() and before.shape == (2, 5, 3, 6, 10, 2)
    for bad, text in (((-1, T0, 60., 300.), 'na must be at least 1'),
                      ((8, np.nan, 60., 300.), 't0 must be finite'),
                      ((8, T0, np.inf, 300.), 'a_lo and a_hi must be finite'),
                      ((8, T0, 300., 300.), 'below a_hi'), ((8, T0, 300., 60.), 'below a_hi'),
                      ((8, T0, -1.7e308, 1.7e308), 'a_hi - a_lo'),
                      ((2**31 // 90, T0, 60., 300.), 'must be below 2\\^31')):
        with pytest.raises(hip_api.HipError, match='shell ages: .*' + text) as err:
            ctx.shell_ages_enable(*bad)
        assert err.value.code == hip_api.NXC_ERR_ARG
    assert np.array_equal(ctx.shell_ages_download(), before)     # a refused enable leaves the block
    entry = ctx.lib.nxc_shell_ages_accumulate
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), *[p]*6) == hip_api.NXC_ERR_ARG
    for hole in range(6):
        args = [p]*6
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*6) == 0
    for name in ('download', 'upload'):
        assert getattr(ctx.lib, 'nxc_shell_ages_' + name)(ctx._h, None) == hip_api.NXC_ERR_ARG
    with pytest.raises(ValueError, match='the block has'):
        ctx.shell_ages_upload(before[:, :, :, :, :-1])
    assert np.array_equal(ctx.shell_ages_download(), before)


# ---- 6. row stores ------------------------------------------------------------------------------------
@pytest.mark.parametrize('slices', ['whole', 'first_row_then_the_rest'])
def test_row_stores(ctx, forces, store, slices):
    """Rows in HBM (float32 and 64-bit stores) over [0, n), and over [0, 1) plus [1, n), against
    the same rows sent from the host and against the restatement.  The rows' times are multiples
    of the 30 s step from 3000 s: the axis puts no age on an edge."""
    st, rows = store
    n_rows = st.total
    cols = tuple(np.ascontiguousarray(rows[c]) for c in (0, 1, 2, 3, 5, 7))
    alt, axis = (1.25, 7.25, 12), (50, 3000., -15.0, 1485.0)
    want, n = restate(forces, cols, 'two', GRID, alt, axis, f'rows {slices}')
    assert want.base.binned > 1000 and want.age_guard >= 1e-9
    assert np.count_nonzero(want.rows.sum(axis=(0, 1, 2))[1:-1]) > 40 and want.rows[..., -1].sum() > 0
    set_map(ctx, forces, 'two', GRID, alt, axis)
    ctx.shell_ages_accumulate(*cols)
    compare(ctx, want, n, 'two', ctx.counters(), 'host')
    host_counts = ctx.shell_download()[1]
    set_map(ctx, forces, 'two', GRID, alt, axis)
    if slices == 'whole':
        ctx.shell_ages_accumulate(rows=(st, 0, n_rows))
        counters = ctx.counters()
    else:
        ctx.shell_ages_accumulate(rows=(st, 0, 1))
        assert ctx.counters()['samples'] == 1
        ctx.shell_ages_accumulate(rows=(st, 1, n_rows - 1))
        counters = None
        assert ctx.counters()['samples'] == n_rows - 1
    compare(ctx, want, n, 'two', counters, f'store {slices}')
    assert np.array_equal(ctx.shell_download()[1], host_counts)


# ---- 7. the block's copies and the contraction ---------------------------------------------------------
def block_of(rng, shape):
    """A block with a few empty records and no structure the order of addition could hide."""
    n = rng.integers(0, 30, shape)
    w = rng.uniform(0.5, 2.0, shape + (30,))*(np.arange(30) < n[..., None])
    return np.stack([w.sum(-1), (w*w).sum(-1)], -1)


def test_download_upload_download_round_trip(ctx, forces):
    cols, kind, grid, alt, axis = CASES['first_call']()
    set_map(ctx, forces, kind, grid, alt, axis)
    ctx.shell_ages_accumulate(*cols)
    first = ctx.shell_ages_download()
    assert first.any()
    ctx.shell_ages_enable(*axis)
    assert not ctx.shell_ages_download().any()
    ctx.shell_ages_upload(first)
    assert np.array_equal(ctx.shell_ages_download(), first)
    other = block_of(np.random.default_rng(3), first.shape[:-1])
    ctx.shell_ages_upload(other)
    assert np.array_equal(ctx.shell_ages_download(), other)
    S.compare(ctx, shell_ages(*cols, forces.vrplanet, 'column', [], *grid, *alt, *axis).base)


@pytest.mark.parametrize('ne', [1, 64, 65])
def test_apply_matches_the_ordered_sums(ctx, forces, ne):
    """Both planes against apply_ordered, bit for bit; 64 epochs are one chunk, 65 two."""
    assert apply_plan(10, 65, 64*1024)[2] == 64
    rng = np.random.default_rng(40 + ne)
    grid, alt = (7, 5), (1.5, 4.0, 3)
    set_map(ctx, forces, 'column', grid, alt, AXIS)
    block = block_of(rng, (2,) + grid + (alt[2] + 2, 10))
    ctx.shell_ages_upload(block)
    K = rng.uniform(0., 2., (10, ne))
    K[rng.integers(0, 10), :] = 0.
    got = ctx.shell_ages_apply(K)
    assert got.shape == (2, ne) + grid + (alt[2] + 2, 2)
    for plane in (0, 1):
        assert np.array_equal(got[plane], apply_ordered(block[plane], K)), plane
    assert not np.array_equal(got[0], got[1])
    assert np.array_equal(ctx.shell_ages_download(), block)      # the block is only read
    S_, ww = got[0][..., 0], got[0][..., 1]
    assert np.all(S_ >= 0) and np.all(ww >= 0)


def test_apply_refusals(ctx, forces):
    rng = np.random.default_rng(50)
    grid, alt = (7, 5), (1.5, 4.0, 3)
    set_map(ctx, forces, 'column', grid, alt, AXIS)
    block = block_of(rng, (2,) + grid + (alt[2] + 2, 10))
    ctx.shell_ages_upload(block)
    K = rng.uniform(0., 2., (10, 5))
    for bad in (np.nan, np.inf):
        K_bad = K.copy()
        K_bad[3, 2] = bad
        with pytest.raises(hip_api.HipError, match='not finite') as err:
            ctx.shell_ages_apply(K_bad)
        assert err.value.code == hip_api.NXC_ERR_ARG
    with pytest.raises(ValueError, match='one row per plane'):
        ctx.shell_ages_apply(K[:-1])
    out = np.zeros((2, 5) + grid + (alt[2] + 2, 2))
    Kp, outp = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (K, out))
    assert ctx.lib.nxc_shell_ages_apply(ctx._h, 0, Kp, outp) == hip_api.NXC_ERR_ARG
    assert ctx.lib.nxc_shell_ages_apply(ctx._h, 5, None, outp) == hip_api.NXC_ERR_ARG
    assert ctx.lib.nxc_shell_ages_apply(ctx._h, 5, Kp, None) == hip_api.NXC_ERR_ARG
    assert np.array_equal(ctx.shell_ages_download(), block)
    assert np.array_equal(ctx.shell_ages_apply(K)[1], apply_ordered(block[1], K))
    # more planes than one record's share of the LDS of a workgroup (64 KiB or 160 KiB) holds
    na = 7000
    assert apply_plan(na + 2, 1, 160*1024) is None
    set_map(ctx, forces, 'column', (1, 1), (1.5, 4.0, 1), (na, T0, 0., 7000.))
    with pytest.raises(hip_api.HipError, match='exceed the') as err:
        ctx.shell_ages_apply(np.ones((na + 2, 1)))
    assert err.value.code == hip_api.NXC_ERR_ARG


# ---- 8. the public class ------------------------------------------------------------------------------
def quiet(make, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return make(*args, **kw)


def flow_columns(outputs, ctx):
    """time, x, y, z, vy, frac of every Output's resident rows, downloaded."""
    per_output = []
    for out in outputs:
        view = out.resident_rows(ctx)
        rows, _ = view[0].download(view[1], view[2], index=False)
        per_output.append([np.asarray(rows[c], dtype=np.float64) for c in (0, 1, 2, 3, 5, 7)])
    return [np.concatenate(c) for c in zip(*per_output)]


def check_object(sm, want, n, label):
    """shell_age_sums against the restatement, what is published from them, and the identities."""
    from nexoclom_amd.ShellMap import shell_ages_from_sums
    assert np.array_equal(sm.packets, want.base.counts)
    assert sm.counters['samples_binned'] == want.base.counts.sum() and sm.counters['nonfinite'] == 0
    S.compare_planes(sm.shell_sums, want.base)
    compare_block(sm.shell_age_sums, want, n, 'radiance', label)
    R_cm = sm.unit_km*1e5
    again = shell_ages_from_sums(sm.shell_age_sums, sm.atoms_per_packet, sm.solid_angle, sm._volume,
                                 R_cm, *sm.ages[:2])
    for name, value in again.items():
        assert np.array_equal(getattr(sm, name), value), name
    nalt, nbins = sm.altitude[2], sm.ages[2]
    assert sm.age_density.shape == tuple(sm.dims) + (nalt, nbins) == sm.age_column_profile.shape
    assert sm.age_column.shape == tuple(sm.dims) + (nbins,)
    # the identities: the age planes and the plain sums are two orders of adding the same n terms;
    # nbins + 2 (cells: (nalt + 2)(nbins + 2)) more additions on the host, four roundings of scaling
    per_volume = sm.atoms_per_packet/(sm._volume*R_cm**3)
    per_area = sm.atoms_per_packet/(sm.solid_angle*R_cm**2)
    n_rec = n.sum(-1)
    total = sm.age_density.sum(-1) + sm.age_density_below + sm.age_density_above
    limit = ((n_rec + nbins + 6)*EPS*want.base.abs_sums[0, ..., 0])[..., 1:-1]*per_volume
    assert np.all(np.abs(total - sm.density) <= limit)
    total = sm.age_column.sum(-1) + sm.age_column_below + sm.age_column_above
    n_cell = n.sum(axis=(-1, -2))
    limit = (2*n_cell + (nalt + 2)*(nbins + 2) + 6)*EPS*want.base.abs_sums[1, ..., 0].sum(-1)*per_area
    assert np.all(np.abs(total - sm.column) <= limit)
    return per_volume, per_area


def density_of(sm, sums):
    """Sums of plane A scaled as ShellMap scales its density"""
    return sums*sm.atoms_per_packet/(sm._volume*(sm.unit_km*1e5)**3)


@pytest.mark.parametrize('quantity', ['column', 'radiance'])
def test_end_to_end(ctx, tmp_path, quantity):
    inputs = Input(INPUT, savepath=str(tmp_path))
    inputs.options.endtime = type(inputs.options.endtime)(1800., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(4000, packs_per_it=2000, seed=17, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 2 and all(o.resident_rows(ctx) is not None for o in outs)
    assert len({(float(o.aplanet), float(o.vrplanet)) for o in outs}) == 1
    params = dict(quantity=quantity, dims='12,6', altitude='0.25,3.25,6')
    ages = (0., 1600., 16)
    sm = quiet(ShellMap, inputs, params, ages=ages, context=ctx)
    assert ctx.ages_owner.get('shell') is sm._ages_token
    cols = flow_columns(outs, ctx)
    vr, gt = float(outs[0].vrplanet)/sm.unit_km, sm.g_tables(float(outs[0].aplanet))
    args = (vr, quantity, gt, 12, 6, sm.r_edges[0], sm.r_edges[-1], 6, 16, 1800., 0., 1600.)
    want = shell_ages(*cols, *args)
    ones = shell_ages(*at_one(cols), *args)
    print(f'ShellMap guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e}; {want.base.binned} binned, {int(want.rows.sum())} filed')
    assert guards_hold(want) and guards_hold(ones) and want.base.nonfinite == 0
    assert want.rows.sum() > 10000 and np.count_nonzero(want.rows.sum(axis=(0, 1, 2))) >= 16
    per_volume, per_area = check_object(sm, want, ones.rows, quantity)

    # a constant history returns the steady state, to the same rounding as the identities
    epochs = np.array([0., 500., 2000.])
    first = sm.transient(epochs, ([0.], [1.]))
    assert ctx.ages_owner.get('shell') is sm._ages_token
    assert np.all(first.kernel == 1.0) and first.density.shape == (3, 12, 6, 6)
    direct = np.stack([apply_ordered(sm.shell_age_sums[plane], first.kernel) for plane in (0, 1)])
    assert np.array_equal(first.density, density_of(sm, direct[0][..., 1:-1, 0]))
    assert np.array_equal(first.column_profile, direct[1][..., 1:-1, 0]*per_area)
    n_rec, n_cell = ones.rows.sum(-1), ones.rows.sum(axis=(-1, -2))
    limit = ((n_rec + 24)*EPS*want.base.abs_sums[0, ..., 0])[..., 1:-1]*per_volume
    assert np.all(np.abs(first.density - sm.density) <= limit)
    limit = (2*n_cell + 8*18 + 6)*EPS*want.base.abs_sums[1, ..., 0].sum(-1)*per_area
    assert np.all(np.abs(first.column - sm.column) <= limit)
    if quantity == 'column':
        # positive terms: a record's two orders differ by n 2^-52 of it at most; 18 planes, the
        # pairwise sums over the 432 records and the scaling add a few roundings more
        inside = sm.shell_sums[0, ..., 1:-1, 0].sum()
        np.testing.assert_allclose(first.content, sm.atoms_per_packet*inside,
                                   rtol=(n_rec.max() + 64)*EPS, atol=0)
    else:
        assert first.content is None

    # a plain map takes the context's set: the block is gone, the next call uploads once
    plain = quiet(ShellMap, inputs, params, context=ctx)
    assert np.array_equal(plain.packets, sm.packets) and not hasattr(plain, 'shell_age_sums')
    np.testing.assert_allclose(plain.density, sm.density, rtol=S.RTOL, atol=0)
    np.testing.assert_allclose(plain.column, sm.column, rtol=S.RTOL, atol=0)
    assert ctx.ages_owner.get('shell') is None
    history = ([-400., 0., 300.], [0.2, 3.0, 1.0])
    varied = sm.transient(epochs, history)
    assert ctx.ages_owner.get('shell') is sm._ages_token
    K = response_matrix(sm.age_edges, epochs, history)
    assert np.array_equal(varied.kernel, K)
    direct = np.stack([apply_ordered(sm.shell_age_sums[plane], K) for plane in (0, 1)])
    assert np.array_equal(varied.density, density_of(sm, direct[0][..., 1:-1, 0]))
    cell = np.zeros((3, 12, 6, 2))
    for k in range(8):
        cell = cell + direct[1][:, :, :, k]
    assert np.array_equal(varied.column, cell[..., 0]*per_area)
    again = sm.transient(epochs, ([0.], [1.]))
    assert np.array_equal(again.density, first.density) and np.array_equal(again.column, first.column)
    # a step: the source switched on 300 s before the epoch fills only the three youngest bins, and
    # the bin that ends at the step sees the ramp's share of its launch interval
    step = sm.transient([300.], ([-1e-3, 0.], [0., 1.]))
    assert np.all(step.kernel[:4, 0] == 1.0) and not step.kernel[5:, 0].any()
    np.testing.assert_allclose(step.kernel[4, 0], 0.5e-3/100., rtol=1e-9)
    A = sm.shell_age_sums[0, ..., 1:-1, :, 0]
    young = density_of(sm, (((A[..., 0] + A[..., 1]) + A[..., 2]) + A[..., 3]) + A[..., 4]*step.kernel[4, 0])
    assert np.array_equal(step.density[0], young)
    assert young.sum() < 0.5*sm.density.sum()


def test_around_io(ctx, tmp_path):
    """origin = a moon: the rows are moved into the moon's frame first, and keep their times."""
    from tests.test_gpu_moon_frame import IoRun
    run = IoRun(ctx, savepath=str(tmp_path))
    params = dict(quantity='column', origin='Io', dims='12,6', altitude='0,4,4')
    sm = quiet(ShellMap, run.inputs, params, ages=(0., 3000., 6), context=ctx)
    args = (run.vr, 'column', [], 12, 6, 1.0, 5.0, 4, 6, 6000., 0., 3000.)
    cols = (run.rows[0], *run.five)
    want = shell_ages(*cols, *args)
    ones = shell_ages(*at_one(cols), *args)
    print(f'Io guards: edge {want.edge_guard:.3e} bin {want.bin_guard:.3e}; {want.base.binned} binned')
    assert guards_hold(want) and guards_hold(ones) and want.base.binned > 1000
    assert np.count_nonzero(want.rows.sum(axis=(0, 1, 2))) >= 6
    per_volume, _ = check_object(sm, want, ones.rows, 'Io')
    assert sm.unit == 'R_Io' and sm.unit_km == run.io_km
    steady = sm.transient([0.], ([0.], [1.]))
    limit = ((ones.rows.sum(-1) + 14)*EPS*want.base.abs_sums[0, ..., 0])[..., 1:-1]*per_volume
    assert np.all(np.abs(steady.density[0] - sm.density) <= limit)


if __name__ == '__main__':                   # the guards of every case, without a GPU
    mercury = H.mercury_forces('Na', 1.3)
    for case in CASES:
        restate(mercury, *CASES[case](), case)
    a, b = CASES['first_call']()[0], CASES['second_call']()[0]
    restate(mercury, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), 'column', GRID, ALT, AXIS,
            'both calls')
    restate(mercury, aged(S.five(cloud(2001, 71)), 21), 'column', (5, 3), (1.0, 3.0, 4), AXIS,
            'bad arguments')
