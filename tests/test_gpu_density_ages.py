"""k_density_ages, nxc_density_ages_* and ModelDensity(ages=...) on the GPU against
tests/density_ages_restatement.py (the "Density ages" definition of include/nexoclom_hip.h restated
with NumPy).

Dyadic scenes -- fractions in multiples of 1/16, times in multiples of 30 s, an axis of 30 s bins
from 60 s -- are held to ``np.array_equal``: every sum of f and of f f is then exact in fp64
whatever the order of the atomics.  Anything else is held to the summation bound of
tests/density_spectrum_restatement.py, (n - 1) 2^-52 sum |term| per record of n rows, derived there
and not measured.  Counts are always exact.  The device exposes no rows-per-record, so a second
pass over the same samples with frac = 1 gives them exactly ({n, n} per record)."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import Input, ModelDensity, hip_api
from nexoclom_amd.ModelDensity import DensityIndex
from nexoclom_amd.transient import response_matrix
from oracle import np_oracle as O
from tests import helpers as H
from tests.age_cube_restatement import apply_ordered, apply_plan
from tests.density_ages_restatement import check, check_exact, restate, rows_per_record
from tests.test_gpu_density_moments import WAVE_CASES, boundary_points, make_rows, wave_case
from tests.test_gpu_moon_frame import IoRun

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
T0 = 600.0
AXIS = (8, T0, 60.0, 300.0)            # 8 bins of 30 s from 60 s: inv_da = 1/30, edges on row ages
EPS = 2.0**-52


def quiet(make, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return make(*args, **kw)


def set_index(ctx, points, dr, axis=None):
    index = DensityIndex(points, dr)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    if axis is not None:
        ctx.density_ages_enable(*axis)
    return index


def download(ctx, index, Q):
    s0, counts = ctx.density_download()
    got = ctx.density_ages_download()
    sums = np.zeros((Q,) + got.shape[1:])
    sums[index.order] = got
    return sums, index.scatter(s0, Q), index.scatter(counts, Q)


def device_ages(ctx, points, dr, axis, calls):
    """(sums (Q, na + 2, 2), S0, counts, rows per record) in the points' order: one set, one enable
    and one accumulate per item of ``calls`` (five columns, time first, or ('rows', (store, first,
    count))); the rows per record from a second pass with frac = 1 (host columns only)."""
    index = set_index(ctx, points, dr, axis)
    for call in calls:
        if isinstance(call[0], str):
            ctx.density_ages_accumulate(rows=call[1])
        else:
            ctx.density_ages_accumulate(*call)
    got = download(ctx, index, len(points))
    if any(isinstance(call[0], str) for call in calls):
        return (*got, None)
    set_index(ctx, points, dr, axis)
    for t, x, y, z, frac in calls:
        ctx.density_ages_accumulate(t, x, y, z, np.ones_like(frac))
    return (*got, rows_per_record(download(ctx, index, len(points))[0]))


def aged(rng, n, dtype=np.float64, nan_every=0):
    """Row times in multiples of 30 s over [0, T0] -- ages 0 .. 600 s, every edge of AXIS among
    them -- and fractions in sixteenths, zeros among them."""
    t = (30.*rng.integers(0, 21, n)).astype(dtype)
    if nan_every:
        t[::nan_every] = np.nan
    return t, (rng.integers(0, 17, n)/16).astype(dtype)


def with_times(cols, t, frac=None):
    """Seven columns of make_rows as the five of the ages pass."""
    x, y, z, _, _, _, f = cols
    return (np.ascontiguousarray(t, dtype=x.dtype), x, y, z, f if frac is None else frac.astype(x.dtype))


# ---- 1. the wave-cooperative adds ---------------------------------------------------------------------
@pytest.mark.parametrize('bins', ['same bin', 'two bins', 'all bins'])
@pytest.mark.parametrize('name', WAVE_CASES)
def test_wave_shapes(ctx, name, bins):
    """The shapes of tests/test_gpu_density_moments.py with times added: lanes l and l + 32 hold
    the same point and the same bin, the same point and different bins (a bin per half wave), or
    whatever 21 ages give; several points come with the shapes themselves."""
    rng = np.random.default_rng(100 + WAVE_CASES.index(name))
    pts, dr, calls = wave_case(name, rng)
    five = []
    for cols in calls:
        n = len(cols[0])
        t, frac = aged(rng, n)
        if bins == 'same bin':
            t[:] = 510.                                               # age 90 s: plane 2
        elif bins == 'two bins':
            t = np.where((np.arange(n) % 64) < 32, 510., 390.)         # planes 2 and 6
        five.append(with_times(cols, t, frac))
    merged = tuple(np.concatenate(c) for c in zip(*five))
    want = restate(pts, dr, *AXIS, *merged)
    expected_hits = {'identical': 64, 'lower hit': 32, 'upper hit': 32, 'lane 0': 1, 'lane 63': 1}
    if name in expected_hits:
        assert want.counts[0] == expected_hits[name]
    else:
        assert want.counts.sum() >= 1
    check_exact(device_ages(ctx, pts, dr, AXIS, five), want, f'{name} {bins}')


# ---- 2. every edge of the axis ------------------------------------------------------------------------
@pytest.mark.parametrize('na', [8, 1])
def test_every_edge_of_the_axis(ctx, na):
    """One point, 96 rows on every edge: ages 0 and 30 s (below), 60 .. 300 s (300 = a_hi lands
    in the top plane), 330 s, and a NaN time."""
    rng = np.random.default_rng(7)
    ages = np.concatenate([[0., 30.], 60. + 30.*np.arange(9), [330., np.nan]])
    t = np.repeat(T0 - ages, 96)
    rng.shuffle(t)
    n = len(t)
    xyz = rng.normal(0, 0.01, (n, 3))
    frac = rng.integers(1, 17, n)/16
    cols = (t, *np.ascontiguousarray(xyz.T), frac)
    axis = (na, T0, 60., 300.)
    want = restate(np.zeros((1, 3)), 0.1, *axis, *cols)
    assert want.counts[0] == n and np.all(want.rows[0] > 0)          # all na + 2 planes are filled
    if na == 8:
        assert want.rows[0].tolist() == [192] + [96]*8 + [288]
    else:
        assert want.rows[0].tolist() == [192, 768, 288]
    check_exact(device_ages(ctx, np.zeros((1, 3)), 0.1, axis, [cols]), want, f'edges na={na}')


# ---- 3. members with f == 0 ---------------------------------------------------------------------------
def test_zero_fractions_are_counted(ctx):
    rng = np.random.default_rng(8)
    n = 500
    t, frac = aged(rng, n, nan_every=7)
    zero = np.arange(n) % 3 == 0
    frac[zero] = 0.
    assert np.isnan(t[zero]).any()
    xyz = rng.normal(0, 0.03, (n, 3))
    cols = (t, *np.ascontiguousarray(xyz.T), frac)
    pts = np.array([[0., 0., 0.], [0.05, 0., 0.]])
    want = restate(pts, 0.1, *AXIS, *cols)
    some = tuple(c[~zero] for c in cols)
    without = restate(pts, 0.1, *AXIS, *some)
    assert want.counts.sum() > without.counts.sum() > 100
    assert np.array_equal(want.sums, without.sums) and np.array_equal(want.s0, without.s0)
    got = device_ages(ctx, pts, 0.1, AXIS, [cols])
    check_exact(got, want, 'zeros')
    # the frac = 1 pass counted the NaN times of the f == 0 members in the top plane
    top_zero = restate(pts, 0.1, *AXIS, *(c[zero & np.isnan(t)] for c in cols)).rows[:, -1]
    assert top_zero.sum() > 0 and np.all(got[3][:, -1] >= top_zero)
    assert np.array_equal(got[3] - without.rows, restate(pts, 0.1, *AXIS, *(c[zero] for c in cols)).rows)


# ---- 4. host columns ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns_match_the_restatement(ctx, dtype):
    rng = np.random.default_rng(31)
    dr = 0.1
    seven = make_rows(rng, 50_000, dtype)
    t = rng.uniform(0., T0, 50_000)                 # ages over [0, 600): all ten planes of AXIS
    cols = with_times(seven, t)
    pts = np.concatenate([rng.uniform(-1, 1, (500, 3)),
                          np.stack(seven[:3], axis=1)[:50].astype(np.float64)])
    want = restate(pts, dr, *AXIS, *cols)
    assert want.counts.sum() > 10_000 and np.all(want.rows.sum(0) > 0)
    check(device_ages(ctx, pts, dr, AXIS, [cols]), want, f'columns {np.dtype(dtype).name}')
    # the plain pass over the same samples: the same counts, S0 within the bound, the block untouched
    index = set_index(ctx, pts, dr, AXIS)
    ctx.density_accumulate(*cols[1:])
    sums, s0, counts = download(ctx, index, len(pts))
    assert np.array_equal(counts, want.counts) and not sums.any()
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0)
    # boundary set: rows on the spheres, +-1 ulp; membership must still be scipy's
    q, ring = boundary_points(dr, rng, 6000, dtype)
    seven = make_rows(rng, len(ring), dtype, xyz=ring)
    cols = with_times(seven, rng.uniform(0., T0, len(ring)))
    want = restate(q, dr, *AXIS, *cols)
    assert want.counts.sum() > len(q)
    check(device_ages(ctx, q, dr, AXIS, [cols]), want, 'boundary')


# ---- 5. the second trip of the grid-stride loop -------------------------------------------------------
def test_second_trip_of_the_grid_stride_loop(ctx):
    """2^20 + 65 rows: more than the 256 CUs x 8 workgroups x 256 threads of a full grid, so the
    workgroups stride on to a ragged second trip."""
    rng = np.random.default_rng(33)
    p, dr = 2**20 + 65, 0.05
    seven = make_rows(rng, p)
    t, frac = aged(rng, p)
    cols = with_times(seven, t, frac)
    pts = np.concatenate([rng.uniform(-1, 1, (300, 3)), np.stack(seven[:3], axis=1)[-3:]])
    want = restate(pts, dr, *AXIS, *cols)
    assert want.counts.sum() > 10_000 and want.counts[-1] >= 1
    check_exact(device_ages(ctx, pts, dr, AXIS, [cols]), want, 'second trip')


# ---- 6. row stores ------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[True, False], ids=['narrow', 'wide'])
def lossless_store(request, ctx):
    """Rows of integrate_const_rows in HBM (float32 / int32, or 64-bit) and their host copy, from a
    run without a loss process (no lifetime, no photoionisation): every row keeps frac = 1.0
    exactly and every time is a multiple of the 30 s step, so the store's paths can be held to the
    bit.  (tests/test_gpu_age_cube.py builds the same store.)"""
    endtime, step = 3000., 30.
    forces = H.mercury_forces('Na', 1.3)
    X0 = H.sample_x0(300, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    ctx.set_forces(forces.GM, forces.vrplanet, forces.gravity, forces.radpres, 0.0, None,
                   forces.v_tab, forces.a_tab)
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    st = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=request.param, resident=True)['store']
    try:
        assert st.narrow == request.param and st.total > 10000
        rows, _ = st.download(index=False)
        assert rows.dtype == (np.float32 if request.param else np.float64)
        assert np.all(rows[7] == 1.0)                 # the premise of the exact comparisons
        yield st, rows
    finally:
        st.free()


@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, lossless_store, part):
    """Rows in HBM (narrow and wide stores), whole and as a slice with first > 0 that ends inside
    the store, against the host's columns of the same rows and the restatement: the same bits."""
    st, rows = lossless_store
    first, count = (0, st.total) if part == 'whole' else (777, st.total - 777 - 999)
    cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (0, 1, 2, 3, 7))
    axis = (50, 3000., -15.0, 1485.0)                # the step is 30 s: no age on an edge
    rng = np.random.default_rng(34)
    xyz = np.stack(cols[1:4], axis=1).astype(np.float64)
    pick = xyz[rng.choice(count, 400, replace=False)]
    pts = np.concatenate([pick, pick + rng.normal(0, 0.05, pick.shape)])
    dr = 0.05
    want = restate(pts, dr, *axis, *cols)
    assert want.counts.sum() > 1000 and want.bin_guard >= 1e-9
    assert want.sums[:, -1, 0].sum() > 0 and np.count_nonzero(want.rows[:, 1:-1].sum(0)) > 40
    from_store = device_ages(ctx, pts, dr, axis, [('rows', (st, first, count))])
    from_host = device_ages(ctx, pts, dr, axis, [cols])
    check_exact(from_host, want, f'host {part}')
    for a, b in zip(from_store[:3], from_host[:3]):
        assert np.array_equal(a, b)


# ---- 7. the contraction -------------------------------------------------------------------------------
def block_of(rng, Q, planes):
    """A block with a few empty records and no structure the order of addition could hide."""
    n = rng.integers(0, 30, (Q, planes))
    w = rng.uniform(0.5, 2.0, (Q, planes, 30))*(np.arange(30) < n[..., None])
    return np.stack([w.sum(-1), (w*w).sum(-1)], -1)


def line(Q):
    return np.stack([np.arange(Q, dtype=float), np.zeros(Q), np.zeros(Q)], axis=1)


def applied(ctx, Q, planes, ne, seed):
    rng = np.random.default_rng(seed)
    index = set_index(ctx, line(Q), 0.25, (planes - 2, T0, 0., 100.))
    assert np.array_equal(index.order, np.arange(Q))
    block = block_of(rng, Q, planes)
    ctx.density_ages_upload(block)
    assert np.array_equal(ctx.density_ages_download(), block)        # upload round-trips
    K = rng.uniform(0., 2., (planes, ne))
    K[rng.integers(0, planes), :] = 0.
    return block, K, ctx.density_ages_apply(K)


def test_apply_matches_the_ordered_sums(ctx):
    stride, run, chunk = apply_plan(10, 70, 64*1024)
    assert chunk == 64 and run > 8
    cases = [(1, 10, 1), (run - 1, 10, 3), (run + 1, 10, 70), (3*run + 7, 10, 70), (40, 9, 1),
             (40, 66, 70), (1, 3, 1)]
    for seed, (Q, planes, ne) in enumerate(cases):
        block, K, got = applied(ctx, Q, planes, ne, 40 + seed)
        assert got.shape == (ne, Q, 2)
        assert np.array_equal(got, apply_ordered(block, K)), (Q, planes, ne)
    # a K that is not finite is refused and leaves the block as it was
    block, K, _ = applied(ctx, 37, 10, 5, 50)
    for bad in (np.nan, np.inf):
        K_bad = K.copy()
        K_bad[3, 2] = bad
        with pytest.raises(hip_api.HipError, match='not finite') as err:
            ctx.density_ages_apply(K_bad)
        assert err.value.code == hip_api.NXC_ERR_ARG
    with pytest.raises(ValueError, match='one row per plane'):
        ctx.density_ages_apply(K[:-1])
    out = np.zeros((5, 37, 2))
    assert ctx.lib.nxc_density_ages_apply(ctx._h, 0, K.ctypes.data_as(C.POINTER(C.c_double)),
                                          out.ctypes.data_as(C.POINTER(C.c_double))) == hip_api.NXC_ERR_ARG
    assert np.array_equal(ctx.density_ages_download(), block)
    assert np.array_equal(ctx.density_ages_apply(K), apply_ordered(block, K))


# ---- 8. the entries -----------------------------------------------------------------------------------
def test_entries(ctx):
    rng = np.random.default_rng(44)
    seven = make_rows(rng, 4000)
    t, frac = aged(rng, 4000)
    cols = with_times(seven, t, frac)
    pts = rng.uniform(-1, 1, (40, 3))
    dr = 0.2
    fresh = hip_api.Context(0)
    try:
        for call in (lambda: fresh.density_ages_enable(*AXIS),
                     lambda: fresh.density_ages_accumulate(*cols),
                     fresh.density_ages_download):
            with pytest.raises(hip_api.HipError, match='nxc_density_set has not been called') as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        index = set_index(fresh, pts, dr)
        for call in (lambda: fresh.density_ages_accumulate(*cols), fresh.density_ages_download,
                     lambda: fresh.density_ages_upload(np.zeros((40, 2, 2))),
                     lambda: fresh.density_ages_apply(np.ones((2, 1)))):
            with pytest.raises(hip_api.HipError, match='nxc_density_ages_enable has not') as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        fresh.density_ages_enable(*AXIS)
        fresh.density_ages_accumulate(*cols)
        want = restate(pts, dr, *AXIS, *cols)
        assert want.counts.sum() > 100
        check_exact(download(fresh, index, 40), want, 'entries')
        # bad arguments leave the block as it was
        for bad, text in (((-1, T0, 60., 300.), 'na must be at least 1'),
                          ((8, np.nan, 60., 300.), 't0 must be finite'),
                          ((8, T0, np.inf, 300.), 'a_lo and a_hi must be finite'),
                          ((8, T0, 300., 300.), 'below a_hi'), ((8, T0, 300., 60.), 'below a_hi'),
                          ((2**31 // 40, T0, 60., 300.), 'n_points \\* \\(na \\+ 2\\) must be below 2\\^31')):
            with pytest.raises(hip_api.HipError, match='density ages: .*' + text) as err:
                fresh.density_ages_enable(*bad)
            assert err.value.code == hip_api.NXC_ERR_ARG
        check_exact(download(fresh, index, 40), want, 'after the refusals')
        ptrs = [c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols]
        for null in range(5):
            with_null = list(ptrs)
            with_null[null] = None
            assert fresh.lib.nxc_density_ages_accumulate(fresh._h, C.c_int64(4000), *with_null) \
                == hip_api.NXC_ERR_ARG
        assert fresh.lib.nxc_density_ages_accumulate(fresh._h, C.c_int64(-1), *ptrs) == hip_api.NXC_ERR_ARG
        assert fresh.lib.nxc_density_ages_accumulate(fresh._h, C.c_int64(0), *[None]*5) == 0
        for entry in ('download', 'upload'):
            assert getattr(fresh.lib, 'nxc_density_ages_' + entry)(fresh._h, None) == hip_api.NXC_ERR_ARG
        check_exact(download(fresh, index, 40), want, 'after the bad calls')
        # upload then download round-trips; a second enable zeroes; na = 0 frees
        block = block_of(rng, 40, 10)
        fresh.density_ages_upload(block)
        assert np.array_equal(fresh.density_ages_download(), block)
        with pytest.raises(ValueError, match='the block has'):
            fresh.density_ages_upload(block[:, :-1])
        fresh.density_ages_enable(*AXIS)
        assert not fresh.density_ages_download().any()
        fresh.density_ages_enable(0)
        with pytest.raises(hip_api.HipError, match='nxc_density_ages_enable has not'):
            fresh.density_ages_accumulate(*cols)
        # density_set switches the block off; without points there is no block
        fresh.density_ages_enable(*AXIS)
        set_index(fresh, pts, dr)
        with pytest.raises(hip_api.HipError, match='nxc_density_ages_enable has not'):
            fresh.density_ages_download()
        set_index(fresh, np.zeros((0, 3)), dr)
        with pytest.raises(hip_api.HipError, match='density ages: the index has no points'):
            fresh.density_ages_enable(*AXIS)
    finally:
        fresh.close()


def test_the_density_blocks_are_independent(ctx):
    """A plain, moments or spectrum pass on the same handle leaves the age block untouched, and an
    ages pass leaves theirs untouched."""
    rng = np.random.default_rng(45)
    seven = make_rows(rng, 6000)
    x, y, z, vx, vy, vz, f = seven
    t, frac = aged(rng, 6000)
    cols = with_times(seven, t, frac)
    pts = rng.uniform(-1, 1, (30, 3))
    index = set_index(ctx, pts, 0.25, AXIS)
    ctx.density_moments_enable()
    ctx.density_spectrum_enable(4, 0., 1e-3)
    ctx.density_ages_accumulate(*cols)
    want = restate(pts, 0.25, *AXIS, *cols)
    assert want.counts.sum() > 200
    check_exact(download(ctx, index, 30), want, 'ages first')
    assert not ctx.density_moments_download().any() and not ctx.density_spectrum_download().any()
    block = ctx.density_ages_download()
    ctx.density_accumulate(x, y, z, f)
    ctx.density_moments_accumulate(*seven)
    ctx.density_spectrum_accumulate(*seven)
    assert np.array_equal(ctx.density_ages_download(), block)
    assert ctx.density_moments_download().any() and ctx.density_spectrum_download().any()
    assert np.array_equal(index.scatter(ctx.density_download()[1], 30), 4*want.counts)
    moments, spectrum = ctx.density_moments_download(), ctx.density_spectrum_download()
    ctx.density_ages_accumulate(*cols)
    assert np.array_equal(ctx.density_moments_download(), moments)
    assert np.array_equal(ctx.density_spectrum_download(), spectrum)
    assert np.array_equal(ctx.density_ages_download(), 2*block)           # dyadic: exact


# ---- 9. the public flow -------------------------------------------------------------------------------
def trajectory(n):
    t = np.linspace(0, 1, n)
    return -2.5 + 5*t, -1.5 + 4*t, 0.6*np.sin(6*t)


def flow_columns(outputs, ctx):
    """time, x, y, z, frac of every Output's resident rows, downloaded."""
    per_output = []
    for out in outputs:
        view = out.resident_rows(ctx)
        rows, _ = view[0].download(view[1], view[2], index=False)
        per_output.append([np.asarray(rows[c], dtype=np.float64) for c in (0, 1, 2, 3, 7)])
    return [np.concatenate(c) for c in zip(*per_output)]


def check_object(model, want, axis, label):
    """age_sums, packets and S0 against the restatement, and what is published from them."""
    nbins = axis[0]
    scale = model.atoms_per_packet/float(model.Vpix)
    s0 = model.density*float(model.Vpix)/model.atoms_per_packet      # four more roundings
    assert np.array_equal(model.packets, want.counts)
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0 + 4*2.0**-53*want.s0)
    check((model.age_sums, want.s0, model.packets), want, label)
    assert model.age_density.shape == (len(want.s0), nbins)
    assert np.array_equal(model.age_density, model.age_sums[:, 1:-1, 0]*scale)
    assert np.array_equal(model.age_below, model.age_sums[:, 0, 0]*scale)
    assert np.array_equal(model.age_above, model.age_sums[:, -1, 0]*scale)
    assert np.array_equal(model.age_edges, axis[2] + np.arange(nbins + 1)*(axis[3] - axis[2])/nbins)
    # the sum identity: the planes and S0 are two orders of adding the same n terms
    total = model.age_density.sum(1) + model.age_below + model.age_above
    bound = (2*want.bound_s0 + (nbins + 6)*2.0**-52*want.s0)*scale
    assert np.all(np.abs(total - model.density) <= bound)
    return scale, bound


def test_end_to_end(ctx, tmp_path):
    inputs = Input(INPUT, savepath=str(tmp_path))
    inputs.options.endtime = type(inputs.options.endtime)(1800., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2e4, packs_per_it=5000, seed=17, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 4 and all(o.resident_rows(ctx) is not None for o in outs)
    xs, ys, zs = trajectory(200)
    pts = np.stack([xs, ys, zs], axis=1)
    dr, ages = 0.05, (0., 1600., 16)
    axis = (16, 1800., 0., 1600.)
    model = quiet(ModelDensity, inputs, xs, ys, zs, dr=dr, ages=ages, context=ctx)
    want = restate(pts, dr, *axis, *flow_columns(outs, ctx))
    assert want.counts.sum() > 300 and np.count_nonzero(want.rows.sum(0)) > 10
    scale, bound = check_object(model, want, axis, 'resident')
    plain = quiet(ModelDensity, inputs, xs, ys, zs, dr=dr, context=ctx)
    assert np.array_equal(plain.packets, model.packets) and not hasattr(plain, 'age_sums')
    assert np.all(np.abs(plain.density - model.density) <= 2*want.bound_s0*scale + 4*EPS*model.density)

    # transient of a constant history is the density; the block was taken by `plain`'s set, so the
    # first call uploads, and the second finds the claim
    assert ctx.ages_owner.get('density') is None
    epochs, history = np.array([0., 500., 2000.]), ([0.], [1.])
    first = model.transient(epochs, history)
    assert ctx.ages_owner.get('density') is model._ages_token
    assert first.density.shape == (3, 200) and np.all(first.kernel == 1.0)
    assert np.array_equal(first.density, apply_ordered(model.age_sums, first.kernel)[..., 0]*scale)
    assert np.all(np.abs(first.density - model.density) <= bound)
    # a second object takes the context's block; the first re-uploads and gives the same bits
    other = quiet(ModelDensity, inputs, xs[:50], ys[:50], zs[:50], dr=dr, ages=(0., 900., 3),
                  context=ctx)
    assert ctx.ages_owner.get('density') is other._ages_token
    history = ([-400., 0., 300.], [0.2, 3.0, 1.0])
    theirs = other.transient(epochs, history)
    assert np.array_equal(theirs.density,
                          apply_ordered(other.age_sums, theirs.kernel)[..., 0]
                          * (other.atoms_per_packet/float(other.Vpix)))
    again = model.transient(epochs, ([0.], [1.]))
    assert ctx.ages_owner.get('density') is model._ages_token
    assert np.array_equal(again.density, first.density)
    assert np.array_equal(again.effective_packets, first.effective_packets)
    varied = model.transient(epochs, history)
    assert np.array_equal(varied.kernel, response_matrix(model.age_edges, epochs, history))
    assert np.array_equal(varied.density, apply_ordered(model.age_sums, varied.kernel)[..., 0]*scale)
    # the track reads each point at its own time
    times = np.linspace(-200., 1500., 200)
    track = model.transient_track(history, times)
    per_epoch = model.transient(times[[0, 77, 199]], history).density
    assert np.array_equal(track.density[[0, 77, 199]], per_epoch[[0, 1, 2], [0, 77, 199]])


def test_around_io(ctx, tmp_path):
    run = IoRun(ctx, savepath=str(tmp_path))
    rng = np.random.default_rng(12)
    direction = rng.normal(size=(50, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    points = direction*rng.uniform(1.1, 3.0, 50)[:, None]              # within 3 R_Io of Io
    dr = 0.6
    x, y, z, _, _, _, frac = run.seven                     # the rows moved into Io's frame
    axis = (6, 6000., 0., 3000.)
    model = quiet(ModelDensity, run.inputs, *points.T, dr=dr, origin='Io', ages=(0., 3000., 6),
                  context=ctx)
    want = restate(points, dr, *axis, run.rows[0], x, y, z, frac)
    assert want.counts.sum() > 500 and np.count_nonzero(want.counts) > 20
    assert np.count_nonzero(want.rows.sum(0)) >= 6
    check_object(model, want, axis, 'Io')
    assert model.unit == 'R_Io' and model.origin.object == 'Io'
