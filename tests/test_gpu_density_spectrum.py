"""k_density_spectrum on the GPU against tests/density_spectrum_restatement.py: the two planes of
spectrum sums, S0 and the counts per point, through host columns (float64, float32), row stores
and the ModelDensity(spectrum=...) flow.  Device and restatement add bit-identical terms to the
same records, so every sum is held to the summation bound derived there ((n - 1) 2^-52 sum|term|
per record and sum); counts and membership are scipy's.  The device exposes only sums, so the rows
per record are compared exactly through a second pass over the same samples with frac = 1, where
plane 0 holds that number."""
import contextlib
import ctypes as C
import io
import math

import numpy as np
import pytest

from nexoclom_amd import Input, ModelDensity, Output, hip_api
from nexoclom_amd.ModelDensity import DensityIndex, parse_spectrum, spectrum_frames
from tests import density_moments_restatement as moments_restatement
from tests.density_spectrum_restatement import check, frames_of, restate, seen_counts
from tests.test_gpu_density_moments import (INPUT, WAVE_CASES, boundary_points, flow_columns,
                                            make_rows, trajectory, wave_case)

pytestmark = pytest.mark.gpu
COS_60, COS_90 = math.cos(math.radians(60.)), math.cos(math.radians(90.))
# 16 bins that leave rows of make_rows (|v| about 2.3e-4 R/s) seen from a spacecraft of about
# 2e-4 R/s below, inside and above the range
BINS = (16, 1.5e-4, 4.5e-4)


def cone_spec(rng, Q, cos_half=COS_60, all_sky=False, bins=BINS):
    """(frames, nv, s_lo, s_hi, cos_half, all_sky): per point a random u of about 2e-4 R/s and a
    random unit boresight."""
    u = rng.normal(0, 2e-4 / math.sqrt(3), (Q, 3))
    b = rng.normal(size=(Q, 3))
    b /= np.linalg.norm(b, axis=1)[:, None]
    return (frames_of(u, b, Q), *bins, cos_half, all_sky)


def download(ctx, index, Q):
    s0, counts = ctx.density_download()
    dev = ctx.density_spectrum_download()
    sums = np.zeros((2, Q) + dev.shape[2:])
    sums[:, index.order] = dev
    return sums, index.scatter(s0, Q), index.scatter(counts, Q)


def device_spectrum(ctx, points, dr, spec, calls):
    """(sums (2, Q, nv + 2, 2), S0, counts) in the points' order after one set, one enable and one
    accumulate per item of ``calls`` (seven columns, or ('rows', (store, first, count)))."""
    index = DensityIndex(points, dr)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    frames, nv, s_lo, s_hi, cos_half, all_sky = spec
    ctx.density_spectrum_enable(nv, s_lo, s_hi, cos_half, all_sky, frames[index.order])
    for call in calls:
        if isinstance(call[0], str):
            ctx.density_spectrum_accumulate(rows=call[1])
        else:
            ctx.density_spectrum_accumulate(*call)
    return download(ctx, index, len(points))


def with_unit_frac(cols):
    return (*cols[:6], np.ones_like(cols[6]))


def check_case(ctx, points, dr, spec, calls, label, columns=None):
    """The sums of ``calls`` within their bounds, counts equal; then the same samples with frac = 1
    (``columns``: what a row store holds, as host columns): the rows per record, exactly."""
    merged = columns if columns is not None else tuple(np.concatenate(c) for c in zip(*calls))
    want = restate(points, dr, *spec, *merged)
    got = device_spectrum(ctx, points, dr, spec, calls)
    check(*got, want, label)
    unit = [with_unit_frac(c) for c in ([columns] if columns is not None else calls)]
    ones, _, counts = device_spectrum(ctx, points, dr, spec, unit)
    assert np.array_equal(counts, want.counts), label
    assert np.array_equal(seen_counts(ones), want.seen), label
    assert np.array_equal(ones[0, :, :, 1], want.seen), label      # 1 * 1 per seen row
    return want, got


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns_match_the_restatement(ctx, dtype):
    rng = np.random.default_rng(51)
    dr = 0.1
    cols = make_rows(rng, 50_000, dtype)
    pts = np.concatenate([rng.uniform(-1, 1, (500, 3)),
                          np.stack(cols[:3], axis=1)[:50].astype(np.float64)])
    spec = cone_spec(rng, len(pts))
    want, _ = check_case(ctx, pts, dr, spec, [cols], f'columns {np.dtype(dtype).name}')
    assert want.counts.sum() > 10_000 and want.counts[-50:].min() >= 1
    below, inside, above = want.seen[:, 0].sum(), want.seen[:, 1:-1].sum(axis=0), want.seen[:, -1].sum()
    assert below > 0 and above > 0 and (inside > 0).all()
    assert 1000 < want.seen.sum() < want.counts.sum() - 1000        # the cone cuts
    # boundary set: rows on the spheres, +-1 ulp; membership must still be scipy's
    q, ring = boundary_points(dr, rng, 6000, dtype)
    cols = make_rows(rng, len(ring), dtype, xyz=ring)
    want, _ = check_case(ctx, q, dr, cone_spec(rng, len(q)), [cols], 'boundary')
    assert want.counts.sum() > len(q)


def test_planted_edges(ctx):
    """u = 0, nv = 4 over [2^-13, 5 * 2^-13): inv_ds = 2^13, every speed and t exact.  One point per
    planted row, frac = 1, so plane 0 of a point reads 1 in the record its row reached."""
    a = 2.0**-13
    nv, s_lo, s_hi = 4, a, 5*a
    nan = float('nan')

    def planted(velocities, cos_half, all_sky):
        n = len(velocities)
        pts = np.stack([2.0*np.arange(n), np.zeros(n), np.zeros(n)], axis=1)
        v = np.asarray(velocities, dtype=np.float64)
        cols = (*pts.T.copy(), *v.T.copy(), np.ones(n))
        spec = (frames_of(0., [0., 0., 1.], n), nv, s_lo, s_hi, cos_half, all_sky)
        want = restate(pts, 0.1, *spec, *cols)
        got = device_spectrum(ctx, pts, 0.1, spec, [cols])
        check(*got, want, 'planted')
        assert np.array_equal(got[2], np.ones(n))                  # every row is a member
        assert np.array_equal(np.nan_to_num(got[0][0, :, :, 0]), want.seen)
        return got[0]

    # the whole sky: s at s_lo, at an interior edge, at s_hi, s = 0, one bin up, NaN vx
    sums = planted([[a, 0, 0], [0, 2*a, 0], [0, 0, 5*a], [0, 0, 0], [0, -3*a, 0], [nan, 0, 0]],
                   -1.0, True)
    assert [int(np.flatnonzero(row)[0]) for row in sums[0, :, :, 0]] == [1, 2, nv + 1, 0, 3, nv + 1]
    assert np.array_equal(sums[0, :, :, 0].sum(axis=1), np.ones(6))
    assert np.array_equal(sums[1, :5, :, 0].sum(axis=1), [a, 2*a, 5*a, 0., 3*a])   # g = 1 * s
    assert np.isnan(sums[1, 5, nv + 1]).all() and not np.isnan(sums[1, 5, :nv + 1]).any()
    # a cone of 90 degrees about b = +z: perpendicular (not seen: cos(radians(90)) > 0), along -b
    # (seen, from +z), along +b (not seen), NaN vx (not seen, still counted), s = 0 (seen: 0 >= 0)
    sums = planted([[2*a, 0, 0], [0, 0, -2*a], [0, 0, 2*a], [nan, 0, 0], [0, 0, 0]], COS_90, False)
    assert COS_90 > 0
    planes = [np.flatnonzero(row).tolist() for row in sums[0, :, :, 0]]
    assert planes == [[], [2], [], [], [0]]
    assert not np.isnan(sums).any()


@pytest.mark.parametrize('name', WAVE_CASES + ['odd lanes seen'])
def test_wave_shapes(ctx, name):
    if name == 'odd lanes seen':
        # one wave, all 64 lanes hit the point; b = +z and a cone of 60 degrees: the odd lanes'
        # rows fly along -z (seen), the even lanes' along +z (not seen)
        rng = np.random.default_rng(99)
        pts, dr = np.zeros((1, 3)), 0.1
        xyz = rng.normal(0, 0.005, (64, 3))
        speed = rng.uniform(1e-4, 5e-4, 64)
        v = np.zeros((64, 3))
        v[:, 2] = np.where(np.arange(64) % 2 == 1, -speed, speed)
        calls = [(*xyz.T.copy(), *v.T.copy(), rng.uniform(0, 1, 64))]
        spec = (frames_of(0., [0., 0., 1.], 1), *BINS, COS_60, False)
        want, _ = check_case(ctx, pts, dr, spec, calls, name)
        assert want.counts[0] == 64 and want.seen.sum() == 32
        return
    rng = np.random.default_rng(WAVE_CASES.index(name))
    pts, dr, calls = wave_case(name, rng)
    # through a cone (a lane that hits may not be seen), then the whole sky (every hit is seen:
    # the shape of the hits is the shape of the spectrum adds)
    check_case(ctx, pts, dr, cone_spec(rng, len(pts)), calls, name + ', cone')
    want, _ = check_case(ctx, pts, dr, cone_spec(rng, len(pts), all_sky=True), calls, name + ', sky')
    assert np.array_equal(want.seen.sum(axis=1), want.counts)
    expected_hits = {'identical': 64, 'lower hit': 32, 'upper hit': 32, 'lane 0': 1, 'lane 63': 1}
    if name in expected_hits:
        assert want.counts[0] == expected_hits[name]
    else:
        assert want.counts.sum() >= 1


def test_second_trip_of_the_grid_stride_loop(ctx):
    """2^20 + 65 rows: more than the 256 CUs x 8 workgroups x 256 threads of a full grid at the
    highest occupancy a 256-thread kernel can have, so the workgroups stride on to a ragged
    second trip."""
    rng = np.random.default_rng(53)
    p, dr = 2**20 + 65, 0.05
    cols = make_rows(rng, p)
    pts = np.concatenate([rng.uniform(-1, 1, (300, 3)), np.stack(cols[:3], axis=1)[-3:]])
    want, _ = check_case(ctx, pts, dr, cone_spec(rng, len(pts)), [cols], 'second trip')
    assert want.counts.sum() > 10_000 and want.counts[-1] >= 1 and want.seen.sum() > 1000


@pytest.mark.parametrize('narrow', [True, False])
def test_row_stores_match_the_restatement(ctx, narrow):
    """Rows as Input.run leaves them in HBM (float32 or 64-bit), read where they are: columns
    1-7 of the downloaded rows feed the restatement.  Then a sub-range of the store."""
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(9000., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, 3000, seed=8, context=ctx, save=narrow)
    view = out.resident_rows(ctx)
    assert view is not None and view[0].narrow == narrow
    store, first, count, _ = view
    rows, _ = store.download(first, count, index=False)
    rng = np.random.default_rng(52)
    dr = 0.05
    xyz = np.stack(rows[1:4], axis=1).astype(np.float64)
    pick = xyz[rng.choice(count, 750, replace=False)]
    pts = np.concatenate([pick, pick + rng.normal(0, 0.05, pick.shape)])
    speed = np.linalg.norm(np.stack(rows[4:7], axis=1).astype(np.float64), axis=1)
    bins = (16, float(np.quantile(speed, 0.2)), float(np.quantile(speed, 0.8)))
    spec = cone_spec(rng, len(pts), bins=bins)
    want, _ = check_case(ctx, pts, dr, spec, [('rows', (store, first, count))],
                         f'rows narrow={narrow}', columns=tuple(rows[1:8]))
    assert want.counts.sum() > 2000 and want.seen.sum() > 200
    a, n = count // 3, count // 2
    want, _ = check_case(ctx, pts, dr, spec, [('rows', (store, first + a, n))], 'sub-range',
                         columns=tuple(r[a:a + n] for r in rows[1:8]))
    assert 0 < want.counts.sum()


def test_entries(ctx):
    rng = np.random.default_rng(54)
    cols = make_rows(rng, 4000)
    pts = rng.uniform(-1, 1, (40, 3))
    dr = 0.2
    spec = cone_spec(rng, len(pts))
    fresh = hip_api.Context(0)
    try:
        index = DensityIndex(pts, dr)
        frames = spec[0][index.order]
        enable = lambda nv=spec[1], **kw: fresh.density_spectrum_enable(           # noqa: E731
            nv, **{**dict(s_lo=spec[2], s_hi=spec[3], cos_half=spec[4], all_sky=spec[5],
                          frames=frames), **kw})
        for call in (lambda: fresh.density_spectrum_accumulate(*cols), enable,
                     fresh.density_spectrum_download):
            with pytest.raises(hip_api.HipError, match='nxc_density_set has not been called') as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        args = (index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
        fresh.density_set(*args)
        for call in (lambda: fresh.density_spectrum_accumulate(*cols),
                     fresh.density_spectrum_download):
            with pytest.raises(hip_api.HipError, match='nxc_density_spectrum_enable has not') as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        enable()
        ptrs = [c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols]
        for null in (0, 3, 4, 5, 6):
            with_null = list(ptrs)
            with_null[null] = None
            rc = fresh.lib.nxc_density_spectrum_accumulate(fresh._h, C.c_int64(len(cols[0])), *with_null)
            assert rc == hip_api.NXC_ERR_ARG
        assert fresh.lib.nxc_density_spectrum_accumulate(fresh._h, C.c_int64(-1), *ptrs) == hip_api.NXC_ERR_ARG
        # p = 0 is accepted (null columns too) and adds nothing
        assert fresh.lib.nxc_density_spectrum_accumulate(fresh._h, C.c_int64(0), *[None]*7) == 0
        sums, s0, counts = download(fresh, index, len(pts))
        assert sums.shape == (2, 40, 18, 2)
        assert not sums.any() and not s0.any() and not counts.any()
        fresh.density_spectrum_accumulate(*cols)
        want = restate(pts, dr, *spec, *cols)
        assert want.counts.sum() > 100 and want.seen.sum() > 50
        check(*download(fresh, index, len(pts)), want, 'entries')
        # a refused enable leaves the spectrum there is as it is: the check comes first
        bad_frames = frames.copy()
        bad_frames[7, 5] = np.nan
        long_b = frames.copy()
        long_b[3, 4:7] *= 1.0 + 1e-9
        for kw in (dict(nv=-1), dict(s_lo=-1e-4), dict(s_lo=spec[3]), dict(s_hi=np.inf),
                   dict(cos_half=1.5), dict(frames=bad_frames), dict(frames=long_b),
                   dict(frames=frames[:-1]), dict(frames=np.concatenate([frames, frames[:1]])),
                   dict(nv=2**31 // 40)):
            with pytest.raises(hip_api.HipError, match='density spectrum') as err:
                enable(**kw)
            assert err.value.code == hip_api.NXC_ERR_ARG
        check(*download(fresh, index, len(pts)), want, 'after refusals')
        enable(all_sky=True, frames=long_b)              # no boresight is asked of the whole sky
        # enabled again with another nv: freed, allocated anew and zeroed
        enable(nv=5)
        sums, s0, counts = download(fresh, index, len(pts))
        assert sums.shape == (2, 40, 7, 2) and not sums.any()
        assert np.array_equal(counts, want.counts)        # the pair array is nxc_density_set's
        fresh.density_spectrum_accumulate(*cols)
        five = restate(pts, dr, spec[0], 5, *spec[2:], *cols)
        sums, _, counts = download(fresh, index, len(pts))
        assert np.array_equal(counts, 2*want.counts)
        assert np.all(np.abs(sums - five.sums) <= five.bound)
        # nv = 0 frees it
        fresh.density_spectrum_enable(0)
        with pytest.raises(hip_api.HipError, match='nxc_density_spectrum_enable has not'):
            fresh.density_spectrum_download()
        # a new density_set zeroes and switches the spectrum off
        enable()
        fresh.density_set(*args)
        with pytest.raises(hip_api.HipError, match='nxc_density_spectrum_enable has not'):
            fresh.density_spectrum_accumulate(*cols)
        enable()
        sums, s0, counts = download(fresh, index, len(pts))
        assert not sums.any() and not s0.any() and not counts.any()
        # Q = 0: accepted, nothing to add to
        none = DensityIndex(np.zeros((0, 3)), dr)
        fresh.density_set(none.points, none.cell_start, none.origin, none.h, none.dr, none.dims)
        fresh.density_spectrum_enable(spec[1], *spec[2:], frames=np.zeros((0, 8)))
        fresh.density_spectrum_accumulate(*cols)
        assert fresh.density_spectrum_download().shape == (2, 0, 18, 2)
    finally:
        fresh.close()


def test_other_consumers_are_unchanged_after_a_spectrum_call(ctx):
    """k_density and k_density_moments over the same samples, on the handle that has just served
    density_spectrum_accumulate, give their own results and leave the spectrum block as it was,
    bit for bit."""
    rng = np.random.default_rng(55)
    cols = make_rows(rng, 20_000)
    x, y, z, vx, vy, vz, frac = cols
    pts = rng.uniform(-1, 1, (60, 3))
    dr, Q = 0.15, 60
    spec = cone_spec(rng, Q)
    index = DensityIndex(pts, dr)

    def begin():
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
        ctx.density_spectrum_enable(spec[1], *spec[2:], frames=spec[0][index.order])
        ctx.density_moments_enable()
    begin()
    ctx.density_spectrum_accumulate(*cols)
    want = restate(pts, dr, *spec, *cols)
    assert want.counts.sum() > 1000 and want.seen.sum() > 300
    check(*download(ctx, index, Q), want, 'spectrum first')
    block = ctx.density_spectrum_download()
    assert not ctx.density_moments_download().any()
    ctx.density_accumulate(x, y, z, frac)
    ctx.density_moments_accumulate(*cols)
    assert np.array_equal(ctx.density_spectrum_download(), block)
    _, counts = ctx.density_download()
    assert np.array_equal(index.scatter(counts, Q), 3*want.counts)
    moments = moments_restatement.restate(pts, dr, *cols)
    got = np.zeros((Q, 10))
    got[index.order] = ctx.density_moments_download()
    assert np.all(np.abs(got - moments.sums) <= moments.bound)
    # k_density alone after a fresh set: its own pair, and nothing in the enabled blocks
    begin()
    ctx.density_accumulate(x, y, z, frac)
    sums, s0, counts = download(ctx, index, Q)
    assert np.array_equal(counts, want.counts)
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0)
    assert not sums.any() and not ctx.density_moments_download().any()


def model_spec(inputs, pts, spectrum):
    """The restatement's spec of a ``spectrum=`` argument, formed with the host's own helpers: the
    frames in the points' order and the range in R/s."""
    R = float(inputs.geometry.planet.radius.value)
    parsed = parse_spectrum(spectrum, len(pts))
    s_lo, s_hi, nbins = parsed['speed']
    frames = spectrum_frames(parsed, R, np.arange(len(pts)))
    return frames, nbins, s_lo/R, s_hi/R, parsed['cos_half'], parsed['all_sky']


def check_model(model, want, label):
    """``spectrum_sums`` within the bounds, the counts, S0 (which the object holds scaled into
    ``density``: undoing that costs four more roundings, 4 * 2^-53 S0) and what is derived."""
    s0 = model.density * float(model.Vpix) / model.atoms_per_packet
    check(model.spectrum_sums, want.s0, model.packets, want, label)
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0 + 4 * 2.0**-53 * want.s0)
    scale = model.atoms_per_packet / float(model.Vpix)
    assert np.array_equal(model.density_spectrum, model.spectrum_sums[0, :, 1:-1, 0]*scale)
    assert np.array_equal(model.density_in_view, model.spectrum_sums[0, :, :, 0].sum(axis=1)*scale)
    assert np.all(model.density_in_view <= model.density*(1 + 1e-12))
    empty = want.seen[:, 1:-1] == 0
    assert not model.spectrum_effective_packets[empty].any()
    assert not model.flux_effective_packets[empty].any()
    eff = model.spectrum_effective_packets[~empty]
    assert np.all((eff >= 1 - 1e-12) & (eff <= want.seen[:, 1:-1][~empty]*(1 + 1e-12)))
    assert np.isfinite(model.flux_spectrum).all() and np.isfinite(model.density_spectrum).all()


def ram_spectrum(pts, half_angle=60.):
    """A spacecraft flying along the points at 3 km/s, looking into the ram direction."""
    tangent = np.gradient(pts, axis=0)
    velocity = 3.0 * tangent / np.linalg.norm(tangent, axis=1)[:, None]
    return dict(speed=(0.5, 6.0, 16), velocity=velocity, boresight='ram', half_angle=half_angle)


def test_end_to_end(ctx, tmp_path):
    inputs = Input(INPUT, savepath=str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2e4, packs_per_it=5000, seed=17, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 4 and all(o.resident_rows(ctx) is not None for o in outs)
    xs, ys, zs = trajectory(200)
    pts = np.stack([xs, ys, zs], axis=1)
    dr = 0.05
    spectrum = ram_spectrum(pts)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ModelDensity(inputs, xs, ys, zs, dr=dr, spectrum=spectrum, context=ctx)
        sky = ModelDensity(inputs, xs, ys, zs, dr=dr, spectrum=dict(spectrum, half_angle=180.),
                           context=ctx)
        plain = ModelDensity(inputs, xs, ys, zs, dr=dr, context=ctx)
    cols = flow_columns(outs, ctx)
    want = restate(pts, dr, *model_spec(inputs, pts, spectrum), *cols)
    assert want.counts.sum() > 300 and 50 < want.seen.sum() < want.counts.sum()
    assert (want.seen[:, 1:-1].sum(axis=0) > 0).sum() >= 4
    check_model(model, want, 'resident')
    # the whole sky: every row within dr is in view
    want_sky = restate(pts, dr, *model_spec(inputs, pts, dict(spectrum, half_angle=180.)), *cols)
    assert np.array_equal(want_sky.seen.sum(axis=1), want_sky.counts)
    check_model(sky, want_sky, 'all sky')
    np.testing.assert_allclose(sky.density_in_view, sky.density, rtol=1e-12, atol=0)
    # without spectrum= on the same run: today's attributes, and nothing else
    assert np.array_equal(plain.packets, model.packets)
    assert plain.atoms_per_packet == model.atoms_per_packet
    np.testing.assert_allclose(plain.density, model.density, rtol=1e-12, atol=0)
    assert not hasattr(plain, 'spectrum_sums') and not hasattr(plain, 'flux')
    # the restored .npz Outputs: host float32 columns
    with contextlib.redirect_stdout(io.StringIO()):
        restored = Input(INPUT)
        for k, f in enumerate(inputs.search()[1]):
            back = Output.restore(f)
            back.idnum = k + 1
            restored._catalogue.append(back)
        host = ModelDensity(restored, xs, ys, zs, dr=dr, spectrum=spectrum, context=ctx)
    want_host = restate(pts, dr, *model_spec(inputs, pts, spectrum), *flow_columns(restored._catalogue))
    assert np.array_equal(host.packets, model.packets)
    check_model(host, want_host, 'restored')


def test_end_to_end_adaptive_step(ctx):
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(9000., 's')
    inputs.options.step_size = 0.
    inputs.options.resolution = 1e-4
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2000, packs_per_it=1000, seed=19, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert all(o.resident_rows(ctx) is not None for o in outs)
    cols = flow_columns(outs, ctx)
    rng = np.random.default_rng(56)
    assert len(cols[0]) > 300                     # one row per packet that is still there
    pick = rng.choice(len(cols[0]), 150, replace=False)
    pts = np.concatenate([np.stack(cols[:3], axis=1)[pick], [[90., 90., 90.]]])
    dr = 0.2
    spectrum = dict(speed=(0.5, 6.0, 16), velocity=rng.normal(0, 2., pts.shape), boresight='ram',
                    half_angle=75.)
    with contextlib.redirect_stdout(io.StringIO()):
        model = ModelDensity(inputs, *pts.T, dr=dr, spectrum=spectrum, context=ctx)
    want = restate(pts, dr, *model_spec(inputs, pts, spectrum), *cols)
    assert want.counts.sum() > 150 and 20 < want.seen.sum() < want.counts.sum()
    check_model(model, want, 'adaptive')
