"""k_density_moments on the GPU against tests/density_moments_restatement.py: the ten moment sums,
S0 and the counts per point, through host columns (float64, float32), row stores and the
ModelDensity(moments=True) flow.  Device and restatement add bit-identical terms, so every sum is
held to the summation bound derived there ((n - 1) 2^-52 sum|term| per point and sum); counts and
membership are scipy's."""
import contextlib
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import Input, ModelDensity, Output, constants, hip_api
from nexoclom_amd.ModelDensity import DensityIndex, moments_from_sums
from tests.density_moments_restatement import check, restate

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
BULK = np.array([2e-4, -1e-4, 5e-5])             # R/s


def make_rows(rng, p, dtype=np.float64, xyz=None):
    """Seven columns x, y, z, vx, vy, vz, frac: positions uniform in [-1, 1]^3 (or ``xyz``),
    velocities a bulk plus a normal of 1e-4 R/s (first moments cancel in part), frac in (0, 1)."""
    xyz = rng.uniform(-1, 1, (p, 3)) if xyz is None else np.asarray(xyz)
    v = BULK + rng.normal(0, 1e-4, (len(xyz), 3))
    frac = rng.uniform(0, 1, len(xyz))
    return tuple(np.ascontiguousarray(c, dtype=dtype)
                 for c in (*xyz.astype(dtype).T, *v.T, frac))


def boundary_points(dr, rng, n, dtype):
    """Rows on spheres of radius dr around query points, each also nudged by one ulp (of the
    rows' type) towards and away from its point: (points, rows)."""
    q = rng.uniform(-1, 1, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    on = (q + dr*u).astype(dtype)
    far = np.nextafter(on, (on + np.sign(u)).astype(dtype))
    near = np.nextafter(on, (on - np.sign(u)).astype(dtype))
    return q, np.concatenate([on, far, near])


def download(ctx, index, Q):
    s0, counts = ctx.density_download()
    sums = np.zeros((Q, 10))
    sums[index.order] = ctx.density_moments_download()
    return sums, index.scatter(s0, Q), index.scatter(counts, Q)


def device_moments(ctx, points, dr, calls):
    """(sums (Q, 10), S0, counts) in the points' order after one set, one enable and one
    accumulate per item of ``calls`` (seven columns, or ('rows', (store, first, count)))."""
    index = DensityIndex(points, dr)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    ctx.density_moments_enable()
    for call in calls:
        if isinstance(call[0], str):
            ctx.density_moments_accumulate(rows=call[1])
        else:
            ctx.density_moments_accumulate(*call)
    return download(ctx, index, len(points))


def device_plain(ctx, points, dr, call):
    """k_density over the same samples with the moments enabled: (S0, counts, moment block)."""
    index = DensityIndex(points, dr)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    ctx.density_moments_enable()
    if isinstance(call[0], str):
        ctx.density_accumulate(rows=call[1])
    else:
        x, y, z, _, _, _, frac = call
        ctx.density_accumulate(x, y, z, frac)
    sums, s0, counts = download(ctx, index, len(points))
    return s0, counts, sums


def both_paths(ctx, points, dr, call, want, label):
    """Case 5: k_density_moments against the restatement, then k_density's {S0, count} over the
    same samples: counts equal, S0 within the bound, and the moment block untouched."""
    got = device_moments(ctx, points, dr, [call])
    check(*got, want, label)
    s0, counts, block = device_plain(ctx, points, dr, call)
    assert np.array_equal(counts, got[2])
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0)
    assert not block.any()
    return got


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns_match_the_restatement(ctx, dtype):
    rng = np.random.default_rng(21)
    dr = 0.1
    cols = make_rows(rng, 50_000, dtype)
    pts = np.concatenate([rng.uniform(-1, 1, (500, 3)),
                          np.stack(cols[:3], axis=1)[:50].astype(np.float64)])
    want = restate(pts, dr, *cols)
    assert want.counts.sum() > 10_000 and want.counts[-50:].min() >= 1
    both_paths(ctx, pts, dr, cols, want, f'columns {np.dtype(dtype).name}')
    # boundary set: rows on the spheres, +-1 ulp; membership must still be scipy's
    q, ring = boundary_points(dr, rng, 6000, dtype)
    cols = make_rows(rng, len(ring), dtype, xyz=ring)
    want = restate(q, dr, *cols)
    assert want.counts.sum() > len(q)
    check(*device_moments(ctx, q, dr, [cols]), want, 'boundary')


def wave_case(name, rng):
    """(points, dr, list of column sets): shapes at which the wave-cooperative adds can go wrong.
    One point at the origin, dr = 0.1; a row 'hits' close to it and 'misses' 0.13 away along x,
    still a candidate of the walk (its cell or the next)."""
    dr = 0.1
    pts = np.zeros((1, 3))

    def lanes(hit):
        hit = np.asarray(hit, dtype=bool)
        xyz = rng.normal(0, 0.005, (len(hit), 3))
        xyz[~hit] += [0.13, 0., 0.]
        return make_rows(rng, len(hit), xyz=xyz)
    lower = np.arange(64) < 32
    only = lambda k: np.arange(64) == k                                   # noqa: E731
    if name.startswith('p='):
        p = int(name[2:])
        cols = make_rows(rng, p, xyz=rng.normal(0, 0.03, (p, 3)))      # nearly all hit the origin
        return np.concatenate([pts, rng.normal(0, 0.08, (5, 3))]), dr, [cols]
    if name == 'identical':
        cols = tuple(np.repeat(c[:1], 64) for c in make_rows(rng, 1, xyz=[[0.01, 0.02, -0.03]]))
        return pts, dr, [cols]
    if name == 'same position':
        return np.zeros((2, 3)), dr, [make_rows(rng, 130, xyz=rng.normal(0, 0.06, (130, 3)))]
    if name == 'two launches':
        return (np.concatenate([pts, [[0.05, 0., 0.]]]), dr,
                [make_rows(rng, 70, xyz=rng.normal(0, 0.06, (70, 3))) for _ in range(2)])
    hit = {'lower hit': lower, 'upper hit': ~lower, 'lane 0': only(0), 'lane 63': only(63)}[name]
    return pts, dr, [lanes(hit)]


WAVE_CASES = ['p=1', 'p=63', 'p=64', 'p=65', 'p=257', 'identical', 'lower hit', 'upper hit',
              'lane 0', 'lane 63', 'same position', 'two launches']


@pytest.mark.parametrize('name', WAVE_CASES)
def test_wave_shapes(ctx, name):
    pts, dr, calls = wave_case(name, np.random.default_rng(WAVE_CASES.index(name)))
    merged = tuple(np.concatenate(c) for c in zip(*calls))
    want = restate(pts, dr, *merged)
    expected_hits = {'identical': 64, 'lower hit': 32, 'upper hit': 32, 'lane 0': 1, 'lane 63': 1}
    if name in expected_hits:
        assert want.counts[0] == expected_hits[name]
    else:
        assert want.counts.sum() >= 1
    check(*device_moments(ctx, pts, dr, calls), want, name)


def test_second_trip_of_the_grid_stride_loop(ctx):
    """2^20 + 65 rows: more than the 256 CUs x 8 workgroups x 256 threads of a full grid at the
    highest occupancy a 256-thread kernel can have (k_density_moments, with more registers, holds
    fewer), so the workgroups stride on to a ragged second trip."""
    rng = np.random.default_rng(23)
    p, dr = 2**20 + 65, 0.05
    cols = make_rows(rng, p)
    pts = np.concatenate([rng.uniform(-1, 1, (300, 3)), np.stack(cols[:3], axis=1)[-3:]])
    want = restate(pts, dr, *cols)
    assert want.counts.sum() > 10_000 and want.counts[-1] >= 1
    check(*device_moments(ctx, pts, dr, [cols]), want, 'second trip')


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
    rng = np.random.default_rng(22)
    dr = 0.05
    xyz = np.stack(rows[1:4], axis=1).astype(np.float64)
    pick = xyz[rng.choice(count, 750, replace=False)]
    pts = np.concatenate([pick, pick + rng.normal(0, 0.05, pick.shape)])
    want = restate(pts, dr, *rows[1:8])
    assert want.counts.sum() > 2000
    both_paths(ctx, pts, dr, ('rows', (store, first, count)), want, f'rows narrow={narrow}')
    a, n = count // 3, count // 2
    want = restate(pts, dr, *(r[a:a + n] for r in rows[1:8]))
    assert 0 < want.counts.sum()
    check(*device_moments(ctx, pts, dr, [('rows', (store, first + a, n))]), want, 'sub-range')


def test_entries(ctx):
    rng = np.random.default_rng(24)
    cols = make_rows(rng, 4000)
    pts = rng.uniform(-1, 1, (40, 3))
    dr = 0.2
    fresh = hip_api.Context(0)
    try:
        with pytest.raises(hip_api.HipError, match='nxc_density_set has not been called') as err:
            fresh.density_moments_accumulate(*cols)
        assert err.value.code == hip_api.NXC_ERR_STATE
        with pytest.raises(hip_api.HipError, match='nxc_density_set has not been called') as err:
            fresh.density_moments_enable()
        assert err.value.code == hip_api.NXC_ERR_STATE
        index = DensityIndex(pts, dr)
        args = (index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
        fresh.density_set(*args)
        for call in (lambda: fresh.density_moments_accumulate(*cols),
                     fresh.density_moments_download):
            with pytest.raises(hip_api.HipError, match='nxc_density_moments_enable has not') as err:
                call()
            assert err.value.code == hip_api.NXC_ERR_STATE
        fresh.density_moments_enable()
        import ctypes as C
        ptrs = [c.ctypes.data_as(C.POINTER(C.c_double)) for c in cols]
        for null in (0, 3, 5, 6):
            with_null = list(ptrs)
            with_null[null] = None
            rc = fresh.lib.nxc_density_moments_accumulate(fresh._h, C.c_int64(len(cols[0])), *with_null)
            assert rc == hip_api.NXC_ERR_ARG
        assert fresh.lib.nxc_density_moments_accumulate(fresh._h, C.c_int64(-1), *ptrs) == hip_api.NXC_ERR_ARG
        # p = 0 is accepted (null columns too) and adds nothing
        assert fresh.lib.nxc_density_moments_accumulate(fresh._h, C.c_int64(0), *[None]*7) == 0
        sums, s0, counts = download(fresh, index, len(pts))
        assert not sums.any() and not s0.any() and not counts.any()
        fresh.density_moments_accumulate(*cols)
        want = restate(pts, dr, *cols)
        assert want.counts.sum() > 100
        check(*download(fresh, index, len(pts)), want, 'entries')
        # a new density_set zeroes and disables
        fresh.density_set(*args)
        with pytest.raises(hip_api.HipError, match='nxc_density_moments_enable has not'):
            fresh.density_moments_accumulate(*cols)
        fresh.density_moments_enable()
        sums, s0, counts = download(fresh, index, len(pts))
        assert not sums.any() and not s0.any() and not counts.any()
        # Q = 0: accepted, nothing to add to
        none = DensityIndex(np.zeros((0, 3)), dr)
        fresh.density_set(none.points, none.cell_start, none.origin, none.h, none.dr, none.dims)
        fresh.density_moments_enable()
        fresh.density_moments_accumulate(*cols)
        assert fresh.density_moments_download().shape == (0, 10)
    finally:
        fresh.close()


def test_other_consumers_are_unchanged_after_a_moments_call(ctx):
    """density_accumulate, image_accumulate and camera_accumulate on the handle that has just
    served density_moments_accumulate: the values taken before that call come back.  Counts
    are compared exactly; the weight sums to 1e-12 relative, the tolerance the existing tests of
    these three consumers use for sums of positive terms added by atomics in a free order
    (tests/test_gpu_density.py, tests/test_gpu_api.py).  Each pixel or point here sums at most a
    few thousand positive terms, whose order alone moves the sum by at most n 2^-52 < 1e-12."""
    rng = np.random.default_rng(25)
    cols = make_rows(rng, 20_000)
    x, y, z, vx, vy, vz, frac = cols
    pts = rng.uniform(-1, 1, (60, 3))
    dr = 0.15
    index = DensityIndex(pts, dr)
    edges = np.linspace(-1, 1, 25)
    cam_edges = np.linspace(-0.3, 0.3, 21)

    def others():
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                        index.dims)
        ctx.density_accumulate(x, y, z, frac)
        ctx.set_image(np.eye(3), 0.0, 1.0, 'column', edges, edges, [])
        ctx.image_accumulate(x, y, z, vy, frac)
        ctx.camera_set((0., -6., 0.), np.eye(3), 0.0, 1.0, 'column', cam_edges, cam_edges)
        ctx.camera_accumulate(x, y, z, vy, frac)
        return (*ctx.density_download(), *ctx.image_download(), *ctx.camera_download())
    before = others()
    assert before[1].sum() > 100 and before[3].sum() > 1000 and before[5].sum() > 1000
    check(*device_moments(ctx, pts, dr, [cols]), restate(pts, dr, *cols), 'between')
    after = others()
    for k in (1, 3, 5):                                      # counts
        assert np.array_equal(after[k], before[k])
    for k in (0, 2, 4):                                      # sums: the atomics' order is free
        np.testing.assert_allclose(after[k], before[k], rtol=1e-12, atol=0)


def trajectory(n):
    t = np.linspace(0, 1, n)
    return -2.5 + 5*t, -1.5 + 4*t, 0.6*np.sin(6*t)


def flow_columns(outputs, ctx=None):
    """x, y, z, vx, vy, vz, frac of every Output, as ModelDensity reads them: the resident rows
    (downloaded) with ``ctx``, else X."""
    per_output = []
    for out in outputs:
        view = out.resident_rows(ctx) if ctx is not None else None
        if view is not None:
            rows, _ = view[0].download(view[1], view[2], index=False)
            per_output.append([np.asarray(r, dtype=np.float64) for r in rows[1:8]])
        else:
            per_output.append([out.X[c].values.astype(np.float64)
                               for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')])
    return [np.concatenate(c) for c in zip(*per_output)]


def check_model(model, want, pts, inputs):
    """``moment_sums`` within the bound, the frac sums and counts, and the quotients against the
    host formulas applied to the restatement's sums.

    ``velocity``, per component: u_a = R S1_a / S0, where S1_a is within b1 = (n - 1) 2^-52
    sum|f v_a| and S0 within b0 = (n - 1) 2^-52 sum|f| of the restatement's (``want.bound``), so
    the quotients differ by at most R (b1 / S0 + |S1_a| b0 / S0^2) to first order, and the
    division and the product with R add two roundings on either side, 4 * 2^-53 |u_a|.  Beside it
    the 1e-12 of the issue, relative to the point's speed |u|: a component whose terms cancel to
    nothing has no relative accuracy of its own in any order of addition.

    The covariance bound.  C_ab = S2_ab/S0 - u_a u_b is a difference of two numbers of size
    <v^2> = (S2_xx + S2_yy + S2_zz)/S0.  S2_ab and S0 carry a relative summation error of at most
    (n - 1) 2^-52 each (positive terms for the diagonal; |S2_ab| terms are bounded by the
    diagonal's), S1_a of at most (n - 1) 2^-52 sum|f v_a| <= (n - 1) 2^-52 S0 sqrt(<v^2>), which
    enters u_a u_b twice; the divisions, products and the subtraction add a few 2^-53 <v^2>.
    Together below (4 (n - 1) + 4) 2^-52 <v^2> <= n 2^-50 <v^2> per entry.  The temperature is
    m 1e6 / (3 k_B) times the trace: three entries, and five more roundings of at most 2^-53 <v^2>
    each, which is less than one more n 2^-50 <v^2>.  effective_packets = S0^2 / sum f^2 has
    positive terms only: relative (n - 1) 2^-52 for each of the three factors, and three
    roundings."""
    R = float(inputs.geometry.planet.radius.value)
    mass = constants.ATOMIC_MASS[inputs.options.species] * constants.AMU
    u, cov, temp, eff = moments_from_sums(want.s0, want.sums, R, mass)
    hit = want.counts > 0
    assert hit.sum() > 20 and (~hit).sum() > 0
    assert model.velocity.shape == (len(pts), 3) and model.velocity_covariance.shape == (len(pts), 3, 3)
    s0 = want.s0[hit][:, None]
    tol_u = R*(want.bound[hit, :3]/s0 + np.abs(want.sums[hit, :3])*want.bound_s0[hit][:, None]/(s0*s0)) \
        + 4 * 2.0**-53 * np.abs(u[hit])
    assert np.all(np.abs(model.velocity[hit] - u[hit]) <= tol_u)
    speed = np.linalg.norm(u[hit], axis=1)[:, None]
    assert np.all(np.abs(model.velocity[hit] - u[hit]) <= 1e-12*speed)
    v2 = (want.sums[:, 3:6].sum(axis=1) / np.where(hit, want.s0, 1.)) * R*R
    tol = want.counts * 2.0**-50 * v2
    assert np.all(np.abs(model.velocity_covariance[hit] - cov[hit]) <= tol[hit, None, None])
    assert np.all(np.abs(model.temperature[hit] - temp[hit])
                  <= mass*1e6/(3*constants.K_B) * 4*tol[hit])
    assert np.all(np.abs(model.effective_packets[hit] - eff[hit])
                  <= (3*want.counts[hit] + 3) * 2.0**-52 * eff[hit])
    assert np.all((eff[hit] >= 1 - 1e-12) & (eff[hit] <= want.counts[hit] * (1 + 1e-12)))
    assert np.isnan(model.velocity[~hit]).all() and np.isnan(model.temperature[~hit]).all()
    assert np.isnan(model.velocity_covariance[~hit]).all()
    assert not model.effective_packets[~hit].any()


def check_s0(model, want):
    """S0, which the object holds scaled into ``density`` (S0 * atoms_per_packet / Vpix): undoing
    that costs four more roundings, 4 * 2^-53 S0, beside the summation bound."""
    s0 = model.density * float(model.Vpix) / model.atoms_per_packet
    assert np.array_equal(model.packets, want.counts)
    assert np.all(np.abs(s0 - want.s0) <= want.bound_s0 + 4 * 2.0**-53 * want.s0)


def check_sums(model, want, label):
    """moment_sums, the counts and S0."""
    check(model.moment_sums, want.s0, model.packets, want, label)
    check_s0(model, want)


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
    with contextlib.redirect_stdout(io.StringIO()):
        model = ModelDensity(inputs, xs, ys, zs, dr=dr, moments=True, context=ctx)
        plain = ModelDensity(inputs, xs, ys, zs, dr=dr, moments=False, context=ctx)
    want = restate(pts, dr, *flow_columns(outs, ctx))
    assert want.counts.sum() > 300
    check_sums(model, want, 'resident')
    check_model(model, want, pts, inputs)
    # moments=False on the same run: today's attributes, and nothing else
    # (the order of the atomics is free, so the frac sums of the two objects are each held to
    # the summation bound against the restatement, i.e. to twice the bound against each other)
    assert np.array_equal(plain.packets, model.packets)
    check_s0(plain, want)
    assert plain.atoms_per_packet == model.atoms_per_packet
    assert float(plain.Vpix) == float(model.Vpix) and plain.totalsource == model.totalsource
    assert not hasattr(plain, 'velocity') and not hasattr(plain, 'moment_sums')
    # the restored .npz Outputs: host float32 columns
    with contextlib.redirect_stdout(io.StringIO()):
        restored = Input(INPUT)
        for k, f in enumerate(inputs.search()[1]):
            back = Output.restore(f)
            back.idnum = k + 1
            restored._catalogue.append(back)
        host = ModelDensity(restored, xs, ys, zs, dr=dr, moments=True, context=ctx)
    want_host = restate(pts, dr, *flow_columns(restored._catalogue))
    assert np.array_equal(host.packets, model.packets)
    check_sums(host, want_host, 'restored')


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
    rng = np.random.default_rng(26)
    assert len(cols[0]) > 300                     # one row per packet that is still there
    pick = rng.choice(len(cols[0]), 150, replace=False)
    pts = np.concatenate([np.stack(cols[:3], axis=1)[pick], [[90., 90., 90.]]])
    dr = 0.2
    with contextlib.redirect_stdout(io.StringIO()):
        model = ModelDensity(inputs, *pts.T, dr=dr, moments=True, context=ctx)
    want = restate(pts, dr, *cols)
    assert want.counts.sum() > 150
    check_sums(model, want, 'adaptive')
    check_model(model, want, pts, inputs)
