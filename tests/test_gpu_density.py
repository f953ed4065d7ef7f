"""ModelDensity on the GPU against scipy.spatial.KDTree.query_ball_point -- the very call the
reference makes (ModelDensity.py:66-76) -- through the three ways rows reach k_density (float32
and float64 row stores, host columns), end to end against a restatement of ModelDensity.py:56-85,
and at full size (Input.run(1e6), 1.3e8 rows resident)."""
import contextlib
import io
import os

import numpy as np
import pytest
from scipy.spatial import KDTree

import nexoclom_amd
from nexoclom_amd import Input, ModelDensity, Output
from nexoclom_amd.ModelDensity import DensityIndex

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')


def kdtree_sums(points, dr, x, y, z, frac):
    """ModelDensity.py:66-76 for one Output: (frac sums, counts) per point."""
    data = np.stack([np.asarray(c, dtype=np.float64) for c in (x, y, z)], axis=1)
    found = KDTree(data).query_ball_point(points, dr)
    frac = np.asarray(frac, dtype=np.float64)
    return (np.array([frac[f].sum() for f in found]),
            np.array([len(f) for f in found], dtype=np.float64))


def device_sums(ctx, points, dr, *, columns=None, rows=None):
    index = DensityIndex(points, dr)
    ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    if rows is not None:
        ctx.density_accumulate(rows=rows)
    else:
        ctx.density_accumulate(*columns)
    s, c = ctx.density_download()
    return index.scatter(s, len(points)), index.scatter(c, len(points))


def check(got, want):
    assert np.array_equal(got[1], want[1])
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12, atol=0)


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


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_kernel_matches_kdtree_on_host_columns(ctx, dtype):
    rng = np.random.default_rng(1)
    dr = 0.05
    # random sets
    rows = rng.uniform(-1, 1, (200_000, 3)).astype(dtype)
    frac = rng.uniform(0, 1, 200_000).astype(dtype)
    pts = np.concatenate([rng.uniform(-1.1, 1.1, (2000, 3)), rows[:50].astype(np.float64)])
    cols = (rows[:, 0], rows[:, 1], rows[:, 2], frac)
    got = device_sums(ctx, pts, dr, columns=cols)
    want = kdtree_sums(pts, dr, *cols)
    check(got, want)
    assert want[1].sum() > 10_000
    # boundary set: rows on the spheres, +-1 ulp
    q, ring = boundary_points(dr, rng, 60_000, dtype)
    ring_frac = rng.uniform(0, 1, len(ring)).astype(dtype)
    cols = (ring[:, 0], ring[:, 1], ring[:, 2], ring_frac)
    got = device_sums(ctx, q, dr, columns=cols)
    want = kdtree_sums(q, dr, *cols)
    check(got, want)
    assert want[1].sum() > len(q)
    # duplicate points, one point, points far from every row
    dup = np.repeat(pts[:7], 5, axis=0)
    check(device_sums(ctx, dup, dr, columns=cols), kdtree_sums(dup, dr, *cols))
    one = q[:1]
    got = device_sums(ctx, one, dr, columns=cols)
    check(got, kdtree_sums(one, dr, *cols))
    assert got[1][0] >= 1
    away = np.array([[50., 50., 50.], [-30., 0., 0.], [0., 0., 1e6]])
    got = device_sums(ctx, away, dr, columns=cols)
    assert np.array_equal(got[1], [0, 0, 0]) and np.array_equal(got[0], [0, 0, 0])


def test_second_trip_of_the_grid_stride_loop(ctx):
    """2^20 + 65 rows: more than the 256 CUs x 8 workgroups x 256 threads that one full grid of
    k_density holds at most on an MI355X, so the workgroups stride on to a ragged second trip."""
    rng = np.random.default_rng(3)
    p, dr = 2**20 + 65, 0.05
    rows = rng.uniform(-1, 1, (p, 3))
    frac = rng.uniform(0, 1, p)
    pts = np.concatenate([rng.uniform(-1, 1, (300, 3)), rows[-3:]])
    cols = (rows[:, 0], rows[:, 1], rows[:, 2], frac)
    want = kdtree_sums(pts, dr, *cols)
    check(device_sums(ctx, pts, dr, columns=cols), want)
    assert want[1].sum() > 10_000 and want[1][-1] >= 1


@pytest.mark.parametrize('narrow', [True, False])
def test_kernel_matches_kdtree_on_row_stores(ctx, narrow):
    """Rows as Input.run leaves them in HBM (float32, what save() keeps) or 64-bit
    (save=False), read where they are."""
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(9000., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, 3000, seed=8, context=ctx, save=narrow)
    view = out.resident_rows(ctx)
    assert view is not None and view[0].narrow == narrow
    store, first, count, _ = view
    rows, _ = store.download(first, count, index=False)
    x, y, z, frac = rows[1], rows[2], rows[3], rows[7]
    rng = np.random.default_rng(2)
    dr = 0.05
    xyz = np.stack([x, y, z], axis=1).astype(np.float64)
    pick = xyz[rng.choice(count, 1500, replace=False)]
    u = rng.normal(size=pick.shape)
    u /= np.linalg.norm(u, axis=1)[:, None]
    on = pick - dr*u                              # a row on the sphere of radius dr around each
    pts = np.concatenate([on, np.nextafter(on, on + u), np.nextafter(on, on - u),
                          pick + rng.normal(0, 0.05, pick.shape), np.repeat(pick[:3], 4, axis=0),
                          [[40., 40., 40.]]])
    got = device_sums(ctx, pts, dr, rows=(store, first, count))
    want = kdtree_sums(pts, dr, x, y, z, frac)
    check(got, want)
    assert want[1].sum() > 5000 and np.array_equal(got[1][-1:], [0])
    check(device_sums(ctx, pick[:1], dr, rows=(store, first, count)),
          kdtree_sums(pick[:1], dr, x, y, z, frac))


def reference_density(outputs, endtime, radius_km, pts, dr):
    """ModelDensity.py:56-85 restated with NumPy / scipy over each Output's X."""
    density, packets, totalsource = np.zeros(len(pts)), np.zeros(len(pts)), 0.
    for out in outputs:
        X = Output.restore(out).X
        s, c = kdtree_sums(pts, dr, X.x.values, X.y.values, X.z.values, X.frac.values)
        density += s
        packets += c
        totalsource += out.totalsource
    Vpix = 4/3/np.pi*dr**3 * (radius_km*1e5)**3
    atoms_per_packet = 1e23 / (totalsource / endtime)
    return density*atoms_per_packet/Vpix, packets, totalsource, Vpix


def trajectory(n):
    t = np.linspace(0, 1, n)
    return -2.5 + 5*t, -1.5 + 4*t, 0.6*np.sin(6*t)


def test_end_to_end_resident_restored_and_reference(ctx, tmp_path):
    inputs = Input(INPUT, savepath=str(tmp_path))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2e4, packs_per_it=5000, seed=17, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 4 and all(o.resident_rows(ctx) is not None for o in outs)
    rng = np.random.default_rng(5)
    tx, ty, tz = trajectory(300)
    xs = np.concatenate([tx, rng.uniform(-2, 2, 300)])
    ys = np.concatenate([ty, rng.uniform(-2, 2, 300)])
    zs = np.concatenate([tz, rng.uniform(-0.5, 0.5, 300)])
    dr = 0.05
    with contextlib.redirect_stdout(io.StringIO()):
        resident = ModelDensity(inputs, xs, ys, zs, dr=dr, context=ctx)
        restored = Input(INPUT)
        for k, f in enumerate(inputs.search()[1]):
            back = Output.restore(f)
            back.idnum = k + 1
            restored._catalogue.append(back)
        host = ModelDensity(restored, xs, ys, zs, dr=dr, context=ctx)
        density, packets, totalsource, Vpix = reference_density(
            inputs._catalogue, inputs.options.endtime.value,
            inputs.geometry.planet.radius.value, np.stack([xs, ys, zs], axis=1), dr)
    assert packets.sum() > 1000
    for d in (resident, host):
        assert np.array_equal(d.packets, packets)
        np.testing.assert_allclose(d.density, density, rtol=1e-12, atol=0)
        assert d.totalsource == totalsource and float(d.Vpix) == Vpix
    assert resident.npackets == 20000


def test_full_size_resident_run(ctx):
    """Input.run(1e6): 1.3e8 float32 rows in HBM.  A 2 000-point trajectory and a 32^3 grid; 50
    of those points checked by brute force over every downloaded row (counts exact); two runs
    agree (counts identical, density to 1e-13)."""
    inputs = Input(INPUT)
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(1e6, seed=99, context=ctx)
    assert sum(o.resident_rows(ctx)[2] for o in inputs._catalogue) > 1.2e8
    tx, ty, tz = trajectory(2000)
    g = np.linspace(-3, 3, 32)
    gx, gy, gz = (a.ravel() for a in np.meshgrid(g, g, g, indexing='ij'))
    xs, ys, zs = np.concatenate([tx, gx]), np.concatenate([ty, gy]), np.concatenate([tz, gz])
    with contextlib.redirect_stdout(io.StringIO()):
        first = ModelDensity(inputs, xs, ys, zs, context=ctx)
        second = ModelDensity(inputs, xs, ys, zs, context=ctx)
    assert np.array_equal(first.packets, second.packets)
    np.testing.assert_allclose(second.density, first.density, rtol=1e-13, atol=0)
    rng = np.random.default_rng(6)
    hit = np.flatnonzero(first.packets > 0)
    check_at = np.concatenate([rng.choice(hit, 40, replace=False),
                               rng.choice(len(xs), 10, replace=False)])
    q = np.stack([xs[check_at], ys[check_at], zs[check_at]], axis=1)
    dr = 0.05
    counts, kd = np.zeros(len(q)), np.zeros(len(q))
    box = dr*(1 + 1e-9)
    for out in inputs._catalogue:
        store, first_row, count, _ = out.resident_rows(ctx)
        rows, _ = store.download(first_row, count, index=False)
        x, y, z = (rows[c].astype(np.float64) for c in (1, 2, 3))
        for j, (qx, qy, qz) in enumerate(q):
            near = np.flatnonzero(np.abs(x - qx) <= box)
            near = near[(np.abs(y[near] - qy) <= box) & (np.abs(z[near] - qz) <= box)]
            dx, dy, dz = qx - x[near], qy - y[near], qz - z[near]
            counts[j] += np.count_nonzero((dx*dx + dy*dy) + dz*dz <= dr*dr)
            if len(near):      # and the reference's own call over the same rows
                sub = np.stack([x[near], y[near], z[near]], axis=1)
                kd[j] += KDTree(sub).query_ball_point(q[j], dr, return_length=True)
    assert np.array_equal(first.packets[check_at], counts)
    assert np.array_equal(counts, kd)
    assert counts.sum() > 1000
