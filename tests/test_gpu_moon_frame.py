"""The moon-centred frame on the GPU: k_frame_rows through its three entries against the NumPy
restatement (tests/moon_frame_restatement.py), and the four products with a moon origin against
the composition of the entries they are made of -- the run's rows from HBM, moved on the host
columns' entry, handed to the product's own host-column entry with the moon's unit, g-value tables
and shifted vrplanet set by hand."""
import contextlib
import io
import os

import numpy as np
import pytest
from scipy.spatial import KDTree

import nexoclom_amd
from nexoclom_amd import CameraImage, Input, ModelDensity, ModelImage, Output, ShellMap, hip_api
from nexoclom_amd.CameraImage import camera_basis
from nexoclom_amd.ModelDensity import DensityIndex
from nexoclom_amd.ShellMap import shell_axes
from nexoclom_amd.atomicdata import gValue
from oracle import np_oracle as O
from tests import helpers as H
from tests import moon_frame_restatement as R
from tests.density_moments_restatement import products as density_terms
from tests.pixel_moments_restatement import image_moments

pytestmark = pytest.mark.gpu

IO_INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles', 'Na.io.torus.input')
RTOL = 1e-11
BLOCK = 256
GRID_THREADS = 256*8*BLOCK        # the grid's cap on the 256 CUs of an MI355X: one trip of the loop
# omega t reaches 12 rad over the 3000 s of the stores below; M_z = U_z = 0 as for any moon
FRAME = R.Frame(4.1e-3, np.array([-4.96, 3.19, 0.]), np.array([-1.3e-4, -2.0e-4, 0.]), 39.2)
OTHER = R.Frame(-7e-4, np.array([2.5, 1.25, 0.]), np.array([3e-4, -1e-4, 0.]), 0.75)


def quiet(make, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return make(*args, **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def check_moved(frame, t, state, got, label=''):
    """got (6, n) against the restatement of the rows (t, state (6, n)): z' and vz' bit-equal, x',
    y', vx', vy' within the bound of the definition (fp64), plus one float32 ulp of the expected
    value for float32 rows."""
    assert got.dtype == state[0].dtype and got.shape == (6, len(t)), label
    wide = [np.asarray(c, dtype=np.float64) for c in (t, *state)]
    want = R.move_rows(frame, *wide)                                          # fp64, unrounded
    pos, vel = R.bounds(frame, wide[1], wide[2], wide[4], wide[5])
    assert np.array_equal(bits(got[2]), bits(want[2].astype(got.dtype))), label
    assert np.array_equal(bits(got[5]), bits(want[5].astype(got.dtype))), label
    worst = 0.0
    for k, bound in ((0, pos), (1, pos), (3, vel), (4, vel)):
        if got.dtype == np.float32:
            bound = bound + R.f32_ulp(want[k])
        err = np.abs(got[k].astype(np.float64) - want[k])
        worst = max(worst, float(np.max(err/bound, initial=0.0)))
        assert np.all(err <= bound), (label, k)
    print(f'{label}: {len(t)} rows, worst error / bound {worst:.3f}')


# ---- 1. the kernel ------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[True, False], ids=['narrow', 'wide'])
def store(request, ctx):
    """Rows of a tiny constant-step run in HBM (float32 / int32, or 64-bit) and their host copy."""
    endtime, step = 3000., 30.
    X0 = H.sample_x0(300, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, H.mercury_forces('Na', 1.3))
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    st = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=request.param, resident=True)['store']
    try:
        assert st.narrow == request.param and st.total > 10000
        rows, index = st.download()
        assert FRAME.omega*float(rows[0].max()) > 2*np.pi
        yield st, rows, index
    finally:
        st.free()


def move_and_check(ctx, frame, st, rows, index, first, count, label):
    """Rows [first, first + count) through nxc_frame_rows: the copied columns bit for bit, the moved
    ones against the restatement and against the host-column entry of the same width."""
    moved = ctx.frame_rows(frame, st, first, count)
    try:
        assert moved.total == count and moved.narrow == st.narrow
        if count == 0:
            return None
        got, got_index = moved.download()
    finally:
        moved.free()
    src = rows[:, first:first + count]
    for c in (0, 7, 8):                                     # t, frac, lossfrac
        assert np.array_equal(bits(got[c]), bits(src[c])), (label, c)
    assert got_index.dtype == index.dtype and np.array_equal(got_index, index[first:first + count])
    check_moved(frame, src[0], src[1:7], got[1:7], label)
    columns = ctx.frame_columns(frame, *src[:7])
    assert columns.dtype == got.dtype and np.array_equal(bits(columns), bits(got[1:7])), label
    return got


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 1023, 1025, 2*BLOCK + 1, 8*BLOCK + 1])
@pytest.mark.parametrize('first', [777, 1000])
def test_rows_of_a_store(ctx, store, first, count):
    """Slices with first > 0 from an odd row (no column of the slice is 16-byte aligned: one row
    per thread) and from a multiple of four."""
    st, rows, index = store
    move_and_check(ctx, FRAME, st, rows, index, first, count, f'first {first} count {count}')


def test_the_whole_store_and_its_end(ctx, store):
    st, rows, index = store
    move_and_check(ctx, FRAME, st, rows, index, 0, st.total, 'whole')
    move_and_check(ctx, OTHER, st, rows, index, st.total - 333, 333, 'tail')
    move_and_check(ctx, FRAME, st, rows, index, st.total, 0, 'nothing at the end')


def test_aligned_rows_take_sixteen_bytes_a_thread(ctx, store):
    """A moved store of 1024 rows has every column on a 16-byte boundary, and so has the store it
    is moved into from a first row and a count that are multiples of four: the wide path of the
    rows entry against the restatement, and the identity gives back the rows.  (A count that is
    no multiple of four leaves the new store's columns unaligned: one row per thread again.  The
    wide path with rows left over is the host columns', whose device columns are always
    aligned.)"""
    st, rows, index = store
    base = ctx.frame_rows(FRAME, st, 776, 1024)
    try:
        host, host_index = base.download()
        again = move_and_check(ctx, R.IDENTITY, base, host, host_index, 0, 1024, 'identity, aligned')
        assert np.array_equal(bits(again), bits(host))
        move_and_check(ctx, OTHER, base, host, host_index, 4, 1016, 'aligned')
        move_and_check(ctx, OTHER, base, host, host_index, 0, 1021, 'aligned source only')
        move_and_check(ctx, OTHER, base, host, host_index, 4, 1, 'one row')
    finally:
        base.free()


def test_identity_returns_its_input(ctx, store):
    st, rows, index = store
    got = move_and_check(ctx, R.IDENTITY, st, rows, index, 5, 4001, 'identity')
    assert np.array_equal(bits(got), bits(rows[:, 5:4006]))


def cloud(n, seed, dtype):
    rng = np.random.default_rng(seed)
    cols = [rng.uniform(0, 3000, n)] + [rng.uniform(-7, 7, n) for _ in range(3)] + \
           [rng.uniform(-3e-4, 3e-4, n) for _ in range(3)]
    return [c.astype(dtype) for c in cols]


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025, 2*BLOCK + 1, 8*BLOCK + 1])
def test_host_columns(ctx, p, dtype):
    cols = cloud(p, 100 + p, dtype)
    got = ctx.frame_columns(FRAME, *cols)
    assert got.shape == (6, p) and got.dtype == dtype
    if p:
        check_moved(FRAME, cols[0], cols[1:], got, f'host columns {p}')
        same = ctx.frame_columns(R.IDENTITY, *cols)
        assert np.array_equal(bits(same), bits(np.stack(cols[1:])))


def test_second_trip_of_the_grid_stride_loop(ctx):
    """More 16-byte groups than one grid of threads (float64 host columns, two rows a thread), and
    more rows than that from an odd first row of a float32 store (one row a thread)."""
    p = 2*GRID_THREADS + 2*BLOCK + 3
    cols = cloud(p, 7, np.float64)
    check_moved(FRAME, cols[0], cols[1:], ctx.frame_columns(FRAME, *cols), 'second trip, columns')
    endtime, step = 3000., 30.
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, H.mercury_forces('Na', 1.3))
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(H.sample_x0(30000, 52, endtime))
    st = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=True, resident=True)['store']
    try:
        assert st.total > GRID_THREADS + BLOCK + 1, st.total
        rows, index = st.download()
        move_and_check(ctx, FRAME, st, rows, index, 1, st.total - 1, 'second trip, rows')
    finally:
        st.free()


def test_refusals(ctx, store):
    st, rows, index = store
    nan = float('nan')
    for bad in (R.Frame(nan, FRAME.M, FRAME.U, 1.0), R.Frame(1e-3, FRAME.M*nan, FRAME.U, 1.0),
                R.Frame(1e-3, FRAME.M, np.array([0., float('inf'), 0.]), 1.0),
                R.Frame(1e-3, FRAME.M, FRAME.U, 0.0), R.Frame(1e-3, FRAME.M, FRAME.U, -1.0)):
        with pytest.raises(hip_api.HipError, match='nxc_frame_desc'):
            ctx.frame_rows(bad, st, 0, 10)
        with pytest.raises(hip_api.HipError, match='nxc_frame_desc'):
            ctx.frame_columns(bad, *cloud(5, 1, np.float64))
    for first, count in ((-1, 5), (st.total + 1, 0), (0, st.total + 1), (st.total - 3, 4), (0, -1)):
        with pytest.raises(hip_api.HipError, match='outside the store'):
            ctx.frame_rows(FRAME, st, first, count)
    lib, desc = ctx.lib, hip_api.Context.frame_desc(FRAME)
    import ctypes as C
    assert lib.nxc_frame_rows(ctx._h, None, st._r, 0, 1, C.byref(C.c_void_p())) != 0
    assert b'description is null' in lib.nxc_last_error_string()
    assert lib.nxc_frame_columns(ctx._h, C.byref(desc), 3, *[None]*8) != 0
    assert b'column is null' in lib.nxc_last_error_string()
    assert lib.nxc_frame_columns(ctx._h, C.byref(desc), 0, *[None]*8) == 0
    # and the store is as it was
    after, _ = st.download()
    assert np.array_equal(bits(after), bits(rows))


# ---- 2. the products around Io ------------------------------------------------------------------------
def io_inputs(savepath=None, vprob=None):
    inputs = Input(IO_INPUT, savepath=savepath) if savepath else Input(IO_INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
    if vprob is not None:
        inputs.speeddist.vprob = type(inputs.speeddist.vprob)(vprob, 'km/s')
        inputs.speeddist.delv = type(inputs.speeddist.delv)(0.2, 'km/s')
    return inputs


class IoRun:
    """A run from Io with its rows in HBM, and what the composition needs of it by hand."""

    def __init__(self, ctx, savepath=None, vprob=None):
        self.ctx = ctx
        self.inputs = io_inputs(savepath, vprob)
        with contextlib.redirect_stdout(io.StringIO()):
            self.inputs.run(256, seed=5, context=ctx)
            self.inputs.wait()
        (self.out,) = self.inputs._catalogue
        assert self.out.resident_rows(ctx) is not None and self.out._store.narrow
        moon = self.out._bodies['moons'][0]
        assert moon['name'] == 'Io'
        self.frame = R.moon_frame(moon['radius'], moon['a'], moon['omega'], moon['phi'])
        jupiter_km = self.inputs.geometry.planet.radius.value
        self.io_km = next(m for m in self.inputs.geometry.planet.moons
                          if m.object == 'Io').radius.value
        np.testing.assert_allclose(self.frame.scale, jupiter_km/self.io_km, rtol=1e-14)
        self.aplanet = float(self.out.aplanet)
        # vy' + (vrplanet + U_y) is the Sun-relative radial velocity, in Io radii per second
        self.vr = (float(self.out.vrplanet) + self.frame.U[1]*jupiter_km)/self.io_km
        self.g_tables = [(t.velocity/self.io_km, t.g)
                         for t in (gValue('Na', w, self.aplanet) for w in (5891, 5897))]
        self.app = 1e23/(self.out.totalsource/6000.)
        rows, _ = self.out._host_rows()
        assert rows.dtype == np.float32 and rows.shape[1] > 2000
        self.rows = rows
        moved = ctx.frame_columns_f32(self.frame, *rows[:7])
        x, y, z, vx, vy, vz = moved
        self.five = (x, y, z, vy, rows[7])
        self.seven = (x, y, z, vx, vy, vz, rows[7])


@pytest.fixture(scope='module')
def io_run(ctx, tmp_path_factory):
    return IoRun(ctx, savepath=str(tmp_path_factory.mktemp('io_run')))


IMAGE = dict(origin='Io', dims='16,16', width='12,12')
XEDGES = np.linspace(-6, 6, 17)


def set_image_by_hand(run, quantity, img):
    apix = (12/16)**2*(run.io_km*1e5)**2
    np.testing.assert_allclose(float(img.Apix), apix, rtol=1e-14)
    run.ctx.set_image(img.image_rotation(), run.vr, apix, quantity, XEDGES, XEDGES,
                      run.g_tables if quantity == 'radiance' else [], downcast_f32=False)
    return apix


def compare_image(run, img, want_image, want_counts):
    assert want_counts.sum() > 1000
    assert np.array_equal(img.packet_image, want_counts.astype(float))
    np.testing.assert_allclose(img.image, want_image*run.app, rtol=RTOL, atol=0)
    np.testing.assert_allclose(img.atoms_per_packet, run.app, rtol=1e-14)
    assert img.unit == 'R_Io' and img.unit_km == run.io_km and img.counters['nonfinite'] == 0


@pytest.mark.parametrize('quantity', ['column', 'radiance'])
def test_model_image_around_io(io_run, quantity):
    run, ctx = io_run, io_run.ctx
    img = quiet(ModelImage, run.inputs, dict(IMAGE, quantity=quantity), context=ctx)
    set_image_by_hand(run, quantity, img)
    ctx.image_accumulate(*run.five)
    want_image, want_counts = ctx.image_download()
    compare_image(run, img, want_image, want_counts)
    assert img.counters['samples'] == run.rows.shape[1]
    # in slabs of 97 rows: the same counts, the same sums
    slabs = quiet(ModelImage, run.inputs, dict(IMAGE, quantity=quantity), context=ctx, slab_rows=97)
    compare_image(run, slabs, want_image, want_counts)
    assert slabs.counters['samples'] == run.rows.shape[1]
    # and run by run (create_image's own path)
    weighted, counted = quiet(img.create_image, run.out)
    assert np.array_equal(counted.histogram, want_counts.astype(float))
    np.testing.assert_allclose(weighted.histogram, want_image, rtol=RTOL, atol=0)


def test_model_image_moments_around_io(io_run):
    run, ctx = io_run, io_run.ctx
    img = quiet(ModelImage, run.inputs, dict(IMAGE, quantity='radiance'), context=ctx, moments=True)
    apix = set_image_by_hand(run, 'radiance', img)
    ctx.image_moments_enable()
    ctx.image_moments_accumulate(*run.seven)
    want_image, want_counts = ctx.image_download()
    want_sums = ctx.image_moments_download()
    compare_image(run, img, want_image, want_counts)
    # sum |term| per pixel and sum from the restatement of the pixel moments, over the moved rows
    restated = image_moments(*run.seven, run.vr, img.image_rotation(), 'radiance', run.g_tables,
                             (16, 16), [-6., 6.], [-6., 6.], apix)
    assert np.array_equal(restated.counts, want_counts)
    assert np.all(np.abs(img.moment_sums - want_sums) <= RTOL*restated.abs_sums)
    assert np.count_nonzero(want_sums[..., 0]) > 50
    # velocities relative to Io, in km/s: a cloud launched at 0.5 - 4.5 km/s
    seen = img.packet_image > 20
    # (read in Jupiter's frame they would carry Io's 17 km/s)
    assert seen.any() and np.all(np.abs(img.velocity[seen]) < 6) and np.all(img.velocity_dispersion[seen] < 6)


def test_model_image_cube_around_io(io_run):
    run, ctx = io_run, io_run.ctx
    img = quiet(ModelImage, run.inputs, dict(IMAGE, quantity='radiance'), context=ctx,
                cube=(-5, 5, 4))
    set_image_by_hand(run, 'radiance', img)
    ctx.image_cube_enable(4, -5/run.io_km, 5/run.io_km)
    ctx.image_cube_accumulate(*run.seven)
    want_image, want_counts = ctx.image_download()
    want_sums = ctx.image_cube_download()
    compare_image(run, img, want_image, want_counts)
    assert want_sums.shape == (16, 16, 6, 2) and img.cube_sums.shape == want_sums.shape
    np.testing.assert_allclose(img.cube_sums, want_sums, rtol=RTOL, atol=0)     # terms w, w w >= 0
    # Io-relative speeds: the four bins over +-5 km/s hold the cloud, and the planes sum to the image
    assert np.count_nonzero(want_sums[:, :, 1:-1, 0]) > 50
    assert want_sums[:, :, 1:-1, 0].sum() > 0.9*want_sums[..., 0].sum()
    np.testing.assert_allclose(want_sums[..., 0].sum(-1), want_image, rtol=1e-12, atol=0)


def test_camera_image_around_io(io_run):
    run, ctx = io_run, io_run.ctx
    params = dict(quantity='radiance', origin='Io', observer='0,-6,1', fov='60,60', dims='16,16')
    cam = quiet(CameraImage, run.inputs, params, context=ctx)
    observer = np.array([0., -6., 1.])
    basis = camera_basis(-observer, np.array([0., 0., 1.]))
    half = np.tan(np.radians(60.)/2)
    edges = np.linspace(-half, half, 17)
    area = (2*half/16)**2*(run.io_km*1e5)**2
    ctx.camera_set(observer, basis, run.vr, area, 'radiance', edges, edges, run.g_tables)
    ctx.camera_accumulate(*run.five)
    want_image, want_counts = ctx.camera_download()
    compare_image(run, cam, want_image, want_counts)


def test_shell_map_around_io(io_run):
    run, ctx = io_run, io_run.ctx
    params = dict(quantity='radiance', origin='Io', dims='12,6', altitude='0,4,4')
    sm = quiet(ShellMap, run.inputs, params, context=ctx)
    axes = shell_axes(12, 6, 0., 4., 4)
    ctx.shell_set(run.vr, 'radiance', axes['lon_edges'], axes['mu_edges'], 1.0, 5.0, 4, run.g_tables)
    ctx.shell_accumulate(*run.five)
    want_column, want_counts, want_sums = ctx.shell_download()
    assert want_counts.sum() > 1000 and np.array_equal(sm.packets, want_counts.astype(float))
    np.testing.assert_allclose(sm.shell_sums, want_sums, rtol=RTOL, atol=0)     # terms >= 0
    area = axes['solid_angle']*(run.io_km*1e5)**2
    np.testing.assert_allclose(sm.column, want_column*run.app/area, rtol=RTOL, atol=0)
    assert sm.unit == 'R_Io' and np.array_equal(sm.altitude_edges_km, sm.altitude_edges*run.io_km)


def test_model_density_around_io(io_run):
    run, ctx = io_run, io_run.ctx
    rng = np.random.default_rng(12)
    direction = rng.normal(size=(50, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    points = direction*rng.uniform(1.1, 3.0, 50)[:, None]              # within 3 R_Io of Io
    dr = 0.6
    index = DensityIndex(points, dr)
    args = (index.points, index.cell_start, index.origin, index.h, index.dr, index.dims)
    x, y, z, vx, vy, vz, frac = run.seven

    plain = quiet(ModelDensity, run.inputs, *points.T, dr=dr, origin='Io', context=ctx)
    ctx.density_set(*args)
    ctx.density_accumulate(x, y, z, frac)
    want_sums, want_counts = ctx.density_download()
    assert want_counts.sum() > 500 and np.count_nonzero(want_counts) > 20
    assert np.array_equal(plain.packets, index.scatter(want_counts, 50))
    scale = run.app/(4/3/np.pi*dr**3*(run.io_km*1e5)**3)
    np.testing.assert_allclose(plain.density, index.scatter(want_sums, 50)*scale, rtol=RTOL, atol=0)
    assert plain.unit == 'R_Io' and plain.origin.object == 'Io'

    moments = quiet(ModelDensity, run.inputs, *points.T, dr=dr, moments=True, origin='Io',
                    context=ctx)
    ctx.density_set(*args)
    ctx.density_moments_enable()
    ctx.density_moments_accumulate(x, y, z, vx, vy, vz, frac)
    want_sums, want_counts = ctx.density_download()
    want_moments = np.zeros((50, 10))
    want_moments[index.order] = ctx.density_moments_download()
    assert np.array_equal(moments.packets, index.scatter(want_counts, 50))
    # sum |term| per point and sum over the rows within dr, from the moved rows
    wide = [np.asarray(c, dtype=np.float64) for c in (x, y, z)]
    found = KDTree(np.stack(wide, axis=1)).query_ball_point(points, dr)
    assert np.array_equal([len(rows) for rows in found], moments.packets)
    terms = np.abs(density_terms(vx, vy, vz, frac))
    magnitude = np.array([terms[rows].sum(axis=0) for rows in found])
    assert np.all(np.abs(moments.moment_sums - want_moments) <= RTOL*magnitude)
    seen = moments.packets > 20
    assert seen.any() and np.all(np.linalg.norm(moments.velocity[seen], axis=1) < 6)    # km/s, Io's frame


def test_a_restored_run_gives_the_image_of_the_resident_rows(io_run):
    run, ctx = io_run, io_run.ctx
    (path,) = run.inputs.search()[1]
    assert os.path.exists(str(path))
    restored = io_inputs()
    back = Output.restore(str(path))
    back.idnum = 1
    restored._catalogue.append(back)
    assert back.resident_rows(ctx) is None and back.X['x'].dtype == np.float64
    params = dict(IMAGE, quantity='radiance')
    resident = quiet(ModelImage, run.inputs, params, context=ctx)
    host = quiet(ModelImage, restored, params, context=ctx)
    assert resident.packet_image.sum() > 1000
    assert np.array_equal(host.packet_image, resident.packet_image)
    np.testing.assert_allclose(host.image, resident.image, rtol=RTOL, atol=0)
    # and through sample_pass
    sm_params = dict(quantity='column', origin='Io', dims='12,6', altitude='0,4,4')
    from_file = quiet(ShellMap, restored, sm_params, context=ctx)
    from_rows = quiet(ShellMap, run.inputs, sm_params, context=ctx)
    assert np.array_equal(from_file.packets, from_rows.packets) and from_rows.packets.sum() > 1000
    np.testing.assert_allclose(from_file.shell_sums, from_rows.shell_sums, rtol=RTOL, atol=0)


# ---- 3. below Io's escape speed the cloud stays at Io ----------------------------------------------------
@pytest.fixture(scope='module')
def bound_run(ctx):
    return IoRun(ctx, vprob=1.0)


def test_a_bound_cloud_stays_inside_the_frame(bound_run):
    """Launched at 0.8 - 1.2 km/s every row lies within [1, 2] R_Io of Io (tests/
    test_moon_frame_cpu.py): an image 4 R_Io wide holds every sample, and nothing lies below the
    surface."""
    run, ctx = bound_run, bound_run.ctx
    img = quiet(ModelImage, run.inputs, dict(quantity='column', origin='Io', dims='16,16',
                                              width='4,4'), context=ctx)
    n = run.rows.shape[1]
    assert n > 2000 and img.counters['samples'] == n == img.counters['samples_binned']
    r = np.linalg.norm(np.stack(run.five[:3]).astype(np.float64), axis=0)
    assert 1.0 - 2e-5 <= r.min() and r.max() <= 2.0        # (float32 rows resolve 1.4e-5 R_Io)
    sm = quiet(ShellMap, run.inputs, dict(quantity='column', origin='Io', dims='12,6',
                                          altitude='0,1,4'), context=ctx)
    assert not sm.shell_sums[..., 0, :].any() and not sm.column_below.any()
    assert sm.shell_sums[..., 1:, :].any() and sm.counters['samples'] == n
    # seen from Jupiter's centre the same rows are smeared along Io's orbit: far outside 4 R_Io
    planet = quiet(ModelImage, run.inputs, dict(quantity='column', dims='16,16', width='1,1'),
                   context=ctx)
    assert planet.frame is None and planet.counters['samples'] == n
    assert planet.counters['samples_binned'] == 0


def test_the_planet_centred_image_of_these_inputs_is_the_oracles(ctx, coracle):
    """Without an origin nothing changed: the streamed image of the same inputs against the C
    oracle fed with the same packets and tables (tests/test_gpu_bodies.py, at these speeds)."""
    from nexoclom_amd.Output import n_output_steps
    inputs = io_inputs(vprob=1.0)
    n = 256
    params = {'quantity': 'radiance', 'dims': '32,32', 'width': '24,24'}
    img = quiet(ModelImage, inputs, params, npackets=n, seed=5, context=ctx)
    out = quiet(Output, inputs, n, seed=5, integrate=False, save=False, context=ctx)
    bd = out._bodies
    moons = bd['moons']
    b = O.Bodies(**{key: tuple(m[key] for m in moons) for key in ('gm', 'radius', 'a', 'omega', 'phi')},
                 t0=bd['t0'], chx_on=True, chx_k0=bd['chx']['k0'], chx_rho0=bd['chx']['rho0'],
                 chx_width=bd['chx']['width'], chx_height=bd['chx']['height'],
                 chx_omega=bd['chx']['omega'])
    kw = out.forces_kwargs()
    f = O.Forces(GM=kw['GM'], vrplanet=kw['vrplanet'], gravity=kw['gravity'], radpres=kw['radpres'],
                 lifetime=kw['lifetime'], photo=kw['photo'], v_tab=kw['v_tab'], a_tab=kw['a_tab'])
    _, n_iter = n_output_steps(6000., float(inputs.options.step_size))
    desc = coracle.image_desc(img.image_rotation(), f.vrplanet, float(img.Apix), 'radiance',
                              img.g_tables(out.aplanet), img.xedges, img.zedges, downcast=True)
    c = coracle.integrate_const(f, out.X0[['time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac']].values,
                                float(inputs.options.step_size), n_iter, inputs.options.outeredge,
                                img=desc, threads=4, bodies=b)
    assert np.array_equal(img.packet_image, c['counts'].astype(float))
    np.testing.assert_allclose(img.image, c['image']*img.atoms_per_packet, rtol=1e-10)
    assert img.packet_image.sum() > 1000 and img.frame is None
    ctx.set_bodies(None)
