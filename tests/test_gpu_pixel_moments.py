"""k_image_moments / k_camera_moments and the moments of ModelImage / CameraImage on the GPU against
tests/pixel_moments_restatement.py (the "Pixel moments" definition of include/nexoclom_hip.h
restated with NumPy on top of the oracle's create_image and tests/camera_restatement.py).

Comparison rule, everywhere: the restatement's two guards are asserted first (>= 1e-9: no binned
coordinate that close to a bin edge, no decision that close to its threshold -- a condition on the
inputs, which is what makes the exact comparison of counts legitimate); then counts and counters
must be equal exactly, the image to rtol 1e-11 (the project's figure for images summed in another
order) and each of the four sums to |got - want| <= 1e-11 * sum |term| per pixel -- the same figure
against the absolute sum, because m1 and m3 are signed and cancel."""
import contextlib
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import CameraImage, Input, ModelImage, Output, hip_api
from nexoclom_amd.CameraImage import camera_basis
from nexoclom_amd.ModelImage import PIXEL_MOMENT_COLUMNS, pixel_moments_from_sums
from oracle import np_oracle as O
from tests import helpers as H
from tests.pixel_moments_restatement import camera_moments, image_moments

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
GUARD = 1e-9
RTOL = 1e-11
ROWS_RTOL = 1e-12
R_KM = 2440.53

CAMERAS = {
    'outside': dict(o=(1.5, -6.0, 2.0), boresight=None, up=(0, 0, 1), fov=(40, 30)),
    'horizon': dict(o=(0.0, -1.2, 0.0), boresight=(1, 0, 0.05), up=(0, 0, 1), fov=(100, 80)),
    'oblique': dict(o=(3.0, -4.0, 2.5), boresight=(-0.5, 0.8, -0.3), up=(0.2, 0.1, 1), fov=(50, 35)),
}
ROTATIONS = {'x_is_x': (0.0, 0.4), 'general': (0.7, 0.4)}


@pytest.fixture(scope='module')
def forces():
    return H.mercury_forces('Na', 1.3)


def tables(forces, kind):
    if kind == 'column':
        return 'column', []
    if kind == 'constant':
        return 'radiance', [(np.array([-1e30, 1e30]), np.array([2.5, 2.5]))]
    return 'radiance', H.g_tables('Na', forces.aplanet, forces.R_km, (5891, 5897))


class ImageScene:
    """ModelImage's side: set_image / image_moments_* against image_moments."""
    name = 'image'

    def __init__(self, forces, dims=(64, 48), rotation='general'):
        self.forces, self.dims = forces, tuple(dims)
        self.im = H.image_setup(forces, 'column', dims=dims, sublon=ROTATIONS[rotation][0],
                                sublat=ROTATIONS[rotation][1])
        self.M = self.im['M']
        self.half = 4.0

    def place(self, a, b, depth):
        """Points at image coordinates (a, b) in units of the half width, in front of the planet."""
        obs = np.stack([a*self.half, -1.5 - depth, b*self.half], axis=1)
        return obs @ self.M                       # M^T obs per row

    def pixel_centre(self, ix, iz):
        xe, ze = self.im['xedges'], self.im['zedges']
        return ((xe[ix] + xe[ix + 1])/2/self.half, (ze[iz] + ze[iz + 1])/2/self.half,
                (xe[1] - xe[0])/self.half, (ze[1] - ze[0])/self.half)

    def set(self, ctx, quantity, gt, enable=True):
        ctx.set_image(self.M, self.forces.vrplanet, self.im['apix'], quantity, self.im['xedges'],
                      self.im['zedges'], gt)
        if enable:
            ctx.image_moments_enable()

    def restate(self, cols, quantity, gt):
        return image_moments(*cols, self.forces.vrplanet, self.M, quantity, gt, self.dims,
                             self.im['xrange'], self.im['zrange'], self.im['apix'])

    enable = staticmethod(lambda ctx, on=True: ctx.image_moments_enable(on))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.image_moments_accumulate(*a, **k))
    moments = staticmethod(lambda ctx: ctx.image_moments_download())
    pair = staticmethod(lambda ctx: ctx.image_download())

    @staticmethod
    def plain(ctx, x, y, z, vx, vy, vz, frac):
        ctx.image_accumulate(x, y, z, vy, frac)


class CameraScene:
    """CameraImage's side: camera_set / camera_moments_* against camera_moments."""
    name = 'camera'

    def __init__(self, forces, dims=(64, 48), camera='outside'):
        c = CAMERAS[camera]
        self.forces, self.dims = forces, tuple(dims)
        self.o = np.array(c['o'], dtype=float)
        bore = -self.o if c['boresight'] is None else np.array(c['boresight'], dtype=float)
        self.basis = camera_basis(bore, c['up'])
        self.halves = [np.tan(np.radians(f)/2) for f in c['fov']]
        self.uedges = np.linspace(-self.halves[0], self.halves[0], dims[0] + 1)
        self.vedges = np.linspace(-self.halves[1], self.halves[1], dims[1] + 1)
        self.area = (2*self.halves[0]/dims[0])*(2*self.halves[1]/dims[1])*(R_KM*1e5)**2

    def place(self, a, b, depth):
        right, bore, up = self.basis
        ray = bore + (a*self.halves[0])[:, None]*right + (b*self.halves[1])[:, None]*up
        return self.o + (2.0 + depth)[:, None]*ray

    def pixel_centre(self, ix, iz):
        ue, ve = self.uedges, self.vedges
        return ((ue[ix] + ue[ix + 1])/2/self.halves[0], (ve[iz] + ve[iz + 1])/2/self.halves[1],
                (ue[1] - ue[0])/self.halves[0], (ve[1] - ve[0])/self.halves[1])

    def set(self, ctx, quantity, gt, enable=True):
        ctx.camera_set(self.o, self.basis, self.forces.vrplanet, self.area, quantity, self.uedges,
                       self.vedges, gt)
        if enable:
            ctx.camera_moments_enable()

    def restate(self, cols, quantity, gt):
        return camera_moments(*cols, self.o, self.basis, self.uedges, self.vedges,
                              self.forces.vrplanet, self.area, quantity, gt)

    enable = staticmethod(lambda ctx, on=True: ctx.camera_moments_enable(on))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.camera_moments_accumulate(*a, **k))
    moments = staticmethod(lambda ctx: ctx.camera_moments_download())
    pair = staticmethod(lambda ctx: ctx.camera_download())

    @staticmethod
    def plain(ctx, x, y, z, vx, vy, vz, frac):
        ctx.camera_accumulate(x, y, z, vy, frac)


SCENES = {'image': ImageScene, 'camera': CameraScene}
both = pytest.mark.parametrize('which', sorted(SCENES))


def dress(xyz, rng, dtype=np.float64, frac=None):
    """Seven columns x y z vx vy vz frac for the positions xyz: seeded velocities and fractions."""
    n = len(xyz)
    vx, vz = rng.normal(size=n)*2.0/R_KM, rng.normal(size=n)*2.0/R_KM
    vy = rng.uniform(-0.02, 0.02, n)
    frac = rng.uniform(1e-6, 1.0, n) if frac is None else frac
    cols = (xyz[:, 0], xyz[:, 1], xyz[:, 2], vx, vy, vz, frac)
    return tuple(np.ascontiguousarray(np.asarray(c).astype(dtype)) for c in cols)


def cloud(p, seed, dtype=np.float64):
    """p samples around the planet, 1 to 6 radii out, in every direction."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(p, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return dress(d*rng.uniform(1.0, 6.0, p)[:, None], rng, dtype)


def restate(scene, cols, quantity, gt):
    want = scene.restate(cols, quantity, gt)
    print(f'{scene.name} guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e}; '
          f'{want.samples} samples, {want.binned} binned')
    assert want.edge_guard >= GUARD and want.margin_guard >= GUARD
    return want


def compare_sums(got, want, rtol=RTOL, reference=None):
    """|got - want| <= rtol * sum |term| per pixel and sum; the worst ratio is printed first."""
    reference = want.sums if reference is None else reference
    err = np.abs(got - reference)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(want.abs_sums > 0, err/want.abs_sums, np.where(err > 0, np.inf, 0.0))
    worst = ratio.reshape(-1, 4).max(axis=0) if ratio.size else np.zeros(4)
    print('worst |got - want| / sum|term| per sum', dict(zip(PIXEL_MOMENT_COLUMNS, worst)))
    assert np.all(err <= rtol*want.abs_sums)


def compare(ctx, scene, want, counters=None):
    image, counts = scene.pair(ctx)
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(image, want.image, rtol=RTOL, atol=0)
    sums = scene.moments(ctx)
    assert sums.shape == scene.dims + (4,)
    compare_sums(sums, want)
    if counters is not None:
        assert counters['samples'] == want.samples
        assert counters['samples_binned'] == want.binned == want.counts.sum()
        assert counters['nonfinite'] == 0
    return image, counts, sums


def check(ctx, scene, cols, kind):
    quantity, gt = tables(scene.forces, kind)
    want = restate(scene, cols, quantity, gt)
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, *cols)
    compare(ctx, scene, want, ctx.counters())
    return want


# ---- shapes ---------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, which, p):
    scene = SCENES[which](forces)
    want = check(ctx, scene, cloud(p, 100 + p), 'two')
    if p >= 1023:
        assert want.binned > 100 and np.count_nonzero(want.sums[..., 3]) > 50


@both
def test_second_trip_of_the_grid_stride_loop(ctx, forces, which):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    scene = SCENES[which](forces)
    want = check(ctx, scene, cloud(1_200_001, 9, np.float32), 'two')
    assert want.binned > 300_000


def wave_case(scene, case, seed):
    """64 samples (192 for 'gap') aimed at add_record_pairs' pairing of lanes l and l + 32."""
    rng = np.random.default_rng(seed)
    n = 192 if case == 'gap' else 64
    lane = np.arange(n) % 64
    a, b = rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n)
    depth = rng.uniform(0.0, 1.0, n)
    frac = rng.uniform(0.1, 1.0, n)
    inside = np.ones(n, dtype=bool)
    if case == 'lower':
        inside = lane < 32
    elif case == 'upper':
        inside = lane >= 32
    elif case == 'partners':                       # lanes l and l + 32 in the same pixel
        a[32:], b[32:] = a[:32], b[:32]
    elif case == 'one_pixel':
        ca, cb, wa, wb = scene.pixel_centre(scene.dims[0]//3, scene.dims[1]//2)
        a, b = ca + wa*rng.uniform(-0.3, 0.3, n), cb + wb*rng.uniform(-0.3, 0.3, n)
    elif case == 'alternating':                    # binned samples with w == 0 between the others
        frac[1::2] = 0.0
    elif case == 'gap':                            # a wave with nothing to bin between two with some
        inside = (np.arange(n)//64 != 1) & (rng.random(n) < 0.7)
    a = np.where(inside, a, 10.0)                  # far outside the frame / the field of view
    return dress(scene.place(a, b, depth), rng, frac=frac), int(inside.sum())


@both
@pytest.mark.parametrize('case', ['lower', 'upper', 'partners', 'one_pixel', 'alternating', 'gap'])
def test_wave_shapes(ctx, forces, which, case):
    scene = SCENES[which](forces)
    cols, n_inside = wave_case(scene, case, 300 + len(case))
    want = check(ctx, scene, cols, 'constant')
    assert want.binned == n_inside
    if case == 'one_pixel':
        assert np.count_nonzero(want.counts) == 1 and want.counts.max() == 64
    if case == 'partners':
        assert np.all(want.counts % 2 == 0)
    if case == 'alternating':
        assert want.binned == 64 and np.count_nonzero(want.image) <= 32


@both
@pytest.mark.parametrize('dims', [(1, 1), (5, 3), (64, 48), (257, 130)])
def test_image_dims(ctx, forces, which, dims):
    scene = SCENES[which](forces, dims=dims)
    want = check(ctx, scene, cloud(20011, 21), 'column')
    assert want.counts.shape == dims and want.binned > 500


@both
@pytest.mark.parametrize('kind', ['column', 'constant', 'two'])
def test_quantities(ctx, forces, which, kind):
    want = check(ctx, SCENES[which](forces), cloud(30011, 31), kind)
    dark = (want.counts > 0) & (want.image == 0)
    assert np.all(want.sums[dark] == 0)                     # samples with w == 0 add nothing
    assert np.count_nonzero(want.sums[..., 0]) > 100


@pytest.mark.parametrize('rotation', ['x_is_x', 'general'])
def test_image_rotations(ctx, forces, rotation):
    scene = ImageScene(forces, rotation=rotation)
    M = scene.M
    if rotation == 'x_is_x':
        assert M[0, 0] == 1.0 and not M[0, 1:].any() and not M[1:, 0].any() and M[1, 2] != 0
    else:
        assert np.all(np.abs(M) > 1e-3)
    check(ctx, scene, cloud(30011, 33), 'two')


@pytest.mark.parametrize('camera', sorted(CAMERAS))
def test_cameras(ctx, forces, camera):
    want = check(ctx, CameraScene(forces, camera=camera), cloud(30011, 35), 'two')
    assert 1000 < want.binned < want.samples


# ---- sources ---------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns(ctx, forces, which, dtype):
    check(ctx, SCENES[which](forces), cloud(40009, 41, dtype), 'two')


@pytest.fixture(scope='module', params=[True, False], ids=['narrow', 'wide'])
def store(request, ctx, forces):
    """Rows of integrate_const_rows in HBM (float32 / int32, or 64-bit) and their host copy."""
    endtime, step = 3000., 30.
    X0 = H.sample_x0(300, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, forces)
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    st = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=request.param, resident=True)['store']
    try:
        assert st.narrow == request.param and st.total > 10000
        rows, _ = st.download(index=False)
        assert rows.dtype == (np.float32 if request.param else np.float64)
        yield st, rows
    finally:
        st.free()


@both
@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, forces, store, which, part):
    """Rows in HBM, whole and as a slice with first > 0 that ends inside the store, against the same
    rows sent from the host and against the restatement."""
    st, rows = store
    first, count = (0, st.total) if part == 'whole' else (777, st.total - 777 - 999)
    scene = SCENES[which](forces)
    quantity, gt = tables(forces, 'two')
    cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (1, 2, 3, 4, 5, 6, 7))
    want = restate(scene, cols, quantity, gt)
    assert want.binned > 1000
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, *cols)
    host, host_counts, host_sums = compare(ctx, scene, want, ctx.counters())
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, rows=(st, first, count))
    got, got_counts, got_sums = compare(ctx, scene, want, ctx.counters())
    assert np.array_equal(got_counts, host_counts)
    np.testing.assert_allclose(got, host, rtol=ROWS_RTOL, atol=0)
    compare_sums(got_sums, want, rtol=ROWS_RTOL, reference=host_sums)


# ---- state -----------------------------------------------------------------------------------------
@both
def test_two_calls_sum_and_a_set_switches_the_moments_off(ctx, forces, which):
    scene = SCENES[which](forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    a, b = cloud(9001, 61), cloud(7001, 62)
    want_a = restate(scene, a, quantity, gt)
    want = restate(scene, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), quantity, gt)
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    scene.accumulate(ctx, *b)
    compare(ctx, scene, want)
    scene.accumulate(ctx, *(c[:0] for c in a))                   # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0 and ctx.counters()['samples_binned'] == 0
    compare(ctx, scene, want)
    scene.set(ctx, quantity, gt, enable=False)                    # a set zeroes and switches off
    image, counts = scene.pair(ctx)
    assert not image.any() and not counts.any()
    for call in (lambda: scene.moments(ctx), lambda: scene.accumulate(ctx, *a)):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'moments_enable' in str(err.value)
    scene.enable(ctx)
    assert not scene.moments(ctx).any()                           # the enable zeroes
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    scene.enable(ctx, False)                                      # off again: the entries refuse
    with pytest.raises(hip_api.HipError) as err:
        scene.moments(ctx)
    assert 'moments_enable' in str(err.value)
    image, counts = scene.pair(ctx)                               # the image pair is still there
    assert np.array_equal(counts, want_a.counts)


def test_image_clear_zeroes_the_moments_with_the_image(ctx, forces):
    scene = ImageScene(forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    cols = cloud(9001, 61)
    want = restate(scene, cols, quantity, gt)
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, *cols)
    assert scene.moments(ctx).any()
    ctx.image_clear()
    assert not scene.moments(ctx).any() and not scene.pair(ctx)[1].any()
    scene.accumulate(ctx, *cols)                                  # still enabled
    compare(ctx, scene, want, ctx.counters())


def test_before_the_set_the_set_is_named(forces):
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for accumulate, download, enable, name in (
                (fresh.image_moments_accumulate, fresh.image_moments_download,
                 fresh.image_moments_enable, 'nxc_set_image'),
                (fresh.camera_moments_accumulate, fresh.camera_moments_download,
                 fresh.camera_moments_enable, 'nxc_camera_set')):
            for call in (lambda: accumulate(x, x, x, x, x, x, x), download, enable):
                with pytest.raises(hip_api.HipError) as err:
                    call()
                assert err.value.code == hip_api.NXC_ERR_STATE and name in str(err.value)


@both
def test_bad_arguments(ctx, forces, which):
    scene = SCENES[which](forces, dims=(5, 3))
    scene.set(ctx, 'column', [])
    entry = getattr(ctx.lib, f'nxc_{which}_moments_accumulate')
    import ctypes as C
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), p, p, p, p, p, p, p) == hip_api.NXC_ERR_ARG
    for hole in range(7):
        args = [p]*7
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*7) == 0
    assert not scene.moments(ctx).any()


@both
def test_the_plain_accumulate_leaves_the_planes_zero(ctx, forces, which):
    scene = SCENES[which](forces)
    quantity, gt = tables(forces, 'two')
    cols = cloud(20011, 72)
    want = restate(scene, cols, quantity, gt)
    scene.set(ctx, quantity, gt)
    scene.plain(ctx, *cols)
    image, counts = scene.pair(ctx)
    assert np.array_equal(counts, want.counts) and want.binned > 1000
    assert not scene.moments(ctx).any()


def test_the_two_consumers_planes_never_touch(ctx, forces):
    image, cam = ImageScene(forces, dims=(40, 24)), CameraScene(forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    a, b = cloud(9001, 81), cloud(7001, 82)
    want_image, want_cam = restate(image, a, quantity, gt), restate(cam, b, quantity, gt)
    image.set(ctx, quantity, gt)
    cam.set(ctx, quantity, gt)
    image.accumulate(ctx, *a)
    assert not cam.moments(ctx).any() and not cam.pair(ctx)[1].any()
    cam.accumulate(ctx, *b)
    compare(ctx, image, want_image)
    compare(ctx, cam, want_cam)
    cam.set(ctx, quantity, gt)                                    # the camera's set: its own only
    assert not cam.moments(ctx).any()
    compare(ctx, image, want_image)
    image.set(ctx, quantity, gt, enable=False)                    # and the other way round
    cam.accumulate(ctx, *b)
    compare(ctx, cam, want_cam)
    assert not image.pair(ctx)[1].any()
    with pytest.raises(hip_api.HipError):
        image.moments(ctx)                                        # switched off by its set


@both
def test_moments_pass_against_the_plain_atomic_pass(ctx, forces, which):
    """Same samples, same counts and counters, images equal to the order of addition."""
    scene = SCENES[which](forces)
    quantity, gt = tables(forces, 'two')
    cols = cloud(200_003, 91, np.float32)
    ctx.image_mode('atomics')
    try:
        scene.set(ctx, quantity, gt, enable=False)
        scene.plain(ctx, *cols)
        plain_counters = ctx.counters()
        plain, plain_counts = scene.pair(ctx)
    finally:
        ctx.image_mode('auto')
    scene.set(ctx, quantity, gt)
    scene.accumulate(ctx, *cols)
    counters = ctx.counters()
    image, counts = scene.pair(ctx)
    assert plain_counts.sum() > 50_000
    assert np.array_equal(counts, plain_counts)
    assert all(counters[k] == plain_counters[k] for k in ('samples', 'samples_binned', 'nonfinite'))
    np.testing.assert_allclose(image, plain, rtol=RTOL, atol=0)


# ---- public API -----------------------------------------------------------------------------------
def test_public_classes_resident_restored_and_restatement(ctx, tmp_path):
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
    image_params = dict(quantity='radiance', dims='64,48', width='8,8', subobslongitude='0.7',
                        subobslatitude='0.4')
    camera_params = dict(quantity='radiance', observer='2.5,-5,1.5', up='0.1,0,1', fov='44,33',
                         dims='64,48')
    endtime = inputs.options.endtime.value
    for cls, params in ((ModelImage, image_params), (CameraImage, camera_params)):
        with contextlib.redirect_stdout(io.StringIO()):
            plain = cls(inputs, params, context=ctx)
            resident = cls(inputs, params, context=ctx, moments=True)
            host = cls(restored, params, context=ctx, moments=True)
            produced = inputs.produce_image(params, context=ctx, moments=True) \
                if cls is ModelImage else None
        assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
        assert not hasattr(plain, 'moment_sums') and not hasattr(plain, 'velocity')
        image, counts = np.zeros((64, 48)), np.zeros((64, 48))
        sums, mags = np.zeros((64, 48, 4)), np.zeros((64, 48, 4))
        totalsource = 0.
        for out in outs:
            X = Output.restore(out).X
            cols = tuple(X[c].values for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'))
            vr, gt = float(out.vrplanet)/resident.unit_km, resident.g_tables(float(out.aplanet))
            if cls is ModelImage:
                res = image_moments(*cols, vr, resident.image_rotation(), 'radiance', gt, (64, 48),
                                    (-4., 4.), (-4., 4.), float(resident.Apix))
            else:
                res = camera_moments(*cols, resident.observer, resident.basis, resident.uedges,
                                     resident.vedges, vr, resident.pix_area_cm2, 'radiance', gt)
            print(f'{cls.__name__} guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e}')
            assert res.edge_guard >= GUARD and res.margin_guard >= GUARD
            image += res.image
            counts += res.counts
            sums += res.sums
            mags += res.abs_sums
            totalsource += out.totalsource
        assert counts.sum() > 10000
        want = type(res)(counts, image, sums, mags, 0, 0, 0, 0)
        atoms_per_packet = 1e23/(totalsource/endtime)
        quotients = pixel_moments_from_sums(image, sums, resident.unit_km)
        # What the rule for the sums leaves of the quotients on a pixel with image sum S, with
        # e = 1e-11, A_k = sum |term| of sum k, q_k = m_k / S (got: m_k to e A_k, S to e |S|):
        #   u = q1:            du   = e (A1/S + |u|)                  + 2 roundings of |u|
        #   var = q2 - u^2:    dvar = e (A2/S + |q2|) + 2 |u| du      + 5 roundings of q2 + u^2
        #   sigma = sqrt(var): |sigma' - sigma| = |var' - var| / (sigma' + sigma) <= dvar / sigma
        # (a rounding = 1.2e-16; the factor 1.001 covers the terms of second order in e)
        with np.errstate(divide='ignore', invalid='ignore'):
            u, q2 = sums[..., 0]/image, sums[..., 1]/image
            du = 1.001*(RTOL*(mags[..., 0]/image + np.abs(u)) + 2.4e-16*np.abs(u))
            dvar = 1.001*(RTOL*(mags[..., 1]/image + np.abs(q2)) + 2*np.abs(u)*du
                          + 6e-16*(np.abs(q2) + u*u))
            sigma = np.sqrt(np.maximum(q2 - u*u, 0))
            dsigma = dvar/sigma + 2.4e-16*sigma
        solid = (quotients['effective_packets'] >= 2) & (sigma > 0)
        assert solid.sum() > 200
        for obj in filter(None, (resident, host, produced)):
            assert obj.moment_sums.shape == (64, 48, len(PIXEL_MOMENT_COLUMNS))
            assert np.array_equal(obj.packet_image, counts)
            assert np.array_equal(obj.packet_image, plain.packet_image)
            np.testing.assert_allclose(obj.image, image*atoms_per_packet, rtol=RTOL, atol=0)
            np.testing.assert_allclose(obj.image, plain.image, rtol=RTOL, atol=0)
            compare_sums(obj.moment_sums, want)
            if not (cls is ModelImage and obj is host):     # (create_image keeps the last Output's)
                assert obj.counters['samples_binned'] == counts.sum()
            k = resident.unit_km
            assert np.all(np.abs(obj.velocity - quotients['velocity'])[solid] <= (du*k)[solid])
            assert np.all(np.abs(obj.velocity_variance - quotients['velocity_variance'])[solid]
                          <= (dvar*k*k)[solid])
            assert np.all(np.abs(obj.velocity_dispersion - quotients['velocity_dispersion'])[solid]
                          <= (dsigma*k)[solid])
            empty = image == 0
            assert np.all(np.isnan(obj.velocity[empty])) and not obj.effective_packets[empty].any()
            np.testing.assert_allclose(obj.effective_packets[~empty],
                                       quotients['effective_packets'][~empty], rtol=4*RTOL)
