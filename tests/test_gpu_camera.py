"""k_camera and CameraImage on the GPU against tests/camera_restatement.py (the definition of
include/nexoclom_hip.h restated with NumPy).

Every comparison first asserts the restatement's two guards (>= 1e-9: no tangent-plane coordinate
that close to a bin edge, no decision that close to its threshold).  That is a condition on the
inputs, far above the few-ulp differences possible between the device and NumPy, and it is what
makes the exact comparison of packet counts legitimate.  Weighted pixels then agree to rtol 1e-11
(the project's figure for images summed in another order; the camera weight adds about ten
roundings), counts and counters exactly.  The thresholds themselves, which the guards keep
away from, are covered by tests/test_gpu_camera_thresholds.py on the inputs of
tests/threshold_cases.py."""
import contextlib
import io
import os

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import CameraImage, Input, Output, hip_api
from nexoclom_amd.CameraImage import camera_basis
from oracle import np_oracle as O
from tests import helpers as H
from tests.camera_restatement import camera_image

pytestmark = pytest.mark.gpu
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
GUARD = 1e-9
RTOL = 1e-11


class Camera:
    def __init__(self, o, boresight, up, fov, dims):
        self.o = np.array(o, dtype=float)
        bore = -self.o if boresight is None else np.array(boresight, dtype=float)
        self.basis = camera_basis(bore, up)
        half = [np.tan(np.radians(f)/2) for f in fov]
        self.uedges = np.linspace(-half[0], half[0], dims[0] + 1)
        self.vedges = np.linspace(-half[1], half[1], dims[1] + 1)
        self.area = (2*half[0]/dims[0])*(2*half[1]/dims[1])*(2440.53e5)**2

    def specials(self):
        """Samples placed on purpose, each far from every threshold: near the boresight, behind
        the camera, hidden on the far side of the planet, in the planet's shadow, far outside the
        field of view."""
        right, bore, up = self.basis
        unit = self.o/np.linalg.norm(self.o)
        return np.array([self.o + 3.0*(bore + 0.0137*right + 0.0071*up),
                         self.o - 2.0*(bore + 0.21*right),
                         -1.5*unit + 0.05*up + 0.03*right + 0.02*bore,
                         [0.31, 2.0, 0.17],
                         self.o + 2.0*(0.1*bore + right + 0.5*up)])


CAMERAS = {
    # outside the cloud, looking at the planet
    'outside': dict(o=(1.5, -6.0, 2.0), boresight=None, up=(0, 0, 1), fov=(40, 30)),
    # altitude 0.2 R, looking along the horizon: samples on both sides of the camera, a grazing limb
    'horizon': dict(o=(0.0, -1.2, 0.0), boresight=(1, 0, 0.05), up=(0, 0, 1), fov=(100, 80)),
    # on the night side
    'night': dict(o=(0.5, 4.0, 1.0), boresight=None, up=(0, 0, 1), fov=(60, 45)),
    # all nine entries of the basis non-zero, unequal angles
    'oblique': dict(o=(3.0, -4.0, 2.5), boresight=(-0.5, 0.8, -0.3), up=(0.2, 0.1, 1), fov=(50, 35)),
}


def camera(name, dims=(64, 48)):
    return Camera(dims=dims, **CAMERAS[name])


def cloud(cam, p, seed, dtype=np.float64):
    """p samples: the camera's special ones first, then a seeded cloud around the planet."""
    rng = np.random.default_rng(seed)
    n = max(p - 5, 0)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    xyz = np.concatenate([cam.specials(), d*rng.uniform(1.0, 6.0, n)[:, None]])[:p]
    vy = rng.uniform(-0.02, 0.02, len(xyz))
    frac = rng.uniform(1e-6, 1.0, len(xyz))
    return tuple(np.ascontiguousarray(c.astype(dtype)) for c in (xyz[:, 0], xyz[:, 1], xyz[:, 2], vy, frac))


@pytest.fixture(scope='module')
def forces():
    return H.mercury_forces('Na', 1.3)


def tables(forces, kind):
    if kind == 'column':
        return 'column', []
    if kind == 'constant':
        return 'radiance', [(np.array([-1e30, 1e30]), np.array([2.5, 2.5]))]
    lines = (5891,) if kind == 'one' else (5891, 5897)
    return 'radiance', H.g_tables('Na', forces.aplanet, forces.R_km, lines)


def set_camera(ctx, cam, forces, quantity, gt):
    ctx.camera_set(cam.o, cam.basis, forces.vrplanet, cam.area, quantity, cam.uedges, cam.vedges, gt)


def restate(cam, forces, cols, quantity, gt):
    res = camera_image(*cols, cam.o, cam.basis, cam.uedges, cam.vedges, forces.vrplanet, cam.area,
                       quantity, gt)
    print(f'guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e}; '
          f'{res.samples} samples, {res.binned} binned')
    assert res.edge_guard >= GUARD and res.margin_guard >= GUARD
    return res


def compare(ctx, want, counters=None):
    image, counts = ctx.camera_download()
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(image, want.image, rtol=RTOL, atol=0)
    if counters is not None:
        assert counters['samples'] == want.samples
        assert counters['samples_binned'] == want.binned == want.counts.sum()
        assert counters['nonfinite'] == 0
    return image, counts


def check(ctx, cam, forces, cols, kind):
    quantity, gt = tables(forces, kind)
    want = restate(cam, forces, cols, quantity, gt)
    set_camera(ctx, cam, forces, quantity, gt)
    ctx.camera_accumulate(*cols)
    compare(ctx, want, ctx.counters())
    return want


# ---- shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025, 70001])
def test_ragged_waves_and_blocks(ctx, forces, p):
    cam = camera('outside')
    want = check(ctx, cam, forces, cloud(cam, p, 100 + p), 'two')
    if p >= 5:
        # specials: near the boresight and on the far side binned, the latter and the shadowed one dark
        assert want.binned >= 2
    if p == 70001:
        assert want.binned > 20000 and np.count_nonzero(want.counts) > 2000


def test_second_trip_of_the_grid_stride_loop(ctx, forces):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    cam = camera('outside')
    p = 1_200_001
    want = check(ctx, cam, forces, cloud(cam, p, 7, np.float32), 'one')
    assert want.binned > 500_000


@pytest.mark.parametrize('dims', [(1, 1), (5, 3), (64, 48), (257, 130)])
def test_image_dims(ctx, forces, dims):
    cam = camera('oblique', dims)
    want = check(ctx, cam, forces, cloud(cam, 20011, 21), 'column')
    assert want.counts.shape == dims and want.binned > 500
    if dims != (1, 1):          # not symmetric under a transposition of the pixel index
        assert not np.array_equal(want.counts.ravel(), want.counts.T.ravel())


# ---- cameras x quantities --------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['column', 'constant', 'one', 'two'])
@pytest.mark.parametrize('name', sorted(CAMERAS))
def test_cameras_and_quantities(ctx, forces, name, kind):
    cam = camera(name)
    cols = cloud(cam, 30011, 31)
    want = check(ctx, cam, forces, cols, kind)
    assert want.binned > 1000 and want.binned < want.samples
    if name == 'horizon':
        x, y, z = cols[:3]
        side = (x - cam.o[0])*cam.basis[1][0] + (y - cam.o[1])*cam.basis[1][1] + (z - cam.o[2])*cam.basis[1][2]
        assert (side > 0).sum() > 5000 and (side < 0).sum() > 5000
    dark = (want.counts > 0) & (want.image == 0)
    lit = want.image > 0
    assert lit.sum() > 100
    if name != 'horizon':
        assert dark.any() or kind == 'column'


# ---- sources ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns(ctx, forces, dtype):
    cam = camera('night')
    check(ctx, cam, forces, cloud(cam, 40009, 41, dtype), 'two')


@pytest.mark.parametrize('narrow', [True, False])
def test_row_stores(ctx, forces, narrow):
    """Rows of integrate_const_rows in HBM (float32 / int32 or 64-bit), whole and as a slice with
    first > 0 that ends inside the store, against the same rows sent from the host and against
    the restatement."""
    endtime, step = 3000., 30.
    X0 = H.sample_x0(300, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, forces)
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    store = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=narrow, resident=True)['store']
    try:
        assert store.narrow == narrow and store.total > 10000
        rows, _ = store.download(index=False)
        assert rows.dtype == (np.float32 if narrow else np.float64)
        cam = camera('outside')
        quantity, gt = tables(forces, 'two')
        for first, count in ((0, store.total), (777, store.total - 777 - 999)):
            cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (1, 2, 3, 5, 7))
            want = restate(cam, forces, cols, quantity, gt)
            assert want.binned > 1000
            set_camera(ctx, cam, forces, quantity, gt)
            ctx.camera_accumulate(*cols)
            host, host_counts = compare(ctx, want, ctx.counters())
            set_camera(ctx, cam, forces, quantity, gt)
            ctx.camera_accumulate(rows=(store, first, count))
            got, got_counts = compare(ctx, want, ctx.counters())
            assert np.array_equal(got_counts, host_counts)
            np.testing.assert_allclose(got, host, rtol=1e-12, atol=0)
    finally:
        store.free()


# ---- state -----------------------------------------------------------------------------------------
def test_accumulate_sums_set_zeroes_and_the_model_image_is_separate(ctx, forces):
    cam = camera('oblique', (33, 20))
    quantity, gt = tables(forces, 'two')
    a, b = cloud(cam, 9001, 61), cloud(cam, 7001, 62)
    both = tuple(np.concatenate([u, v]) for u, v in zip(a, b))
    want_a = restate(cam, forces, a, quantity, gt)
    want = restate(cam, forces, both, quantity, gt)
    im = H.image_setup(forces, 'radiance', dims=(40, 24))

    def set_image():
        ctx.set_image(im['M'], forces.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                      im['g_tables'])

    set_image()                                   # before the camera exists ...
    set_camera(ctx, cam, forces, quantity, gt)
    ctx.camera_accumulate(*a)
    compare(ctx, want_a, ctx.counters())
    set_image()                                   # ... and between its accumulate calls
    ctx.image_accumulate(*b)
    model, model_counts = ctx.image_download()
    assert model_counts.sum() > 1000
    compare(ctx, want_a)                          # the camera image has not moved
    ctx.camera_accumulate(*b)
    compare(ctx, want)                            # two calls sum
    after, after_counts = ctx.image_download()    # and the ModelImage pair has not moved either
    assert np.array_equal(after, model) and np.array_equal(after_counts, model_counts)
    set_camera(ctx, cam, forces, quantity, gt)    # a set zeroes the camera image only
    image, counts = ctx.camera_download()
    assert not image.any() and not counts.any()
    after, after_counts = ctx.image_download()
    assert np.array_equal(after, model) and np.array_equal(after_counts, model_counts)


def test_accumulate_before_set_is_refused(forces):
    with hip_api.Context(0) as fresh:
        x = np.ones(4)
        with pytest.raises(hip_api.HipError) as err:
            fresh.camera_accumulate(x, x, x, x, x)
        assert 'nxc_camera_set' in str(err.value)
        with pytest.raises(hip_api.HipError):
            fresh.camera_download()
        cam = camera('outside')
        with pytest.raises(hip_api.HipError) as err:
            fresh.camera_set((0., 0.5, 0.), cam.basis, forces.vrplanet, cam.area, 'column',
                             cam.uedges, cam.vedges)
        assert '|o| >= 1' in str(err.value)


def test_nothing_in_the_field_of_view(ctx, forces):
    cam = Camera((0., -20., 0.), (0.1, -1., 0.), (0, 0, 1), (20, 20), (16, 12))   # looks away
    cols = cloud(camera('outside'), 5003, 71)
    want = check(ctx, cam, forces, cols, 'column')
    assert want.binned == 0
    image, counts = ctx.camera_download()
    assert not image.any() and not counts.any()


# ---- public API -----------------------------------------------------------------------------------
def test_camera_image_resident_restored_and_restatement(ctx, tmp_path):
    inputs = Input(INPUT, savepath=str(tmp_path))
    inputs.options.endtime = type(inputs.options.endtime)(3000., 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(2000, packs_per_it=1000, seed=81, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 2 and all(o.resident_rows(ctx) is not None for o in outs)
    params = dict(quantity='radiance', observer='2.5,-5,1.5', up='0.1,0,1', fov='44,33', dims='64,48')
    with contextlib.redirect_stdout(io.StringIO()):
        resident = CameraImage(inputs, params, context=ctx)
        restored = Input(INPUT)
        restored.options.endtime = inputs.options.endtime
        for k, f in enumerate(inputs.search()[1]):
            back = Output.restore(f)
            back.idnum = k + 1
            restored._catalogue.append(back)
        host = CameraImage(restored, params, context=ctx)
    assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
    image, counts = np.zeros((64, 48)), np.zeros((64, 48))
    totalsource = 0.
    for out in outs:
        X = Output.restore(out).X
        cols = tuple(X[c].values for c in ('x', 'y', 'z', 'vy', 'frac'))
        res = camera_image(*cols, resident.observer, resident.basis, resident.uedges,
                           resident.vedges, float(out.vrplanet)/resident.unit_km,
                           resident.pix_area_cm2, 'radiance', resident.g_tables(float(out.aplanet)))
        print(f'guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e}')
        assert res.edge_guard >= GUARD and res.margin_guard >= GUARD
        image += res.image
        counts += res.counts
        totalsource += out.totalsource
    assert counts.sum() > 10000
    atoms_per_packet = 1e23/(totalsource/inputs.options.endtime.value)
    for cam in (resident, host):
        assert np.array_equal(cam.packet_image, counts)
        np.testing.assert_allclose(cam.image, image*atoms_per_packet, rtol=RTOL, atol=0)
        assert cam.totalsource == totalsource and cam.atoms_per_packet == atoms_per_packet
        assert cam.counters['samples_binned'] == counts.sum() and cam.counters['nonfinite'] == 0
    assert np.array_equal(host.packet_image, resident.packet_image)
    np.testing.assert_allclose(host.image, resident.image, rtol=1e-12, atol=0)
    rays = resident.pixel_boresights()
    assert rays.shape == (64, 48, 3)
