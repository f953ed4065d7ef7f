"""k_image_cube / k_camera_cube and cube= of ModelImage / CameraImage on the GPU against
tests/pixel_cube_restatement.py (the "Velocity cube" definition of include/nexoclom_hip.h restated
with NumPy on top of the moments' restatement).  Scenes and sample generators are those of
tests/test_gpu_pixel_moments.py.

Comparison rule, everywhere: the restatement's three guards are asserted first (>= 1e-9: no binned
coordinate that close to a pixel edge, no decision that close to its threshold, no t that close to
an integer -- a condition on the inputs, which is what makes the exact comparison of counts and the
per-plane comparison legitimate); then counts and counters must be equal exactly, the image to rtol
1e-11, every cube entry to |got - want| <= 1e-11 * sum |term| per (pixel, plane, half), and on the
downloaded result the planes of a pixel must sum to its image at rtol 1e-11."""
import contextlib
import io

import numpy as np
import pytest

from nexoclom_amd import CameraImage, Input, ModelImage, Output, hip_api
from tests.pixel_cube_restatement import camera_cube, image_cube
from tests.test_gpu_pixel_moments import (CAMERAS, GUARD, INPUT, ROWS_RTOL, RTOL, CameraScene,  # noqa: F401
                                          ImageScene, cloud, forces, store, tables, wave_case)

pytestmark = pytest.mark.gpu
WIDE = (-0.05, 0.05)            # [R/s] holds every velocity dress() and cloud() give (|v| < 0.03)
NARROW = (0.001, 0.002)         # most samples fall outside


class CubeImage(ImageScene):
    """ModelImage's side: set_image / image_cube_* against image_cube."""

    def set(self, ctx, quantity, gt, cube=None):
        ctx.set_image(self.M, self.forces.vrplanet, self.im['apix'], quantity, self.im['xedges'],
                      self.im['zedges'], gt)
        if cube is not None:
            ctx.image_cube_enable(*cube)

    def restate(self, cols, quantity, gt, cube):
        return image_cube(*cols, self.forces.vrplanet, self.M, quantity, gt, self.dims,
                          self.im['xrange'], self.im['zrange'], self.im['apix'], *cube)

    def along(self, xyz, vlos):
        """Velocities whose line-of-sight component is vlos (to rounding; exactly 0 for 0)."""
        return vlos[:, None]*self.M[1][None, :]

    enable = staticmethod(lambda ctx, *cube: ctx.image_cube_enable(*cube))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.image_cube_accumulate(*a, **k))
    download = staticmethod(lambda ctx: ctx.image_cube_download())
    moments_enable = staticmethod(lambda ctx: ctx.image_moments_enable())
    moments_accumulate = staticmethod(lambda ctx, *a: ctx.image_moments_accumulate(*a))
    moments = staticmethod(lambda ctx: ctx.image_moments_download())


class CubeCamera(CameraScene):
    """CameraImage's side: camera_set / camera_cube_* against camera_cube."""

    def set(self, ctx, quantity, gt, cube=None):
        ctx.camera_set(self.o, self.basis, self.forces.vrplanet, self.area, quantity, self.uedges,
                       self.vedges, gt)
        if cube is not None:
            ctx.camera_cube_enable(*cube)

    def restate(self, cols, quantity, gt, cube):
        return camera_cube(*cols, self.o, self.basis, self.uedges, self.vedges,
                           self.forces.vrplanet, self.area, quantity, gt, *cube)

    def along(self, xyz, vlos):
        d = xyz - self.o
        return vlos[:, None]*d/np.linalg.norm(d, axis=1)[:, None]

    enable = staticmethod(lambda ctx, *cube: ctx.camera_cube_enable(*cube))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.camera_cube_accumulate(*a, **k))
    download = staticmethod(lambda ctx: ctx.camera_cube_download())
    moments_enable = staticmethod(lambda ctx: ctx.camera_moments_enable())
    moments_accumulate = staticmethod(lambda ctx, *a: ctx.camera_moments_accumulate(*a))
    moments = staticmethod(lambda ctx: ctx.camera_moments_download())


SCENES = {'image': CubeImage, 'camera': CubeCamera}
both = pytest.mark.parametrize('which', sorted(SCENES))


def restate(scene, cols, quantity, gt, cube, bin_guard=True):
    want = scene.restate(cols, quantity, gt, cube)
    print(f'{scene.name} guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e}; {want.samples} samples, {want.binned} binned')
    assert want.edge_guard >= GUARD and want.margin_guard >= GUARD
    assert want.bin_guard >= GUARD or not bin_guard
    return want


def compare_cube(got, want, rtol=RTOL, reference=None):
    """|got - want| <= rtol * sum |term| per (pixel, plane, half); the worst ratio is printed first."""
    reference = want.sums if reference is None else reference
    assert got.shape == want.sums.shape
    err = np.abs(got - reference)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(want.abs_sums > 0, err/want.abs_sums, np.where(err > 0, np.inf, 0.0))
    print('worst |got - want| / sum|term| (w, ww):',
          ratio.reshape(-1, 2).max(axis=0) if ratio.size else (0, 0))
    assert np.all(err <= rtol*want.abs_sums)


def compare(ctx, scene, want, counters=None):
    image, counts = scene.pair(ctx)
    assert np.array_equal(counts, want.counts)
    np.testing.assert_allclose(image, want.image, rtol=RTOL, atol=0)
    sums = scene.download(ctx)
    assert sums.shape == scene.dims + want.sums.shape[2:]
    compare_cube(sums, want)
    np.testing.assert_allclose(sums[..., 0].sum(-1), image, rtol=RTOL, atol=0)
    if counters is not None:
        assert counters['samples'] == want.samples
        assert counters['samples_binned'] == want.binned == want.counts.sum()
        assert counters['nonfinite'] == 0
    return image, counts, sums


def check(ctx, scene, cols, kind, cube, bin_guard=True):
    quantity, gt = tables(scene.forces, kind)
    want = restate(scene, cols, quantity, gt, cube, bin_guard)
    scene.set(ctx, quantity, gt, cube)
    scene.accumulate(ctx, *cols)
    compare(ctx, scene, want, ctx.counters())
    return want


# ---- 1. ragged waves and blocks ----------------------------------------------------------------------
@both
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, which, p):
    want = check(ctx, SCENES[which](forces), cloud(p, 100 + p), 'two', (7,) + WIDE)
    if p >= 1023:
        assert want.binned > 100 and np.count_nonzero(want.sums[..., 1:-1, 0]) > 50


@both
def test_second_trip_of_the_grid_stride_loop(ctx, forces, which):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    want = check(ctx, SCENES[which](forces), cloud(1_200_001, 9, np.float32), 'two', (33,) + WIDE)
    assert want.binned > 300_000 and np.count_nonzero(want.sums[..., 1:-1, 0].sum((0, 1))) > 10


# ---- 2. wave shapes ----------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('case', ['lower', 'upper', 'partners', 'one_pixel', 'alternating', 'gap'])
def test_wave_shapes(ctx, forces, which, case):
    scene = SCENES[which](forces)
    cols, n_inside = wave_case(scene, case, 300 + len(case))
    want = check(ctx, scene, cols, 'constant', (7,) + WIDE)
    assert want.binned == n_inside
    if case == 'one_pixel':
        assert np.count_nonzero(want.counts) == 1 and want.counts.max() == 64
    if case == 'alternating':
        assert want.binned == 64 and np.count_nonzero(want.sums[..., 1]) <= 32


def one_pixel(scene, rng, n=64):
    ca, cb, wa, wb = scene.pixel_centre(scene.dims[0]//3, scene.dims[1]//2)
    a, b = ca + wa*rng.uniform(-0.3, 0.3, n), cb + wb*rng.uniform(-0.3, 0.3, n)
    return scene.place(a, b, rng.uniform(0.0, 1.0, n))


def with_velocity(xyz, v, frac):
    cols = (xyz[:, 0], xyz[:, 1], xyz[:, 2], v[:, 0], v[:, 1], v[:, 2], frac)
    return tuple(np.ascontiguousarray(c, dtype=np.float64) for c in cols)


@both
def test_one_pixel_one_bin(ctx, forces, which):
    """64 samples in one record: lanes l and l + 32 add to the same 16 bytes, the highest
    contention add_record_pairs meets."""
    scene = SCENES[which](forces)
    rng = np.random.default_rng(411)
    xyz = one_pixel(scene, rng)
    cols = with_velocity(xyz, scene.along(xyz, rng.uniform(0.0101, 0.0139, 64)),
                         rng.uniform(0.1, 1.0, 64))
    want = check(ctx, scene, cols, 'constant', (7,) + WIDE)          # dv = 1/70: bin 4 is [0.0071, 0.0214)
    assert want.binned == 64 and np.count_nonzero(want.sums[..., 1]) == 1
    assert np.count_nonzero(want.sums[:, :, 5, 1]) == 1


@both
def test_one_pixel_every_plane(ctx, forces, which):
    """64 samples of one pixel over all nv + 2 planes of a cube over [0, 2^-7), nv = 8: eight at rest
    (vlos = v_lo exactly: every product has a zero factor, here and on the device, so t is a zero of
    either sign and the plane is 1), eight just below v_lo (vlos = -1e-7), eight far above v_hi,
    eight below it by a bin, and four in the middle of each bin.  The bin guard is a condition on
    inputs that rounding could move; the samples at rest cannot move, so it is asserted over the
    other 56, restated on their own."""
    scene = SCENES[which](forces)
    rng = np.random.default_rng(412)
    xyz = one_pixel(scene, rng)
    nv, v_hi = 8, 2.0**-7
    dv = v_hi/nv
    vlos = np.concatenate([np.zeros(8), np.full(8, -1e-7), np.full(8, 1.5*v_hi), np.full(8, -dv),
                           np.repeat((np.arange(nv) + 0.5)*dv, 4)])
    vlos[32:] += rng.uniform(-0.2, 0.2, 32)*dv
    order = rng.permutation(64)
    xyz, vlos = xyz[order], vlos[order]
    cols = with_velocity(xyz, scene.along(xyz, vlos), rng.uniform(0.1, 1.0, 64))
    cube = (nv, 0.0, v_hi)
    quantity, gt = tables(forces, 'constant')
    moving = vlos != 0
    restate(scene, tuple(c[moving] for c in cols), quantity, gt, cube)
    want = check(ctx, scene, cols, 'constant', cube, bin_guard=False)
    assert want.bin_guard == 0.0 and want.binned == 64
    assert np.count_nonzero(want.sums[..., 1]) == nv + 2
    ix, iz = np.argwhere(want.counts)[0]
    lit = want.sums[ix, iz, :, 1] > 0
    assert lit.all()


# ---- 3. the bin axis ---------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('nv', [1, 2, 7, 64])
def test_bin_axis(ctx, forces, which, nv):
    scene = SCENES[which](forces)
    cols = cloud(30011, 500 + nv)
    want = check(ctx, scene, cols, 'two', (nv,) + WIDE)
    assert not want.sums[:, :, [0, -1]].any() and want.binned > 1000
    assert not scene.download(ctx)[:, :, [0, -1]].any()               # nothing below, nothing above
    want = check(ctx, scene, cols, 'two', (nv,) + NARROW)
    inside = want.sums[..., 1:-1, 0].sum()
    assert 0 < inside < 0.2*want.image.sum()
    assert want.sums[:, :, 0, 0].sum() > inside and want.sums[:, :, -1, 0].sum() > inside


@pytest.mark.parametrize('which,rotation', [('image', 'x_is_x'), ('image', 'general'), ('camera', None)])
def test_a_velocity_that_is_not_a_number_lands_above(ctx, forces, which, rotation):
    """One sample with vx = NaN and w != 0: plane nv + 1 of its pixel, and a finite image (with
    x_is_x the product M[3] vx has a zero factor and is still not a number)."""
    scene = CubeImage(forces, rotation=rotation) if which == 'image' else CubeCamera(forces)
    nv = 7
    cube = (nv,) + WIDE
    cols = [c.copy() for c in cloud(5003, 61)]
    clean = scene.restate(cols, 'column', [], cube)
    for k in range(len(cols[0])):                           # the first sample that reaches a pixel
        one = scene.restate(tuple(c[k:k + 1] for c in cols), 'column', [], cube)
        if one.image.any():
            break
    cols[3][k] = np.nan
    want = check(ctx, scene, tuple(cols), 'column', cube)
    pixel = tuple(np.argwhere(one.counts)[0])
    assert want.sums[pixel][nv + 1, 0] == one.image[pixel] != 0
    assert np.count_nonzero(want.sums[:, :, nv + 1, 0]) == 1 and not clean.sums[:, :, nv + 1].any()
    assert np.array_equal(want.image, clean.image)
    image, _ = scene.pair(ctx)
    assert np.isfinite(image).all() and np.isfinite(scene.download(ctx)).all()


# ---- 4. inputs ---------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('kind', ['column', 'constant', 'two'])
def test_quantities(ctx, forces, which, kind):
    want = check(ctx, SCENES[which](forces), cloud(30011, 31), kind, (7,) + WIDE)
    dark = (want.counts > 0) & (want.image == 0)
    assert not want.sums[dark].any()                        # samples with w == 0 add nothing
    assert np.count_nonzero(want.sums[..., 0]) > 100


@pytest.mark.parametrize('rotation', ['x_is_x', 'general'])
def test_image_rotations(ctx, forces, rotation):
    check(ctx, CubeImage(forces, rotation=rotation), cloud(30011, 33), 'two', (16,) + WIDE)


@pytest.mark.parametrize('camera', sorted(CAMERAS))
def test_cameras(ctx, forces, camera):
    want = check(ctx, CubeCamera(forces, camera=camera), cloud(30011, 35), 'two', (16,) + WIDE)
    assert 1000 < want.binned < want.samples


@both
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns(ctx, forces, which, dtype):
    check(ctx, SCENES[which](forces), cloud(40009, 41, dtype), 'two', (7,) + WIDE)


@both
@pytest.mark.parametrize('dims', [(1, 1), (5, 3), (257, 130)])
def test_image_dims(ctx, forces, which, dims):
    scene = SCENES[which](forces, dims=dims)
    want = check(ctx, scene, cloud(20011, 21), 'column', (5,) + WIDE)
    assert want.counts.shape == dims and want.binned > 500


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
    speed = max(np.abs(cols[k]).max() for k in (3, 4, 5))
    cube = (9, -2.0*speed, 2.0*speed)
    want = restate(scene, cols, quantity, gt, cube)
    assert want.binned > 1000
    scene.set(ctx, quantity, gt, cube)
    scene.accumulate(ctx, *cols)
    host, host_counts, host_sums = compare(ctx, scene, want, ctx.counters())
    scene.set(ctx, quantity, gt, cube)
    scene.accumulate(ctx, rows=(st, first, count))
    got, got_counts, got_sums = compare(ctx, scene, want, ctx.counters())
    assert np.array_equal(got_counts, host_counts)
    np.testing.assert_allclose(got, host, rtol=ROWS_RTOL, atol=0)
    compare_cube(got_sums, want, rtol=ROWS_RTOL, reference=host_sums)


# ---- 5. state ----------------------------------------------------------------------------------------
@both
def test_two_calls_sum_and_a_set_switches_the_cube_off(ctx, forces, which):
    scene = SCENES[which](forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    cube = (7,) + WIDE
    a, b = cloud(9001, 61), cloud(7001, 62)
    want_a = restate(scene, a, quantity, gt, cube)
    want = restate(scene, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), quantity, gt, cube)
    scene.set(ctx, quantity, gt, cube)
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    scene.accumulate(ctx, *b)
    compare(ctx, scene, want)
    scene.accumulate(ctx, *(c[:0] for c in a))                   # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0 and ctx.counters()['samples_binned'] == 0
    compare(ctx, scene, want)
    scene.set(ctx, quantity, gt)                                  # a set zeroes and switches off
    image, counts = scene.pair(ctx)
    assert not image.any() and not counts.any()
    for call in (lambda: scene.download(ctx), lambda: scene.accumulate(ctx, *a)):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'cube_enable' in str(err.value)
    scene.enable(ctx, *cube)
    assert not scene.download(ctx).any()                          # the enable zeroes
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    # another nv: a new, zeroed cube of the new shape
    other = (12,) + NARROW
    scene.enable(ctx, *other)
    assert scene.download(ctx).shape == (33, 20, 14, 2) and not scene.download(ctx).any()
    scene.set(ctx, quantity, gt, other)
    scene.accumulate(ctx, *a)
    compare(ctx, scene, restate(scene, a, quantity, gt, other), ctx.counters())
    scene.enable(ctx, 0)                                          # off again: the entries refuse
    with pytest.raises(hip_api.HipError) as err:
        scene.download(ctx)
    assert 'cube_enable' in str(err.value)
    image, counts = scene.pair(ctx)                               # the image pair is still there
    assert np.array_equal(counts, want_a.counts)


def test_image_clear_zeroes_the_cube_with_the_image(ctx, forces):
    scene = CubeImage(forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    cube = (7,) + WIDE
    cols = cloud(9001, 61)
    want = restate(scene, cols, quantity, gt, cube)
    scene.set(ctx, quantity, gt, cube)
    scene.accumulate(ctx, *cols)
    assert scene.download(ctx).any()
    ctx.image_clear()
    assert not scene.download(ctx).any() and not scene.pair(ctx)[1].any()
    scene.accumulate(ctx, *cols)                                  # still enabled
    compare(ctx, scene, want, ctx.counters())


def test_before_the_set_the_set_is_named(forces):
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for accumulate, download, enable, name in (
                (fresh.image_cube_accumulate, fresh.image_cube_download, fresh.image_cube_enable,
                 'nxc_set_image'),
                (fresh.camera_cube_accumulate, fresh.camera_cube_download, fresh.camera_cube_enable,
                 'nxc_camera_set')):
            for call in (lambda: accumulate(x, x, x, x, x, x, x), download,
                         lambda: enable(4, -1.0, 1.0), lambda: enable(-1, 2.0, 1.0)):
                with pytest.raises(hip_api.HipError) as err:
                    call()
                assert err.value.code == hip_api.NXC_ERR_STATE and name in str(err.value)


@both
def test_bad_arguments(ctx, forces, which):
    """The enable's refusals leave the cube that is there alone; the accumulate's are the moments'."""
    import ctypes as C
    scene = SCENES[which](forces, dims=(5, 3))
    scene.set(ctx, 'column', [], (4,) + WIDE)
    cols = cloud(2001, 71)
    scene.accumulate(ctx, *cols)
    before = scene.download(ctx)
    assert before.any()
    for bad in ((-1, -1.0, 1.0), (4, 1.0, 1.0), (4, 1.0, -1.0), (4, np.nan, 1.0), (4, 0.0, np.inf),
                (2**31 // 15, -1.0, 1.0)):
        with pytest.raises(hip_api.HipError) as err:
            scene.enable(ctx, *bad)
        assert err.value.code == hip_api.NXC_ERR_ARG and 'velocity cube' in str(err.value)
    assert np.array_equal(scene.download(ctx), before)
    entry = getattr(ctx.lib, f'nxc_{which}_cube_accumulate')
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), p, p, p, p, p, p, p) == hip_api.NXC_ERR_ARG
    for hole in range(7):
        args = [p]*7
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*7) == 0
    assert np.array_equal(scene.download(ctx), before)


@both
def test_cube_and_moments_are_independent(ctx, forces, which):
    """The plain and the moments entries leave the cube zero; a cube pass leaves the moments zero."""
    scene = SCENES[which](forces)
    quantity, gt = tables(forces, 'two')
    cube = (7,) + WIDE
    cols = cloud(20011, 72)
    want = restate(scene, cols, quantity, gt, cube)
    scene.set(ctx, quantity, gt, cube)
    scene.moments_enable(ctx)
    scene.plain(ctx, *cols)
    scene.moments_accumulate(ctx, *cols)
    image, counts = scene.pair(ctx)
    assert np.array_equal(counts, 2*want.counts) and want.binned > 1000
    assert scene.moments(ctx).any() and not scene.download(ctx).any()
    scene.set(ctx, quantity, gt, cube)
    scene.moments_enable(ctx)
    scene.accumulate(ctx, *cols)
    compare(ctx, scene, want, ctx.counters())
    assert not scene.moments(ctx).any()


def test_the_two_consumers_cubes_never_touch(ctx, forces):
    image, cam = CubeImage(forces, dims=(40, 24)), CubeCamera(forces, dims=(33, 20))
    quantity, gt = tables(forces, 'two')
    cube_i, cube_c = (7,) + WIDE, (11,) + WIDE
    a, b = cloud(9001, 81), cloud(7001, 82)
    want_image, want_cam = restate(image, a, quantity, gt, cube_i), restate(cam, b, quantity, gt, cube_c)
    image.set(ctx, quantity, gt, cube_i)
    cam.set(ctx, quantity, gt, cube_c)
    image.accumulate(ctx, *a)
    assert not cam.download(ctx).any() and not cam.pair(ctx)[1].any()
    cam.accumulate(ctx, *b)
    compare(ctx, image, want_image)
    compare(ctx, cam, want_cam)
    cam.set(ctx, quantity, gt, cube_c)                            # the camera's set: its own only
    assert not cam.download(ctx).any()
    compare(ctx, image, want_image)
    image.set(ctx, quantity, gt)                                  # and the other way round
    cam.accumulate(ctx, *b)
    compare(ctx, cam, want_cam)
    assert not image.pair(ctx)[1].any()
    with pytest.raises(hip_api.HipError):
        image.download(ctx)                                       # switched off by its set


# ---- 6. against the plain pass -----------------------------------------------------------------------
@both
def test_cube_pass_against_the_plain_atomic_pass(ctx, forces, which):
    """Same samples, same counts and counters, images equal to the order of addition."""
    scene = SCENES[which](forces)
    quantity, gt = tables(forces, 'two')
    cols = cloud(200_003, 91, np.float32)
    ctx.image_mode('atomics')
    try:
        scene.set(ctx, quantity, gt)
        scene.plain(ctx, *cols)
        plain_counters = ctx.counters()
        plain, plain_counts = scene.pair(ctx)
    finally:
        ctx.image_mode('auto')
    scene.set(ctx, quantity, gt, (64,) + WIDE)
    scene.accumulate(ctx, *cols)
    counters = ctx.counters()
    image, counts = scene.pair(ctx)
    assert plain_counts.sum() > 50_000
    assert np.array_equal(counts, plain_counts)
    assert all(counters[k] == plain_counters[k] for k in ('samples', 'samples_binned', 'nonfinite'))
    np.testing.assert_allclose(image, plain, rtol=RTOL, atol=0)
    np.testing.assert_allclose(scene.download(ctx)[..., 0].sum(-1), plain, rtol=RTOL, atol=0)


# ---- 7. public classes -------------------------------------------------------------------------------
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
    cube_kms, nv = (-6.0, 6.0), 12
    for cls, params in ((ModelImage, image_params), (CameraImage, camera_params)):
        with contextlib.redirect_stdout(io.StringIO()):
            plain = cls(inputs, params, context=ctx)
            resident = cls(inputs, params, context=ctx, cube=cube_kms + (nv,))
            host = cls(restored, params, context=ctx, cube=cube_kms + (nv,))
            produced = inputs.produce_image(params, context=ctx, cube=cube_kms + (nv,)) \
                if cls is ModelImage else None
        assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
        assert not hasattr(plain, 'cube_sums') and plain.cube is None
        cube = (nv, cube_kms[0]/resident.unit_km, cube_kms[1]/resident.unit_km)
        image, counts = np.zeros((64, 48)), np.zeros((64, 48))
        sums, mags = np.zeros((64, 48, nv + 2, 2)), np.zeros((64, 48, nv + 2, 2))
        totalsource = 0.
        for out in outs:
            X = Output.restore(out).X
            cols = tuple(X[c].values for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'))
            vr, gt = float(out.vrplanet)/resident.unit_km, resident.g_tables(float(out.aplanet))
            if cls is ModelImage:
                res = image_cube(*cols, vr, resident.image_rotation(), 'radiance', gt, (64, 48),
                                 (-4., 4.), (-4., 4.), float(resident.Apix), *cube)
            else:
                res = camera_cube(*cols, resident.observer, resident.basis, resident.uedges,
                                  resident.vedges, vr, resident.pix_area_cm2, 'radiance', gt, *cube)
            print(f'{cls.__name__} guards: edge {res.edge_guard:.3e} margin {res.margin_guard:.3e} '
                  f'bin {res.bin_guard:.3e}')
            assert min(res.edge_guard, res.margin_guard, res.bin_guard) >= GUARD
            image += res.image
            counts += res.counts
            sums += res.sums
            mags += res.abs_sums
            totalsource += out.totalsource
        assert counts.sum() > 10000 and np.count_nonzero(sums[..., 1:-1, 0].sum((0, 1))) >= 4
        want = type(res)(counts, image, sums, mags, 0, 0, 0, 0, 0)
        atoms_per_packet = 1e23/(totalsource/endtime)
        for obj in filter(None, (resident, host, produced)):
            assert obj.cube_sums.shape == (64, 48, nv + 2, 2)
            assert np.array_equal(obj.packet_image, counts)
            assert np.array_equal(obj.packet_image, plain.packet_image)
            np.testing.assert_allclose(obj.image, image*atoms_per_packet, rtol=RTOL, atol=0)
            np.testing.assert_allclose(obj.image, plain.image, rtol=RTOL, atol=0)
            compare_cube(obj.cube_sums, want)
            assert obj.cube.shape == (64, 48, nv)
            assert obj.cube_below.shape == (64, 48) == obj.cube_above.shape
            assert np.array_equal(obj.cube, obj.cube_sums[..., 1:-1, 0]*obj.atoms_per_packet)
            np.testing.assert_allclose(obj.cube.sum(-1) + obj.cube_below + obj.cube_above, obj.image,
                                       rtol=RTOL, atol=0)
            np.testing.assert_allclose(obj.velocity_edges, np.linspace(-6.0, 6.0, nv + 1),
                                       rtol=0, atol=1e-14)
            np.testing.assert_allclose(obj.velocity_axis, np.arange(-5.5, 6.0, 1.0), rtol=0, atol=1e-14)
            S, ww = obj.cube_sums[..., 1:-1, 0], obj.cube_sums[..., 1:-1, 1]
            filled = ww != 0
            assert filled.sum() > 500 and not obj.cube_effective_packets[~filled].any()
            assert np.array_equal(obj.cube_effective_packets[filled], (S*S/np.where(filled, ww, 1))[filled])
            assert np.all(obj.cube_effective_packets[filled] >= 1 - 1e-12)
