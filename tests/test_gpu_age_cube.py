"""k_image_ages / k_camera_ages, k_ages_apply and ages= / transient() of ModelImage / CameraImage on
the GPU against tests/age_cube_restatement.py (the "Age cube" definition of include/nexoclom_hip.h
restated with NumPy).  Scenes are those of tests/test_gpu_pixel_moments.py.

Samples: quantity 'column', fractions that are multiples of 1/16, row times that are multiples of
30 s.  The image scene is set with a pixel area of 1 cm^2, so a weight IS its fraction: every sum
of w and of w w is exact in fp64 whatever the order of the atomics, and the image's comparisons
are ``np.array_equal``.  The camera divides each fraction by its footprint, so its weights are not
dyadic and its sums depend on the order of addition: a record of n terms summed in two orders
differs by at most 2 (n - 1) 2^-53 sum |term| (sequential summation, both sides), and the camera is
held to n 2^-52 sum |term| per record with n the record's own packet count.  Counts, counters and
which records are empty are exact for both.  The restatement's guards on pixel edges and occultation
margins are asserted (>= 1e-9) as in the cube's tests; the bin guard is not, where ages sit on
edges on purpose -- the planes then follow from integers, which the CPU tests check."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

from nexoclom_amd import CameraImage, Input, ModelImage, Output, hip_api
from tests.age_cube_restatement import apply_ordered, apply_plan, camera_ages, image_ages
from oracle import np_oracle as O
from tests import helpers as H
from tests.test_gpu_pixel_moments import (GUARD, INPUT, CameraScene, ImageScene, cloud,  # noqa: F401
                                          forces)

pytestmark = pytest.mark.gpu
T0 = 3000.0
EPS = 2.0**-52


class AgesImage(ImageScene):
    """ModelImage's side: set_image (a pixel of 1 cm^2) / image_ages_* against image_ages."""
    exact = True

    def __init__(self, forces, dims=(64, 48), rotation='general'):
        super().__init__(forces, dims, rotation)
        self.im = dict(self.im, apix=1.0)

    def set(self, ctx, ages=None):
        ctx.set_image(self.M, self.forces.vrplanet, self.im['apix'], 'column', self.im['xedges'],
                      self.im['zedges'], [])
        if ages is not None:
            ctx.image_ages_enable(*ages)

    def restate(self, cols, ages):
        return image_ages(*cols, self.forces.vrplanet, self.M, 'column', [], self.dims,
                          self.im['xrange'], self.im['zrange'], self.im['apix'], *ages)

    enable = staticmethod(lambda ctx, *ages: ctx.image_ages_enable(*ages))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.image_ages_accumulate(*a, **k))
    download = staticmethod(lambda ctx: ctx.image_ages_download())
    upload = staticmethod(lambda ctx, sums: ctx.image_ages_upload(sums))
    apply = staticmethod(lambda ctx, K: ctx.image_ages_apply(K))
    plain = staticmethod(lambda ctx, t, x, y, z, vy, frac: ctx.image_accumulate(x, y, z, vy, frac))


class AgesCamera(CameraScene):
    """CameraImage's side: camera_set / camera_ages_* against camera_ages."""
    exact = False

    def set(self, ctx, ages=None):
        ctx.camera_set(self.o, self.basis, self.forces.vrplanet, self.area, 'column', self.uedges,
                       self.vedges, [])
        if ages is not None:
            ctx.camera_ages_enable(*ages)

    def restate(self, cols, ages):
        return camera_ages(*cols, self.o, self.basis, self.uedges, self.vedges,
                           self.forces.vrplanet, self.area, 'column', [], *ages)

    enable = staticmethod(lambda ctx, *ages: ctx.camera_ages_enable(*ages))
    accumulate = staticmethod(lambda ctx, *a, **k: ctx.camera_ages_accumulate(*a, **k))
    download = staticmethod(lambda ctx: ctx.camera_ages_download())
    upload = staticmethod(lambda ctx, sums: ctx.camera_ages_upload(sums))
    apply = staticmethod(lambda ctx, K: ctx.camera_ages_apply(K))
    plain = staticmethod(lambda ctx, t, x, y, z, vy, frac: ctx.camera_accumulate(x, y, z, vy, frac))


SCENES = {'image': AgesImage, 'camera': AgesCamera}
both = pytest.mark.parametrize('which', sorted(SCENES))


def aged(p, seed, dtype=np.float64, xyz=None):
    """Six columns time x y z vy frac: cloud()'s positions and vy (or the positions ``xyz``), times
    that are multiples of 30 s in [0, T0] and fractions that are multiples of 1/16 in (0, 1]."""
    rng = np.random.default_rng(seed + 7000)
    x, y, z, _, vy, _, _ = cloud(p, seed, dtype)
    if xyz is not None:
        x, y, z = (np.ascontiguousarray(xyz[:, k].astype(dtype)) for k in range(3))
    time = (30.0*rng.integers(0, 101, p)).astype(dtype)
    frac = (rng.integers(1, 17, p)/16.0).astype(dtype)
    return time, x, y, z, vy, frac


def restate(scene, cols, ages):
    want = scene.restate(cols, ages)
    print(f'{scene.name} guards: edge {want.edge_guard:.3e} margin {want.margin_guard:.3e} '
          f'bin {want.bin_guard:.3e}; {want.samples} samples, {want.binned} binned')
    assert want.edge_guard >= GUARD and want.margin_guard >= GUARD
    return want


def same_sums(scene, got, want, reference=None):
    """The module's rule for a downloaded block against the restatement (or ``reference``)."""
    reference = want.sums if reference is None else reference
    assert got.shape == want.sums.shape
    assert np.array_equal(got != 0, want.packets[..., None]*np.ones(2) != 0)
    if scene.exact:
        assert np.array_equal(got, reference)
        return
    err = np.abs(got - reference)
    bound = want.packets[..., None]*EPS*want.abs_sums
    print('worst |got - want| / (n eps sum|term|):',
          float(np.max(err[bound > 0]/bound[bound > 0])) if (bound > 0).any() else 0.0)
    assert np.all(err <= bound)


def compare(ctx, scene, want, counters=None):
    image, counts = scene.pair(ctx)
    assert np.array_equal(counts, want.counts)
    sums = scene.download(ctx)
    assert sums.shape == scene.dims + want.sums.shape[2:]
    same_sums(scene, sums, want)
    if scene.exact:
        assert np.array_equal(image, want.image)
        assert np.array_equal(sums[..., 0].sum(-1), image)
    else:
        n = want.counts*EPS
        assert np.all(np.abs(image - want.image) <= n*want.image)
        assert np.all(np.abs(sums[..., 0].sum(-1) - image) <= 2*n*want.image)
    if counters is not None:
        assert counters['samples'] == want.samples
        assert counters['samples_binned'] == want.binned == want.counts.sum()
        assert counters['nonfinite'] == 0
    return image, counts, sums


def check(ctx, scene, cols, ages):
    want = restate(scene, cols, ages)
    scene.set(ctx, ages)
    scene.accumulate(ctx, *cols)
    compare(ctx, scene, want, ctx.counters())
    return want


WIDE = (7, T0, 0.0, 30.0*7*16)            # 7 bins of 480 s hold every age
NARROW = (7, T0, 600.0, 600.0 + 30.0*7*2)  # bins of 60 s; most ages fall outside


# ---- 1. ragged sample counts -------------------------------------------------------------------------
@both
@pytest.mark.parametrize('p', [0, 1, 63, 64, 65, 1023, 1025])
def test_ragged_waves_and_blocks(ctx, forces, which, p):
    want = check(ctx, SCENES[which](forces), aged(p, 100 + p), WIDE)
    if p >= 1023:
        assert want.binned > 100 and np.count_nonzero(want.sums[..., 1:-1, 0]) > 50


@both
def test_second_trip_of_the_grid_stride_loop(ctx, forces, which):
    """More samples than one full grid of workgroups holds, as float32 host columns."""
    want = check(ctx, SCENES[which](forces), aged(1_200_001, 9, np.float32), WIDE)
    assert want.binned > 300_000 and np.count_nonzero(want.sums[..., 1:-1, 0].sum((0, 1))) == 7


# ---- 2. the age axis ---------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('na,m', [(1, 7), (2, 5), (7, 2), (64, 0), (64, 1)])
def test_age_axis_with_ages_on_the_edges(ctx, forces, which, na, m):
    """a_hi - a_lo = 30 na 2^m with a_lo = 300: every age is a_lo plus a multiple of 30 s, so it
    sits on an edge of the m = 0 axis."""
    scene = SCENES[which](forces)
    ages = (na, T0, 300.0, 300.0 + 30.0*na*2**m)
    cols = aged(10007, 500 + na + m)
    want = check(ctx, scene, cols, ages)
    assert want.bin_guard == 0.0 and want.binned > 500
    assert want.sums[:, :, 0, 0].sum() > 0                          # ages 0 .. 270 s
    assert np.count_nonzero(want.sums[..., 1:-1, 0].sum((0, 1))) == na or na == 64
    if ages[3] <= T0:
        assert want.sums[:, :, -1, 0].sum() > 0


def one_pixel(scene, rng, n):
    ca, cb, wa, wb = scene.pixel_centre(scene.dims[0]//3, scene.dims[1]//2)
    a, b = ca + wa*rng.uniform(-0.3, 0.3, n), cb + wb*rng.uniform(-0.3, 0.3, n)
    return scene.place(a, b, rng.uniform(0.0, 1.0, n))


@both
def test_one_pixel_every_plane(ctx, forces, which):
    """96 samples of one pixel over all na + 2 planes of an axis of 8 bins of 30 s from 60 s: ages
    0 and 30 s below it, every edge 60 .. 300 s (the last one is a_hi: the top plane), 330 s and
    T0 above, and half-way into every bin."""
    scene = SCENES[which](forces)
    rng = np.random.default_rng(412)
    age = np.concatenate([np.tile(np.arange(0.0, 360.0, 30.0), 6), np.full(8, T0),
                          np.tile(75.0 + 30.0*np.arange(8), 2)])
    assert len(age) == 96
    cols = list(aged(96, 5, xyz=one_pixel(scene, rng, 96)))
    cols[0] = T0 - rng.permutation(age)
    ages = (8, T0, 60.0, 300.0)
    want = check(ctx, scene, tuple(cols), ages)
    assert want.binned == 96 and np.count_nonzero(want.counts) == 1
    ix, iz = np.argwhere(want.counts)[0]
    assert list(want.packets[ix, iz]) == [12, 8, 8, 8, 8, 8, 8, 8, 8, 20]


@both
def test_a_time_that_is_not_a_number_lands_in_the_top_plane(ctx, forces, which):
    scene = SCENES[which](forces)
    cols = [c.copy() for c in aged(5003, 61)]
    clean = scene.restate(tuple(cols), WIDE)
    assert not clean.sums[:, :, -1].any()
    k = next(k for k in range(5003) if scene.restate(tuple(c[k:k + 1] for c in cols), WIDE).binned)
    cols[0][k] = np.nan
    want = check(ctx, scene, tuple(cols), WIDE)
    assert np.count_nonzero(want.sums[:, :, -1, 0]) == 1 and want.packets[:, :, -1].sum() == 1
    assert np.array_equal(want.image, clean.image)
    assert np.isfinite(scene.download(ctx)).all() and np.isfinite(scene.pair(ctx)[0]).all()


@both
def test_a_sample_without_weight_adds_nothing_and_is_counted(ctx, forces, which):
    """frac = 0 on every second sample, and a NaN time on them: the time of a sample with w == 0 is
    not read, so nothing reaches the top plane."""
    scene = SCENES[which](forces)
    cols = [c.copy() for c in aged(9001, 62)]
    cols[5][1::2] = 0.0
    cols[0][1::2] = np.nan
    want = check(ctx, scene, tuple(cols), WIDE)
    lit = restate(scene, tuple(c[0::2] for c in cols), WIDE)
    assert want.counts.sum() > lit.counts.sum() > 500
    assert np.array_equal(want.packets, lit.packets) and not want.sums[:, :, -1].any()
    assert 500 < want.packets.sum() <= lit.counts.sum()


# ---- 3. input paths ----------------------------------------------------------------------------------
@both
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_columns(ctx, forces, which, dtype):
    check(ctx, SCENES[which](forces), aged(10007, 41, dtype), NARROW)


@both
@pytest.mark.parametrize('dims', [(1, 1), (5, 3), (257, 130)])
def test_image_dims(ctx, forces, which, dims):
    want = check(ctx, SCENES[which](forces, dims=dims), aged(10007, 21), WIDE)
    assert want.counts.shape == dims and want.binned > 300


@pytest.fixture(scope='module', params=[True, False], ids=['narrow', 'wide'])
def lossless_store(request, ctx, forces):
    """Rows of integrate_const_rows in HBM (float32 / int32, or 64-bit) and their host copy, from a
    run without a loss process (no lifetime, no photoionisation): every row keeps frac = 1.0
    exactly, so the weights of the image scene (a pixel of 1 cm^2) are dyadic like aged()'s and the
    store's paths can be held to the bit."""
    endtime, step = T0, 30.
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


@both
@pytest.mark.parametrize('part', ['whole', 'slice'])
def test_row_stores(ctx, forces, lossless_store, which, part):
    """Rows in HBM (narrow and wide stores), whole and as a slice with first > 0 that ends inside
    the store, against the same rows sent from the host in their own width and widened, and against
    the restatement.  Every frac is 1.0, so for the image scene every path gives the same bits:
    ``np.array_equal`` of the blocks, the image pairs and the counts.  The camera's weights are
    fractions of its footprints, not dyadic: its paths are held to the module's bound for it."""
    st, rows = lossless_store
    first, count = (0, st.total) if part == 'whole' else (777, st.total - 777 - 999)
    scene = SCENES[which](forces)
    cols = tuple(np.ascontiguousarray(rows[c, first:first + count]) for c in (0, 1, 2, 3, 5, 7))
    ages = (50, T0, -15.0, 1485.0)                  # the step is 30 s: no age on an edge
    want = restate(scene, cols, ages)
    assert want.binned > 1000 and want.bin_guard >= GUARD
    assert want.sums[:, :, -1, 0].sum() > 0 and np.count_nonzero(want.sums[..., 1:-1, 0].sum((0, 1))) > 40
    got = {}
    for path in ('rows', 'host', 'host widened'):
        scene.set(ctx, ages)
        if path == 'rows':
            scene.accumulate(ctx, rows=(st, first, count))
        else:
            scene.accumulate(ctx, *(c.astype(np.float64) if path == 'host widened' else c
                                    for c in cols))
        got[path] = compare(ctx, scene, want, ctx.counters())
    for path in ('host', 'host widened'):
        assert np.array_equal(got[path][1], got['rows'][1])
        same_sums(scene, got[path][2], want, reference=got['rows'][2])
        if scene.exact:
            assert np.array_equal(got[path][0], got['rows'][0])


def test_a_slice_of_a_store_is_the_rows_it_names(ctx, forces, lossless_store):
    """Two adjacent slices of the store, one call each, sum to the whole store's block bit for bit
    (image scene), and each alone differs from it."""
    st, rows = lossless_store
    scene = AgesImage(forces)
    ages = (50, T0, -15.0, 1485.0)
    cut = st.total//3 + 1
    scene.set(ctx, ages)
    scene.accumulate(ctx, rows=(st, 0, st.total))
    whole = scene.download(ctx)
    scene.set(ctx, ages)
    scene.accumulate(ctx, rows=(st, 0, cut))
    part = scene.download(ctx)
    scene.accumulate(ctx, rows=(st, cut, st.total - cut))
    assert np.array_equal(scene.download(ctx), whole) and not np.array_equal(part, whole)
    assert part.any() and np.array_equal(whole[..., 0], whole[..., 1])       # every weight is 1.0


# ---- 4. state ----------------------------------------------------------------------------------------
@both
def test_two_calls_sum_and_a_set_switches_the_block_off(ctx, forces, which):
    scene = SCENES[which](forces, dims=(33, 20))
    a, b = aged(9001, 61), aged(7001, 62)
    want_a = restate(scene, a, WIDE)
    want = restate(scene, tuple(np.concatenate([u, v]) for u, v in zip(a, b)), WIDE)
    scene.set(ctx, WIDE)
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    scene.accumulate(ctx, *b)
    compare(ctx, scene, want)
    scene.accumulate(ctx, *(c[:0] for c in a))                   # p = 0: nothing but the counters
    assert ctx.counters()['samples'] == 0 and ctx.counters()['samples_binned'] == 0
    compare(ctx, scene, want)
    scene.set(ctx)                                                # a set zeroes and switches off
    image, counts = scene.pair(ctx)
    assert not image.any() and not counts.any()
    for call in (lambda: scene.download(ctx), lambda: scene.accumulate(ctx, *a),
                 lambda: scene.apply(ctx, np.ones((9, 1))), lambda: scene.upload(ctx, want.sums)):
        with pytest.raises(hip_api.HipError) as err:
            call()
        assert err.value.code == hip_api.NXC_ERR_STATE and 'ages_enable' in str(err.value)
    scene.enable(ctx, *WIDE)
    assert not scene.download(ctx).any()                          # the enable zeroes
    scene.accumulate(ctx, *a)
    compare(ctx, scene, want_a, ctx.counters())
    other = (12,) + NARROW[1:]                                    # another na: a new, zeroed block
    scene.enable(ctx, *other)
    assert scene.download(ctx).shape == (33, 20, 14, 2) and not scene.download(ctx).any()
    scene.enable(ctx, 0)                                          # off again: the entries refuse
    with pytest.raises(hip_api.HipError) as err:
        scene.download(ctx)
    assert 'ages_enable' in str(err.value)
    assert np.array_equal(scene.pair(ctx)[1], want_a.counts)      # the image pair is still there


def test_image_clear_zeroes_the_block_with_the_image(ctx, forces):
    scene = AgesImage(forces, dims=(33, 20))
    cols = aged(9001, 61)
    want = restate(scene, cols, WIDE)
    scene.set(ctx, WIDE)
    scene.accumulate(ctx, *cols)
    assert scene.download(ctx).any()
    ctx.image_clear()
    assert not scene.download(ctx).any() and not scene.pair(ctx)[1].any()
    scene.accumulate(ctx, *cols)                                  # still enabled
    compare(ctx, scene, want, ctx.counters())


def test_before_the_set_the_set_is_named(forces):
    x = np.ones(4)
    with hip_api.Context(0) as fresh:
        for prefix, name in (('image', 'nxc_set_image'), ('camera', 'nxc_camera_set')):
            get = lambda what: getattr(fresh, f'{prefix}_ages_{what}')          # noqa: E731
            for call in (lambda: get('accumulate')(x, x, x, x, x, x), get('download'),
                         lambda: get('enable')(4, 0.0, 0.0, 1.0),
                         lambda: get('enable')(-1, 0.0, 2.0, 1.0),
                         lambda: get('apply')(np.ones((2, 1))),
                         lambda: get('upload')(np.zeros((0, 0, 2, 2)))):
                with pytest.raises(hip_api.HipError) as err:
                    call()
                assert err.value.code == hip_api.NXC_ERR_STATE and name in str(err.value)


@both
def test_bad_arguments_leave_the_block_as_it_was(ctx, forces, which):
    scene = SCENES[which](forces, dims=(5, 3))
    scene.set(ctx, (4, T0, 0.0, 3840.0))
    cols = aged(2001, 71)
    scene.accumulate(ctx, *cols)
    before = scene.download(ctx)
    assert before.any()
    for bad in ((-1, T0, 0.0, 1.0), (4, T0, 1.0, 1.0), (4, T0, 1.0, -1.0), (4, T0, np.nan, 1.0),
                (4, T0, 0.0, np.inf), (4, np.nan, 0.0, 1.0), (4, np.inf, 0.0, 1.0),
                (4, T0, -1.7e308, 1.7e308), (2**31 // 15, T0, 0.0, 1.0)):
        with pytest.raises(hip_api.HipError) as err:
            scene.enable(ctx, *bad)
        assert err.value.code == hip_api.NXC_ERR_ARG and 'age cube' in str(err.value)
    assert np.array_equal(scene.download(ctx), before)
    entry = getattr(ctx.lib, f'nxc_{which}_ages_accumulate')
    x = np.ones(4)
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    assert entry(ctx._h, C.c_int64(-1), p, p, p, p, p, p) == hip_api.NXC_ERR_ARG
    for hole in range(6):
        args = [p]*6
        args[hole] = None
        assert entry(ctx._h, C.c_int64(4), *args) == hip_api.NXC_ERR_ARG
    assert entry(ctx._h, C.c_int64(0), *[None]*6) == 0
    # the apply's: ne < 1, a K that is not finite, null pointers
    apply_ = getattr(ctx.lib, f'nxc_{which}_ages_apply')
    K = np.ones((6, 2))
    out = np.zeros((2, 5, 3, 2))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                     # noqa: E731
    assert apply_(ctx._h, 0, dp(K), dp(out)) == hip_api.NXC_ERR_ARG
    assert apply_(ctx._h, -3, dp(K), dp(out)) == hip_api.NXC_ERR_ARG
    assert apply_(ctx._h, 2, None, dp(out)) == hip_api.NXC_ERR_ARG
    assert apply_(ctx._h, 2, dp(K), None) == hip_api.NXC_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (5, 1), (3, 0)):
            Kb = K.copy()
            Kb[at] = bad
            with pytest.raises(hip_api.HipError) as err:
                scene.apply(ctx, Kb)
            assert err.value.code == hip_api.NXC_ERR_ARG and 'not finite' in str(err.value)
    assert not out.any() and np.array_equal(scene.download(ctx), before)
    assert apply_(ctx._h, 2, dp(K), dp(out)) == 0 and out.any()


@both
def test_ages_cube_and_moments_are_independent(ctx, forces, which):
    """All three enabled; each pass fills its own block only, and each block equals its own
    single-pass result."""
    scene = SCENES[which](forces)
    t, x, y, z, vy, frac = cols = aged(10007, 72)
    vx, vz = cloud(10007, 72)[3], cloud(10007, 72)[5]
    seven = (x, y, z, vx, vy, vz, frac)
    cube = (7, -0.05, 0.05)
    ctxm = lambda what: getattr(ctx, f'{which}_{what}')                        # noqa: E731
    singles = {}
    for name in ('ages', 'cube', 'moments'):
        scene.set(ctx, WIDE if name == 'ages' else None)
        if name == 'cube':
            ctxm('cube_enable')(*cube)
        if name == 'moments':
            ctxm('moments_enable')()
        ctxm(name + '_accumulate')(*(cols if name == 'ages' else seven))
        singles[name] = ctxm(name + '_download')()
        assert singles[name].any()
    want = restate(scene, cols, WIDE)
    scene.set(ctx, WIDE)
    ctxm('cube_enable')(*cube)
    ctxm('moments_enable')()
    scene.plain(ctx, *cols)
    assert not any(ctxm(name + '_download')().any() for name in singles)
    for k, name in enumerate(singles):
        ctxm(name + '_accumulate')(*(cols if name == 'ages' else seven))
        for other in list(singles)[k + 1:]:
            assert not ctxm(other + '_download')().any()
    assert np.array_equal(scene.pair(ctx)[1], 4*want.counts)
    same_sums(scene, ctxm('ages_download')(), want, reference=singles['ages'])
    for name in ('cube', 'moments'):
        got = ctxm(name + '_download')()
        if scene.exact and name == 'cube':
            assert np.array_equal(got, singles[name])
        np.testing.assert_allclose(got, singles[name], rtol=1e-11, atol=1e-11*np.abs(singles[name]).max())
    ctxm('cube_enable')(0)                                        # freeing one leaves the others
    ctxm('moments_enable')(False)
    same_sums(scene, ctxm('ages_download')(), want, reference=singles['ages'])
    ctxm('cube_enable')(*cube)
    scene.enable(ctx, 0)
    assert not ctxm('cube_download')().any()
    with pytest.raises(hip_api.HipError):
        scene.download(ctx)


def test_the_two_consumers_blocks_never_touch(ctx, forces):
    image, cam = AgesImage(forces, dims=(40, 24)), AgesCamera(forces, dims=(33, 20))
    ages_i, ages_c = WIDE, (11,) + NARROW[1:]
    a, b = aged(9001, 81), aged(7001, 82)
    want_image, want_cam = restate(image, a, ages_i), restate(cam, b, ages_c)
    image.set(ctx, ages_i)
    cam.set(ctx, ages_c)
    image.accumulate(ctx, *a)
    assert not cam.download(ctx).any() and not cam.pair(ctx)[1].any()
    cam.accumulate(ctx, *b)
    compare(ctx, image, want_image)
    compare(ctx, cam, want_cam)
    cam.set(ctx, ages_c)                                          # the camera's set: its own only
    assert not cam.download(ctx).any()
    compare(ctx, image, want_image)
    image.set(ctx)                                                # and the other way round
    cam.accumulate(ctx, *b)
    compare(ctx, cam, want_cam)
    assert not image.pair(ctx)[1].any()
    with pytest.raises(hip_api.HipError):
        image.download(ctx)                                       # switched off by its set


# ---- 5. against the plain pass -----------------------------------------------------------------------
@both
def test_ages_pass_against_the_plain_atomic_pass(ctx, forces, which):
    """Same samples: the same counts and counters; the image pair identical where the sums are
    exact (the image scene), and to the order of addition for the camera."""
    scene = SCENES[which](forces)
    cols = aged(10007, 91, np.float32)
    ctx.image_mode('atomics')
    try:
        scene.set(ctx)
        scene.plain(ctx, *cols)
        plain_counters = ctx.counters()
        plain, plain_counts = scene.pair(ctx)
    finally:
        ctx.image_mode('auto')
    scene.set(ctx, (64, T0, 0.0, 30.0*64*2))
    scene.accumulate(ctx, *cols)
    counters = ctx.counters()
    image, counts = scene.pair(ctx)
    assert plain_counts.sum() > 2000
    assert np.array_equal(counts, plain_counts)
    assert all(counters[k] == plain_counters[k] for k in ('samples', 'samples_binned', 'nonfinite'))
    if scene.exact:
        assert np.array_equal(image, plain)
    else:
        assert np.all(np.abs(image - plain) <= counts*EPS*plain)


# ---- 6. the contraction ------------------------------------------------------------------------------
def block_and_kernel(rng, dims, na, ne, kind):
    sums = np.stack([rng.normal(size=dims + (na + 2,)), rng.uniform(0, 2, dims + (na + 2,))], -1)
    K = rng.uniform(0, 3, (na + 2, ne))
    if kind == 'zeros':
        K[rng.random(K.shape) < 0.4] = 0.0
        sums[rng.random(sums.shape[:-1]) < 0.3] = 0.0
    elif kind == 'zero row':                        # a row of zeros against an empty plane
        K[na // 2 + 1] = 0.0
        sums[..., na // 2 + 1, :] = 0.0
        K[0] = 0.0
    elif kind == 'negative':
        K = rng.normal(size=K.shape)*1e3
    return sums, K


def check_apply(ctx, scene, sums, K):
    scene.upload(ctx, sums)
    assert np.array_equal(scene.download(ctx), sums)
    got = scene.apply(ctx, K)
    want = apply_ordered(sums, K)
    assert got.shape == want.shape == (K.shape[1],) + scene.dims + (2,)
    assert np.array_equal(got, want)
    dense = np.stack([np.einsum('...k,ke->e...', sums[..., 0], K),
                      np.einsum('...k,ke->e...', sums[..., 1], K*K)], -1)
    mags = np.stack([np.einsum('...k,ke->e...', np.abs(sums[..., 0]), np.abs(K)),
                     np.einsum('...k,ke->e...', sums[..., 1], K*K)], -1)
    assert np.all(np.abs(got - dense) <= 1e-13*mags)
    assert np.array_equal(scene.download(ctx), sums)              # the block is only read


PLANS = sorted({apply_plan(planes, ne, lds)[1] for planes in (9, 66) for ne in (1, 3)
                for lds in (64*1024, 160*1024)})


@both
@pytest.mark.parametrize('ne', [1, 3, 65, 130])
@pytest.mark.parametrize('na', [7, 64])
def test_apply_epochs(ctx, forces, which, na, ne):
    """ne = 65 and 130 take two or more epoch chunks (at most 64 epochs a chunk; 30 with 66 planes
    in 32 KiB), the last one ragged."""
    rng = np.random.default_rng(na*1000 + ne)
    scene = SCENES[which](forces, dims=(33, 5))
    assert apply_plan(na + 2, ne, 64*1024)[2] < ne or ne <= 3
    scene.set(ctx, (na, T0, 0.0, 1.0))
    for kind in ('plain', 'zeros', 'zero row', 'negative'):
        check_apply(ctx, scene, *block_and_kernel(rng, scene.dims, na, ne, kind))


@pytest.mark.parametrize('npix', sorted({1, 5} | {r + d for r in PLANS for d in (-1, 0, 1)}))
@pytest.mark.parametrize('na', [7, 64])
def test_apply_pixel_runs(ctx, forces, na, npix):
    """Pixel counts around every pixel run the plan can choose for these shapes (the device's LDS
    is 64 KiB or 160 KiB a workgroup): one below, at and one above."""
    rng = np.random.default_rng(na*1000 + npix)
    scene = AgesImage(forces, dims=(npix, 1))
    scene.set(ctx, (na, T0, 0.0, 1.0))
    for ne in (1, 3):
        check_apply(ctx, scene, *block_and_kernel(rng, scene.dims, na, ne, 'negative'))


@both
def test_apply_on_the_largest_image(ctx, forces, which):
    rng = np.random.default_rng(5)
    scene = SCENES[which](forces, dims=(257, 130))
    scene.set(ctx, (7, T0, 0.0, 1.0))
    check_apply(ctx, scene, *block_and_kernel(rng, scene.dims, 7, 3, 'zeros'))


@both
def test_apply_of_a_binned_block_and_a_matrix_of_ones_is_the_image(ctx, forces, which):
    scene = SCENES[which](forces)
    cols = aged(10007, 33)
    want = check(ctx, scene, cols, WIDE)
    got = scene.apply(ctx, np.ones((9, 2)))
    sums = scene.download(ctx)
    assert np.array_equal(got, apply_ordered(sums, np.ones((9, 2))))
    image, _ = scene.pair(ctx)
    if scene.exact:
        assert np.array_equal(got[0, ..., 0], image) and np.array_equal(got[1, ..., 0], want.image)
    else:
        assert np.all(np.abs(got[0, ..., 0] - image) <= 2*want.counts*EPS*image)


# ---- 7. public classes -------------------------------------------------------------------------------
def quiet(make, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return make(*args, **kw)


@pytest.fixture(scope='module')
def small_run(ctx, tmp_path_factory):
    """400 packets in two Outputs over 3000 s in steps of 30 s, resident and restored from .npz."""
    inputs = Input(INPUT, savepath=str(tmp_path_factory.mktemp('ages_run')))
    inputs.options.endtime = type(inputs.options.endtime)(T0, 's')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(400, packs_per_it=200, seed=81, context=ctx)
        inputs.wait()
    outs = inputs._catalogue
    assert len(outs) == 2 and all(o.resident_rows(ctx) is not None for o in outs)
    restored = Input(INPUT)
    restored.options.endtime = inputs.options.endtime
    for k, f in enumerate(inputs.search()[1]):
        back = Output.restore(f)
        back.idnum = k + 1
        restored._catalogue.append(back)
    return inputs, restored


IMAGE_PARAMS = dict(quantity='radiance', dims='24,16', width='8,8', subobslongitude='0.7',
                    subobslatitude='0.4')
CAMERA_PARAMS = dict(quantity='radiance', observer='2.5,-5,1.5', up='0.1,0,1', fov='44,33',
                     dims='24,16')
AGES = (-15.0, 2985.0, 100)                 # bins of one step of 30 s, centred on the rows' ages


def restated(cls, obj, outs, keep=None):
    """The restatement over the restored rows of ``outs`` (those with ``keep(age)``), summed."""
    total = None
    for out in outs:
        X = Output.restore(out).X
        cols = tuple(X[c].values for c in ('time', 'x', 'y', 'z', 'vy', 'frac'))
        if keep is not None:
            cols = tuple(c[keep(T0 - cols[0])] for c in cols)
        vr, gt = float(out.vrplanet)/obj.unit_km, obj.g_tables(float(out.aplanet))
        ages = (AGES[2], T0) + AGES[:2]
        if cls is ModelImage:
            res = image_ages(*cols, vr, obj.image_rotation(), 'radiance', gt, (24, 16), (-4., 4.),
                             (-4., 4.), float(obj.Apix), *ages)
        else:
            res = camera_ages(*cols, obj.observer, obj.basis, obj.uedges, obj.vedges, vr,
                              obj.pix_area_cm2, 'radiance', gt, *ages)
        assert min(res.edge_guard, res.margin_guard, res.bin_guard) >= GUARD
        total = res if total is None else type(res)(
            *(a + b for a, b in zip(res[:5], total[:5])), 0, 0, 0, 0, 0)
    return total


@pytest.mark.parametrize('cls,params', [(ModelImage, IMAGE_PARAMS), (CameraImage, CAMERA_PARAMS)],
                         ids=['image', 'camera'])
def test_public_classes_resident_restored_and_restatement(ctx, small_run, cls, params):
    inputs, restored = small_run
    outs = inputs._catalogue
    plain = quiet(cls, inputs, params, context=ctx)
    resident = quiet(cls, inputs, params, context=ctx, ages=AGES)
    want = restated(cls, resident, outs)
    assert want.counts.sum() > 3000 and np.count_nonzero(want.packets.sum((0, 1))) > 90
    app = 1e23/(sum(o.totalsource for o in outs)/T0)
    ones = ([0.0, 1.0], [1.0, 1.0])
    t_s, m = 1000.0, 20
    step = ([t_s, np.nextafter(t_s, np.inf)], [0.0, 1.0])
    young = restated(cls, resident, outs, keep=lambda age: age <= 30.0*m + 15.0)
    assert 0 < young.image.sum() < 0.8*want.image.sum()
    made = [resident, quiet(cls, restored, params, context=ctx, ages=AGES)]
    if cls is ModelImage:
        made.append(quiet(inputs.produce_image, params, context=ctx, ages=AGES))
    assert all(o.resident_rows(ctx) is None for o in restored._catalogue)
    for obj in made + [resident]:           # (the first again: its block has been replaced since)
        assert obj.age_sums.shape == (24, 16, 102, 2)
        assert np.array_equal(obj.packet_image, want.counts)
        assert np.array_equal(obj.packet_image, plain.packet_image)
        np.testing.assert_allclose(obj.image, plain.image, rtol=1e-12, atol=0)
        # packets per plane: the device keeps no count per record, but with positive weights a
        # record is empty exactly where no packet was filed
        assert np.array_equal(obj.age_sums[..., 1] != 0, want.packets != 0)
        np.testing.assert_allclose(obj.age_sums, want.sums, rtol=1e-12, atol=0)
        assert obj.age_cube.shape == (24, 16, 100)
        assert np.array_equal(obj.age_cube, obj.age_sums[..., 1:-1, 0]*obj.atoms_per_packet)
        np.testing.assert_allclose(obj.atoms_per_packet, app, rtol=1e-14)
        np.testing.assert_allclose(obj.age_cube.sum(-1) + obj.age_below + obj.age_above, obj.image,
                                   rtol=1e-12, atol=0)
        assert np.array_equal(obj.age_edges, -15.0 + 30.0*np.arange(101))
        assert np.array_equal(obj.age_axis, 30.0*np.arange(100))
        filled = obj.age_sums[..., 1:-1, 1] != 0
        assert filled.sum() > 500 and not obj.age_effective_packets[~filled].any()
        assert np.all(obj.age_effective_packets[filled] >= 1 - 1e-12)
        # a source that never changed: the image, at every epoch
        steady = obj.transient([0.0, 5e4, -3e3], ones)
        assert np.array_equal(steady.kernel, np.ones((102, 3)))
        assert steady.images.shape == (3, 24, 16) == steady.effective_packets.shape
        for e in range(3):
            np.testing.assert_allclose(steady.images[e], obj.image, rtol=1e-12, atol=0)
        np.testing.assert_allclose(steady.light_curve, obj.image.sum(), rtol=1e-12)
        assert np.array_equal(steady.images, apply_ordered(obj.age_sums, steady.kernel)[..., 0]*app)
        # a source switched on at t_s, seen 30 m + 15 s later: the rows no older than that
        # (bin 0 holds the ages [-15, 15) s: an epoch 16 s before t_s has all of it before t_s)
        on = obj.transient([t_s + 30.0*m + 15.0, t_s - 16.0, t_s + 1e5], step)
        np.testing.assert_allclose(on.images[0], young.image*app, rtol=1e-12, atol=0)
        assert not on.images[1].any() and not on.effective_packets[1].any()
        # long after t_s: everything but the ages at or above a_hi, which stand for the rate long ago
        np.testing.assert_allclose(on.images[2], obj.age_below + obj.age_cube.sum(-1), rtol=1e-12,
                                   atol=0)
        assert obj.age_above.sum() > 0
        filed = young.packets.sum(-1)            # (a hidden or shadowed sample is counted, not filed)
        lit = filed > 0
        assert not on.effective_packets[0][~lit].any()
        assert np.all(on.effective_packets[0][lit] >= 1 - 1e-12)
        assert np.all(on.effective_packets[0][lit] <= filed[lit] + 1e-9)
    assert not hasattr(plain, 'age_sums') and plain.ages is None
    with pytest.raises(ValueError):
        plain.transient([0.0], ones)


def test_model_image_ages_around_io(ctx, tmp_path):
    """origin='Io': the age block of the rows moved into Io's frame, against the restatement over
    the moved columns (k_frame_rows copies the time column)."""
    from tests.test_gpu_moon_frame import IoRun
    run = IoRun(ctx, savepath=str(tmp_path))
    params = dict(origin='Io', dims='16,16', width='12,12', quantity='radiance')
    ages = (-15.0, 5985.0, 50)
    uploads = []
    upload = ctx.image_ages_upload
    ctx.image_ages_upload = lambda sums: (uploads.append(1), upload(sums))[1]
    try:
        img = quiet(ModelImage, run.inputs, params, context=ctx, ages=ages)
        # the block in HBM is still this object's total: applied where it is, nothing uploaded
        assert ctx.ages_owner['image'] is img._ages_token
        first = img.transient([0.0, 7.0], ([0.0], [1.0]))
        assert not uploads
        slabs = quiet(ModelImage, run.inputs, params, context=ctx, ages=ages, slab_rows=97)
        assert ctx.ages_owner['image'] is slabs._ages_token
        again = img.transient([0.0, 7.0], ([0.0], [1.0]))     # replaced since: set up and uploaded
        assert uploads == [1] and ctx.ages_owner['image'] is img._ages_token
        assert np.array_equal(again.images, first.images)
        ctx.image_clear()                                     # a clear drops the claim as well
        assert np.array_equal(img.transient([0.0, 7.0], ([0.0], [1.0])).images, first.images)
        assert uploads == [1, 1]
        # whatever else changes the block drops the claim too: an upload or a pass made on the
        # context directly, and the object's own create_image(), which bins one Output again
        upload(2.0*img.age_sums)
        assert 'image' not in ctx.ages_owner
        assert np.array_equal(img.transient([0.0, 7.0], ([0.0], [1.0])).images, first.images)
        ctx.image_ages_accumulate(rows=(run.out._store, 0, 100))
        assert 'image' not in ctx.ages_owner
        assert np.array_equal(img.transient([0.0, 7.0], ([0.0], [1.0])).images, first.images)
        quiet(img.create_image, run.out)
        assert ctx.ages_owner.get('image') is not img._ages_token
        assert np.array_equal(img.transient([0.0, 7.0], ([0.0], [1.0])).images, first.images)
        assert uploads == [1]*5
        plain = quiet(ModelImage, run.inputs, params, context=ctx)
        assert plain._ages_setup is None and plain._ages_token is None
    finally:
        del ctx.image_ages_upload
    x, y, z, vy, frac = run.five
    apix = (12/16)**2*(run.io_km*1e5)**2
    want = image_ages(run.rows[0], x, y, z, vy, frac, run.vr, img.image_rotation(), 'radiance',
                      run.g_tables, (16, 16), (-6., 6.), (-6., 6.), apix, 50, 6000.0, -15.0, 5985.0)
    assert min(want.edge_guard, want.margin_guard, want.bin_guard) >= GUARD
    assert want.counts.sum() > 1000 and np.count_nonzero(want.packets.sum((0, 1))) > 20
    for obj in (img, slabs):
        assert np.array_equal(obj.packet_image, want.counts)
        assert np.array_equal(obj.age_sums[..., 1] != 0, want.packets != 0)
        np.testing.assert_allclose(obj.age_sums, want.sums, rtol=1e-12, atol=0)
        np.testing.assert_allclose(obj.image, want.image*run.app, rtol=1e-12, atol=0)
        steady = obj.transient([0.0], ([0.0], [1.0]))
        np.testing.assert_allclose(steady.images[0], obj.image, rtol=1e-12, atol=0)


def test_an_adaptive_step_run_is_refused_with_the_reason(ctx):
    inputs = Input(INPUT)
    inputs.options.step_size = 0
    for build in (lambda: ModelImage(inputs, IMAGE_PARAMS, context=ctx, ages=AGES),
                  lambda: CameraImage(inputs, CAMERA_PARAMS, context=ctx, ages=AGES),
                  lambda: inputs.produce_image(IMAGE_PARAMS, context=ctx, ages=AGES)):
        with pytest.raises(NotImplementedError) as err:
            build()
        assert 'step_size = 0' in str(err.value) and 'final row' in str(err.value)
