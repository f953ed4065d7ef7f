"""The nine entries through which stored samples reach their three consumers -- nxc_image_*,
nxc_density_* and nxc_camera_accumulate{, _f32, _rows} -- as one contract: what they refuse and in
which order, that the three routes of the same float32 samples (as they are, widened to float64 on
the host, as rows of a float32 store in HBM) bin the same, what a call without samples does to the
counters, and that a launch is timed.  Shapes near wave and workgroup boundaries: 0, 1, 65, 1025."""
import ctypes as C

import numpy as np
import pytest

from nexoclom_amd import hip_api
from nexoclom_amd.CameraImage import camera_basis
from nexoclom_amd.ModelDensity import DensityIndex
from oracle import np_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
FIRST = 777                           # the samples are rows FIRST .. FIRST + p of the store


class Image:
    entry, needs, clears = 'nxc_image_accumulate', (0, 1, 2, 3, 4), True
    message = 'nxc_set_image has not been called'

    def __init__(self, forces, rows):
        self.f = forces
        self.im = H.image_setup(forces, 'radiance', dims=(200, 120), width=(8., 6.))

    def set(self, ctx):
        im = self.im
        ctx.set_image(im['M'], self.f.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                      im['g_tables'])

    def accumulate(self, ctx, cols=None, rows=None):
        if rows is not None:
            ctx.image_accumulate_rows(*rows)
        else:
            ctx.image_accumulate(*cols)

    def download(self, ctx):
        return ctx.image_download()


class Density:
    entry, needs, clears = 'nxc_density_accumulate', (0, 1, 2, 4), False
    message = 'nxc_density_set has not been called'

    def __init__(self, forces, rows):
        # a dozen points at samples of every shape's range (p = 1: the sample itself), dr such that
        # their neighbours along the trajectory fall inside
        at = FIRST + np.array([0, 0, 1, 7, 31, 63, 64, 200, 511, 777, 1000, 1024])
        self.index = DensityIndex(rows[1:4, at].T.astype(np.float64), 0.05)
        assert len(self.index.points) == 12

    def set(self, ctx):
        i = self.index
        ctx.density_set(i.points, i.cell_start, i.origin, i.h, i.dr, i.dims)

    def accumulate(self, ctx, cols=None, rows=None):
        if rows is not None:
            ctx.density_accumulate(rows=rows)
        else:
            ctx.density_accumulate(*(cols[k] for k in self.needs))

    def download(self, ctx):
        return ctx.density_download()


class Camera:
    entry, needs, clears = 'nxc_camera_accumulate', (0, 1, 2, 3, 4), True
    message = 'nxc_camera_set has not been called'

    def __init__(self, forces, rows):
        self.f = forces
        self.o = np.array([1.5, -6.0, 2.0])
        self.basis = camera_basis(-self.o, (0, 0, 1))
        half = [np.tan(np.radians(a)/2) for a in (80, 60)]
        self.uedges = np.linspace(-half[0], half[0], 201)
        self.vedges = np.linspace(-half[1], half[1], 121)
        self.area = (2*half[0]/200)*(2*half[1]/120)*(2440.53e5)**2
        self.gt = H.g_tables('Na', forces.aplanet, forces.R_km, (5891, 5897))

    def set(self, ctx):
        ctx.camera_set(self.o, self.basis, self.f.vrplanet, self.area, 'radiance', self.uedges,
                       self.vedges, self.gt)

    def accumulate(self, ctx, cols=None, rows=None):
        if rows is not None:
            ctx.camera_accumulate(rows=rows)
        else:
            ctx.camera_accumulate(*cols)

    def download(self, ctx):
        return ctx.camera_download()


CONSUMERS = {'image': Image, 'density': Density, 'camera': Camera}


@pytest.fixture(scope='module')
def forces():
    return H.mercury_forces('Na', 1.3)


@pytest.fixture(scope='module')
def stored(ctx, forces):
    """(a float32 row store in HBM, its rows on the host)"""
    endtime, step = 3000., 30.
    X0 = H.sample_x0(300, 51, endtime)
    _, n_iter = O.n_output_steps(endtime, step)
    H.set_ctx_forces(ctx, forces)
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    store = ctx.integrate_const_rows(step, n_iter, 8.0, narrow=True, resident=True)['store']
    rows, _ = store.download(index=False)
    assert rows.dtype == np.float32 and store.total > FIRST + 1025 + 999
    yield store, rows
    store.free()


@pytest.fixture(params=sorted(CONSUMERS))
def consumer(request, forces, stored):
    return CONSUMERS[request.param](forces, stored[1])


def columns(rows, p, dtype=np.float32):
    return [np.ascontiguousarray(rows[c, FIRST:FIRST + p].astype(dtype)) for c in (1, 2, 3, 5, 7)]


def refused(code, text, call, *args, **kw):
    with pytest.raises(hip_api.HipError) as err:
        call(*args, **kw)
    assert err.value.code == code and text in str(err.value), str(err.value)


def raw(ctx, consumer, suffix, p, cols):
    """The host-column entry itself, with whatever pointers ``cols`` holds (None: a null one)"""
    kind = C.c_float if suffix == '_f32' else C.c_double
    ptrs = [None if cols[k] is None else cols[k].ctypes.data_as(C.POINTER(kind)) for k in consumer.needs]
    ctx._check(getattr(ctx.lib, consumer.entry + suffix)(ctx._h, C.c_int64(p), *ptrs))


def test_before_set_every_entry_reports_the_state_first(consumer, stored):
    store, rows = stored
    with hip_api.Context(0) as fresh:
        for dtype, suffix in ((np.float64, ''), (np.float32, '_f32')):
            cols = columns(rows, 4, dtype)
            refused(hip_api.NXC_ERR_STATE, consumer.message, consumer.accumulate, fresh, cols=cols)
            # ... also in front of the complaints about the arguments
            refused(hip_api.NXC_ERR_STATE, consumer.message, raw, fresh, consumer, suffix, -1, cols)
            refused(hip_api.NXC_ERR_STATE, consumer.message, raw, fresh, consumer, suffix, 4,
                    [None]*5)
        for first, count in ((0, 4), (-1, 4), (0, store.total + 1)):
            refused(hip_api.NXC_ERR_STATE, consumer.message, consumer.accumulate, fresh,
                    rows=(store, first, count))
        refused(hip_api.NXC_ERR_STATE, consumer.message, lambda: fresh._check(
            getattr(fresh.lib, consumer.entry + '_rows')(fresh._h, None, C.c_int64(0), C.c_int64(4))))


@pytest.mark.parametrize('p', [0, 1, 65, 1025])
def test_three_routes_of_the_same_samples_agree(ctx, consumer, stored, p):
    store, rows = stored
    routes = dict(f32=dict(cols=columns(rows, p)), f64=dict(cols=columns(rows, p, np.float64)),
                  rows=dict(rows=(store, FIRST, p)))
    got = {}
    for name, how in routes.items():
        consumer.set(ctx)                                   # zeroes the consumer's sums
        consumer.accumulate(ctx, **how)
        if p:
            assert ctx.last_kernel_ms() > 0
        got[name] = consumer.download(ctx) + (ctx.counters(),)
    sums, counts, ctr = got['f32']
    print(f'{type(consumer).__name__} p={p}: {int(np.asarray(counts, dtype=np.float64).sum())} hits, '
          f'counters {ctr}')
    if p == 0:
        assert not np.any(sums) and not np.any(counts)
    elif p > 1 or isinstance(consumer, Density):            # (one sample may lie outside an image)
        assert np.asarray(counts, dtype=np.float64).sum() >= 1
    if consumer.clears:
        assert ctr['samples'] == p and ctr['nonfinite'] == 0
    for name in ('f64', 'rows'):
        other_sums, other_counts, other_ctr = got[name]
        assert np.array_equal(other_counts, counts), name
        np.testing.assert_allclose(other_sums, sums, rtol=1e-12, atol=0, err_msg=name)
        assert other_ctr == ctr, name


def test_row_ranges_outside_the_store_are_refused(ctx, consumer, stored):
    store, _ = stored
    consumer.set(ctx)
    for first, count in ((store.total - 3, 4), (0, store.total + 1), (-1, 4), (-5, 2), (3, -1)):
        refused(hip_api.NXC_ERR_ARG, 'row range outside the store', consumer.accumulate, ctx,
                rows=(store, first, count))
    sums, counts = consumer.download(ctx)
    assert not np.any(sums) and not np.any(counts)


def test_null_columns_and_negative_counts_are_bad_arguments(ctx, consumer, stored):
    _, rows = stored
    consumer.set(ctx)
    for dtype, suffix in ((np.float64, ''), (np.float32, '_f32')):
        cols = columns(rows, 4, dtype)
        for k in consumer.needs:
            holed = [None if c == k else col for c, col in enumerate(cols)]
            refused(hip_api.NXC_ERR_ARG, 'bad arguments', raw, ctx, consumer, suffix, 4, holed)
        refused(hip_api.NXC_ERR_ARG, 'bad arguments', raw, ctx, consumer, suffix, -1, cols)
        raw(ctx, consumer, suffix, 0, [None]*5)             # nothing to read: null columns are fine
    sums, counts = consumer.download(ctx)
    assert not np.any(sums) and not np.any(counts)


def test_a_call_without_samples(ctx, consumer, stored, forces):
    """Image and camera zero the counters whenever they accept a call; density never touches
    them.  The sums stay as they are."""
    store, rows = stored
    other = Image(forces, rows)                             # leaves counters that are not zero
    other.set(ctx)
    other.accumulate(ctx, cols=columns(rows, 1025))
    left = ctx.counters()
    assert left['samples'] == 1025
    consumer.set(ctx)
    consumer.accumulate(ctx, rows=(store, FIRST, 1025))
    sums, counts = consumer.download(ctx)
    assert np.asarray(counts, dtype=np.float64).sum() >= 1
    if consumer.clears:
        left = ctx.counters()
        assert left['samples'] == 1025
    else:
        assert ctx.counters() == left                       # a density launch leaves them alone
    empties = [dict(cols=columns(rows, 0)), dict(cols=columns(rows, 0, np.float64)),
               dict(rows=(store, FIRST, 0)), dict(rows=(store, store.total, 0))]
    for how in empties:
        if consumer.clears:
            consumer.accumulate(ctx, rows=(store, FIRST, 65))
            assert ctx.counters()['samples'] == 65
            sums, counts = consumer.download(ctx)
        consumer.accumulate(ctx, **how)
        if consumer.clears:
            assert set(ctx.counters().values()) == {0}
        else:
            assert ctx.counters() == left
        after = consumer.download(ctx)
        assert np.array_equal(after[0], sums) and np.array_equal(after[1], counts)
