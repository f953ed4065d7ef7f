"""k_const_fused on a few waves: NXC_TEST_FUSED_WAVES = <blocks>x<waves per block> launches fewer
lanes than there are packets, so that at a few hundred packets a lane hands over to a second
packet (WaveQueue::refill and the per-lane reset beside it), a ballot crosses a chunk boundary,
the last chunk is short, and the claimed position lies beyond the queue with lanes still asking.

Expected values: the C checker (plain, moons), the NumPy oracle (re-emission), the oracle
context (rows) -- tests/lane_refill_cases.py.  One wave alone (1x1) takes the packets in a known
order, so its trips through the loop are those of tests/lane_refill_model.py exactly; with more
waves the hand-out is a race and the trips are bounded.  The inputs put every packet into a speed
bin of its own: within a bin the queue order is not fixed."""
import numpy as np
import pytest

from tests import helpers as H
from tests import lane_refill_cases as K
from tests import lane_refill_model as M
from tests.test_gpu_const_variants import MODELS, bits

pytestmark = pytest.mark.gpu

HOOK = 'NXC_TEST_FUSED_WAVES'
STEP, EDGE, N_ITER = K.STEP, K.EDGE, K.N_ITER
# re-emission against the NumPy oracle: the tolerances of test_surface_reemission_matches_oracle
BOUNCE_TOL = dict(rtol=1e-8, atol=1e-10)


def waves_of(shape):
    blocks, waves = shape.split('x')
    return int(blocks)*int(waves)


@pytest.fixture
def gpu(ctx):
    """The session's context; the force model a test sets does not outlive it."""
    yield ctx
    ctx.set_bounce(None)
    ctx.set_bodies(None)


def prepare(ctx, ref, monkeypatch, shape, ordered=True):
    """The condition on the inputs first (CPU): no two packets in neighbouring speed bins, where
    the test depends on the queue order.  Then the force model and the launch shape."""
    assert not ordered or K.distinct_bins(ref['X0']) >= 2
    H.set_ctx_forces(ctx, ref['f'])
    ctx.set_bounce(ref['bounce'])
    ctx.set_bodies(ref['bodies'])
    if shape is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, shape)


def fresh(ctx, ref):
    ctx.upload_packets(ref['X0'])
    ctx.set_first_index(0)


def set_image(ctx, f, im, downcast):
    ctx.set_image(im['M'], f.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                  im['g_tables'], downcast_f32=downcast)


def check_packets(ctx, got, ref):
    ctr = ctx.counters()
    assert np.array_equal(got['steps'], ref['steps'])
    if ref['bounce'] is None:
        assert np.array_equal(bits(got['final']), bits(ref['final']))
    else:
        np.testing.assert_allclose(got['final'], ref['final'], **BOUNCE_TOL)
    assert ctr['particle_steps'] == ref['work']
    assert ctr['nonfinite'] == 0 and ctr['unfinished'] == 0
    return ctr


def check_image(ctx, ref, image, counts):
    """Counters and the two images of an image pass against the checker's."""
    ctr = ctx.counters()
    got, got_counts = ctx.image_download()
    assert ctr['particle_steps'] == ref['work'] and ctr['samples'] == K.live_records(ref)
    assert ctr['samples_binned'] == int(counts.sum())
    assert ctr['nonfinite'] == 0 and ctr['unfinished'] == 0
    assert np.array_equal(got_counts, counts)
    # the order of the fp64 atomics is not fixed: the tolerance of test_bodies_parity_with_c_oracle;
    # re-emission: the oracle's samples are only that close to the kernel's
    np.testing.assert_allclose(got, image, rtol=1e-11 if ref['bounce'] is None else 1e-8, atol=0)


def check_trips(ctx, ref, shape, by_steps=False):
    trips = ctx.wave_trips()
    if shape == '1x1':
        assert trips == K.trips_1x1(ref, by_steps)[0]
    else:
        low, high = K.trip_bounds(ref, waves_of(shape))
        assert low <= trips <= high
    return trips


# ---- refill edges: one wave, plain forces ------------------------------------------------------
EDGE_CASES = [(n, N_ITER, '19th') for n in (1, 31, 32, 33, 63, 64, 65, 96, 97, 113, 257, 400)] + \
             [(200, N_ITER, 'all'), (97, 0, '19th'), (97, 1, '19th')]


@pytest.mark.parametrize('n,n_iter,dead', EDGE_CASES)
def test_one_wave_refills_its_lanes_as_the_model_says(gpu, monkeypatch, n, n_iter, dead):
    """A chunk of n - b < 32 packets, a ballot that wants more than the chunk has left, a claim
    beyond the queue with lanes asking, packets that end in their first trip: finals and steps
    bit for bit the checker's, wave_trips the model's, twice."""
    ref = K.reference('plain', True, n, n_iter, dead=dead)
    assert dead != 'all' or not ref['steps'].any()
    if n > 1 and n_iter > 1 and dead != 'all':              # lifetimes are not monotone in speed
        assert np.any(np.diff(ref['steps'][M.speed_order(ref['X0'])[0]]) > 0)
    prepare(gpu, ref, monkeypatch, '1x1')
    seen = []
    for _ in range(2):
        fresh(gpu, ref)
        got = gpu.integrate_const(STEP, n_iter, EDGE, want_final=True, want_steps=True)
        check_packets(gpu, got, ref)
        seen.append(check_trips(gpu, ref, '1x1'))
    assert seen[0] == seen[1]


@pytest.mark.parametrize('value', ['0x1', '1x13', '1x', 'x1', '1x1x', '1x1 ', '7', '-1x1', 'axb',
                                   '100000x1', ''])
def test_a_hook_value_out_of_range_or_malformed_is_ignored(gpu, monkeypatch, value):
    """... not an error: the launch is the one the packets size for themselves (ceil(n / 64) waves
    over as many blocks), its results the checker's."""
    ref = K.reference('plain', True, 200)
    prepare(gpu, ref, monkeypatch, value)
    fresh(gpu, ref)
    got = gpu.integrate_const(STEP, N_ITER, EDGE, want_final=True, want_steps=True)
    check_packets(gpu, got, ref)
    low, high = K.trip_bounds(ref, 4)
    assert low <= gpu.wave_trips() <= high


# ---- more waves on one queue head ----------------------------------------------------------------
@pytest.mark.parametrize('n', [65, 257, 400])
@pytest.mark.parametrize('shape', ['1x2', '2x1', '3x4'])
def test_waves_that_race_for_the_queue_head(gpu, monkeypatch, shape, n):
    ref = K.reference('plain', True, n)
    prepare(gpu, ref, monkeypatch, shape)
    fresh(gpu, ref)
    got = gpu.integrate_const(STEP, N_ITER, EDGE, want_final=True, want_steps=True)
    check_packets(gpu, got, ref)
    check_trips(gpu, ref, shape)


# ---- a lane's second packet in every variant -----------------------------------------------------
N_VARIANT = 257


def second_packets_after_a_bounce(ref):
    """Lanes of the one-wave schedule that take a packet which bounces after an earlier packet of
    theirs has bounced: a bounce count that survived the hand-over would draw the later packet's
    rebounds from the wrong Philox blocks."""
    order = M.speed_order(ref['X0'])[0]
    _, lane, _ = K.trips_1x1(ref)
    nb, found = ref['nbounce'], 0
    for l in range(64):
        mine = order[lane[order] == l]
        found += int(np.sum((np.cumsum(nb[mine])[:-1] > 0) & (nb[mine][1:] > 0)))
    return found


@pytest.mark.parametrize('shape', ['1x1', '1x2'])
@pytest.mark.parametrize('model,full', MODELS)
def test_second_packets_without_and_with_an_image(gpu, monkeypatch, model, full, shape):
    """Per-packet results without an image, and with one in both sample precisions: k, fresh and
    nbounce start again with the lane's next packet."""
    ref = K.reference(model, full, N_VARIANT)
    _, _, served = K.trips_1x1(ref)
    assert (served > 1).sum() >= N_VARIANT - 64 - 1        # lanes do take second packets
    if model == 'bounce':
        assert second_packets_after_a_bounce(ref) >= 10
    prepare(gpu, ref, monkeypatch, shape)
    fresh(gpu, ref)
    got = gpu.integrate_const(STEP, N_ITER, EDGE, want_final=True, want_steps=True)
    check_packets(gpu, got, ref)
    check_trips(gpu, ref, shape)
    for downcast in (False, True):
        im, image, counts = K.image_reference(model, full, N_VARIANT, downcast)
        assert counts.sum() > 1000
        set_image(gpu, ref['f'], im, downcast)
        fresh(gpu, ref)
        got = gpu.integrate_const(STEP, N_ITER, EDGE, image=True, want_final=True, want_steps=True)
        check_packets(gpu, got, ref)
        check_image(gpu, ref, image, counts)
        check_trips(gpu, ref, shape)


def narrow_bound(want):
    """|float32(g) - o| for g within BOUNCE_TOL of the oracle's o: that distance plus half a
    float32 ulp of g (2^-24 |g|; below the normal range less than the absolute part)."""
    near = BOUNCE_TOL['atol'] + BOUNCE_TOL['rtol']*np.abs(want)
    return near + 2.0**-24*(np.abs(want) + near)


@pytest.mark.parametrize('narrow', [False, True])
@pytest.mark.parametrize('shape', ['1x1', '1x2'])
@pytest.mark.parametrize('model,full', MODELS)
def test_second_packets_in_the_rows_passes(gpu, monkeypatch, model, full, shape, narrow):
    """Every row -- the eight state columns, lossfrac and the packet index -- of both passes of the
    rows protocol on few waves: lossfrac, row0 and nrow start again with the lane's next packet."""
    ref = K.reference(model, full, N_VARIANT)
    want, want_index, lengths = K.rows_reference(model, full, N_VARIANT, narrow)
    assert want.shape[1] == K.live_records(ref) and (want[8] > 0).sum() > 1000
    prepare(gpu, ref, monkeypatch, shape)
    fresh(gpu, ref)
    res = gpu.integrate_const_rows(STEP, N_ITER, EDGE, narrow=narrow, resident=True)
    try:
        rows, index = res['store'].download()
    finally:
        res['store'].free()
    ctr = gpu.counters()
    assert np.array_equal(res['lengths'], lengths)
    assert rows.dtype == want.dtype and index.dtype == want_index.dtype
    assert np.array_equal(index, want_index)
    if model != 'bounce':
        for c in range(9):
            assert np.array_equal(bits(rows[c]), bits(want[c])), c
    elif narrow:
        exact = K.rows_reference(model, full, N_VARIANT, False)[0]
        err = np.abs(rows.astype(np.float64) - exact)
        assert np.all(err <= narrow_bound(exact)), np.argwhere(err > narrow_bound(exact))[:5]
    else:
        np.testing.assert_allclose(rows, want, **BOUNCE_TOL)
    assert ctr['unfinished'] == 0 and ctr['nonfinite'] == 0
    assert ctr['particle_steps'] == ref['work']             # pass 2 takes the steps again
    check_trips(gpu, ref, shape, by_steps=True)


# ---- the per-wave image queue on a sparse wave ---------------------------------------------------
@pytest.mark.parametrize('downcast', [False, True])
def test_a_sparse_wave_fills_its_image_queue_over_several_trips(gpu, monkeypatch, downcast):
    """40 packets that all live to the end on one wave: at most 40 samples a trip, so the queue
    of 128 is popped every other trip, and the tail drains what is left, not a full wave."""
    ref = K.reference('plain', True, 40, source='long')
    im, image, counts = K.image_reference('plain', True, 40, downcast, source='long')
    assert ref['steps'].min() == N_ITER and K.live_records(ref) == 40*(N_ITER + 1)
    assert counts.sum() > 20*N_ITER and counts.sum() % 64 != 0
    prepare(gpu, ref, monkeypatch, '1x1', ordered=False)
    set_image(gpu, ref['f'], im, downcast)
    fresh(gpu, ref)
    got = gpu.integrate_const(STEP, N_ITER, EDGE, image=True, want_final=True, want_steps=True)
    check_packets(gpu, got, ref)
    check_image(gpu, ref, image, counts)
    assert gpu.wave_trips() == N_ITER + 1           # 40 lanes served at once, whatever the order


SMALL_FRAME = dict(center=(1.0, 0.5), width=(0.5, 0.5))


@pytest.mark.parametrize('downcast', [False, True])
def test_a_frame_that_few_samples_reach(gpu, monkeypatch, downcast):
    """300 packets on one wave and an image that holds a few per cent of their samples: the queue
    gains a handful of entries a trip."""
    ref = K.reference('plain', True, 300)
    im, image, counts = K.image_reference('plain', True, 300, downcast, **SMALL_FRAME)
    assert 0.01 <= counts.sum()/K.live_records(ref) <= 0.10
    prepare(gpu, ref, monkeypatch, '1x1')
    set_image(gpu, ref['f'], im, downcast)
    fresh(gpu, ref)
    got = gpu.integrate_const(STEP, N_ITER, EDGE, image=True, want_final=True, want_steps=True)
    check_packets(gpu, got, ref)
    check_image(gpu, ref, image, counts)
    check_trips(gpu, ref, '1x1')


# ---- the streamed pass ---------------------------------------------------------------------------
@pytest.mark.parametrize('image', [None, False, True])
@pytest.mark.parametrize('pieces', [1, 3, 32])
@pytest.mark.parametrize('shape', ['1x1', '1x2'])
def test_the_streamed_pass_on_few_waves(gpu, monkeypatch, shape, pieces, image):
    """A queue that is still being filled, in pieces of 3 to 4 packets when there are 32: a chunk
    spans piece boundaries.  image: None = without, else the sample precision."""
    n = 113
    ref = K.reference('plain', True, n)
    prepare(gpu, ref, monkeypatch, shape)
    soa = np.ascontiguousarray(ref['X0'].T)
    if image is None:
        gpu.integrate_const_streamed(soa, STEP, N_ITER, EDGE, image=False, pieces=pieces)
        gpu.synchronize()
        ctr = gpu.counters()
        assert ctr['particle_steps'] == ref['work']
        assert ctr['nonfinite'] == 0 and ctr['unfinished'] == 0
        return
    im, want, counts = K.image_reference('plain', True, n, image)
    assert counts.sum() > 1000
    set_image(gpu, ref['f'], im, image)
    gpu.integrate_const_streamed(soa, STEP, N_ITER, EDGE, image=True, pieces=pieces)
    gpu.synchronize()
    check_image(gpu, ref, want, counts)
