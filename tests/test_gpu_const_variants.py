"""Every reachable instantiation of k_const_fused through hip_api, at one small size: the force
model (plain, moons, surface re-emission) x full / reduced forces x image off / 64-bit / float32
samples x rows off / wide / narrow, and the streamed pass.  The specialisations are the same
arithmetic, so whichever one a call is routed to, its per-packet results must equal those of the
run without image: a launch that reaches the wrong instantiation, or hands it the wrong
arguments, shows up here."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N, STEP, N_ITER, EDGE = 257, 30.0, 16, 6.0       # more than one wave, fewer packets than lanes
ENDTIME = STEP*N_ITER


def forces(full):
    """full: gravity + radiation pressure + photo-loss (the compile-time specialisation);
    otherwise gravity + photo-loss."""
    return H.mercury_forces('Na', 1.3, True, full, 0.0)


def packets(seed):
    X0 = H.sample_x0(N, seed, ENDTIME, vprob=1.5, delv=1.2)
    X0[:, 0] = np.random.default_rng(seed + 1).random(N)*ENDTIME       # lifetimes differ
    X0[::19, 7] = 0.0                                                  # packets that start dead
    return X0


def bounce_cfg(f):
    return dict(GM=f.GM, unit_km=f.R_km, accomfactor=0.0, stickcoef=0.4, A=(0., 0., 0.), t0=100.,
                t1=600., temp_dependent=False, tx=np.zeros(8), ty=np.zeros(8), coef=np.zeros(16),
                seed=77)


def moons_cfg(f):
    a = 3.0
    return dict(moons=[dict(gm=f.GM*1e-2, radius=0.2, a=a, omega=float(np.sqrt(-f.GM/a**3)),
                            phi=0.5)], t0=ENDTIME)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def set_image(ctx, f, downcast):
    im = H.image_setup(f, 'radiance', dims=(32, 32))
    ctx.set_image(im['M'], f.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                  im['g_tables'], downcast_f32=downcast)


MODELS = [('plain', True), ('plain', False), ('moons', True), ('moons', False), ('bounce', True)]


@pytest.mark.parametrize('model,full', MODELS)
def test_image_and_rows_variants_give_the_finals_of_the_plain_launch(ctx, model, full):
    f = forces(full)
    X0 = packets(5)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(bounce_cfg(f) if model == 'bounce' else None)
    ctx.set_bodies(moons_cfg(f) if model == 'moons' else None)

    def fresh():
        ctx.upload_packets(X0)
        ctx.set_first_index(0)

    try:
        fresh()
        ref = ctx.integrate_const(STEP, N_ITER, EDGE, want_final=True, want_steps=True)
        final, steps = ref['final'], ref['steps']
        assert ctx.counters()['particle_steps'] > N and 0 < steps.max() <= N_ITER
        images = []
        for downcast in (False, True):
            set_image(ctx, f, downcast)
            fresh()
            got = ctx.integrate_const(STEP, N_ITER, EDGE, image=True, want_final=True,
                                      want_steps=True)
            assert np.array_equal(got['steps'], steps), downcast
            assert np.array_equal(bits(got['final']), bits(final)), downcast
            images.append(ctx.image_download())
            assert images[-1][1].sum() > 0
        # the float32 samples weigh differently: the two image precisions are two kernels
        assert not np.array_equal(images[0][0], images[1][0])
        live = final[:, 7] > 0
        assert live.any() and not live.all()
        want_len = steps + live
        for narrow in (False, True):
            fresh()
            res = ctx.integrate_const_rows(STEP, N_ITER, EDGE, narrow=narrow)
            assert np.array_equal(res['lengths'], want_len), narrow
            last = (np.cumsum(want_len) - 1)[live]
            with np.errstate(over='ignore', under='ignore'):
                want = final[live].astype(np.float32) if narrow else final[live]
            assert res['rows'].dtype == want.dtype
            assert np.array_equal(bits(res['rows'][:8, last].T), bits(want)), narrow
    finally:
        ctx.set_bounce(None)
        ctx.set_bodies(None)


@pytest.mark.parametrize('full', [True, False])
def test_streamed_variants_equal_the_uploaded_pass(ctx, full):
    f = forces(full)
    soa = np.ascontiguousarray(packets(9).T)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    for downcast in (False, True):
        set_image(ctx, f, downcast)
        ctx.upload_soa(soa)
        ctx.integrate_const(STEP, N_ITER, EDGE, image=True)
        want_ctr = ctx.counters()
        want, want_counts = ctx.image_download()
        ctx.image_clear()
        ctx.integrate_const_streamed(soa, STEP, N_ITER, EDGE, image=True, pieces=3)
        ctx.synchronize()
        assert ctx.counters() == want_ctr, downcast
        got, got_counts = ctx.image_download()
        assert np.array_equal(got_counts, want_counts) and want_counts.sum() > 100
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)
    ctx.upload_soa(soa)
    ctx.integrate_const(STEP, N_ITER, EDGE, image=False)
    want_ctr = ctx.counters()
    ctx.integrate_const_streamed(soa, STEP, N_ITER, EDGE, image=False, pieces=3)
    ctx.synchronize()
    assert want_ctr['particle_steps'] > N and ctx.counters() == want_ctr
