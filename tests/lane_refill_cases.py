"""Inputs and expected values of tests/test_gpu_lane_refill.py (TEST INFRASTRUCTURE): packets whose
queue order is known, and what the C checker, the NumPy oracle and the oracle context make of
them.  Nothing here touches a GPU; tests/test_lane_refill_model_cpu.py checks the conditions that
the GPU tests put on these inputs."""
import functools

import numpy as np

from oracle import np_oracle as O
from oracle.c_oracle import COracle
from tests import helpers as H
from tests import lane_refill_model as M
from tests.oracle_context import OracleContext, bodies_of, compact_rows
from tests.test_gpu_const_variants import bounce_cfg, forces, moons_cfg

STEP, EDGE, N_ITER = 30.0, 6.0, 40


def packets(n, seed, n_iter=N_ITER, dead='19th'):
    """n packets off the surface, every one in a speed bin of its own (the queue order after the
    upload is then M.speed_order's), remaining times drawn over (0, step n_iter], and every 19th
    packet -- or every packet -- dead at the start."""
    endtime = STEP*max(n_iter, 1)
    X0 = M.spread_speeds(H.sample_x0(n, seed, endtime, vprob=1.5, delv=1.2), seed + 1)
    X0[:, 0] = (1.0 - np.random.default_rng(seed + 2).random(n))*endtime
    if dead == 'all':
        X0[:, 7] = 0.0
    else:
        X0[7::19, 7] = 0.0
    return X0


def long_lived(n, seed):
    """n packets launched straight up at 3 to 4 km/s: none comes back, leaves or fades within
    N_ITER steps."""
    rng = np.random.default_rng(seed)
    X0 = H.sample_x0(n, seed, STEP*N_ITER)
    X0[:, 4:7] = X0[:, 1:4]*(rng.uniform(3.0, 4.0, n)/2440.53)[:, None]
    return X0


@functools.lru_cache(maxsize=None)
def checker():
    return COracle()


@functools.lru_cache(maxsize=None)
def reference(model, full, n, n_iter=N_ITER, seed=5, dead='19th', source='surface'):
    """What a run of `model` ('plain', 'moons', 'bounce') over the packets must give:
    X0, f, final (n, 8), steps, work, traj (8, n_iter + 1, n) and, for re-emission, the bounce
    counts.  Plain and moons: the C checker; re-emission: the NumPy oracle.  Computed once per
    case; callers leave it unchanged."""
    f = forces(full)
    X0 = long_lived(n, seed) if source == 'long' else packets(n, seed, n_iter, dead)
    out = dict(f=f, X0=X0, n_iter=n_iter, bounce=None, bodies=None, nbounce=None)
    if model == 'bounce':
        out['bounce'] = bounce_cfg(f)
        res, nb, work = O.constant_step_driver_bounce(f, X0, STEP*n_iter, STEP, EDGE,
                                                      dict(out['bounce'], tpow=0.25))
        traj = np.ascontiguousarray(res.transpose(1, 2, 0))            # (8, n_iter + 1, n)
        steps = (traj[7, :n_iter] > 0).sum(axis=0).astype(np.int64)
        out.update(traj=traj, steps=steps, work=work, nbounce=nb,
                   final=np.ascontiguousarray(traj[:, steps, np.arange(n)].T))
    else:
        if model == 'moons':
            out['bodies'] = moons_cfg(f)
        c = checker().integrate_const(f, X0, STEP, n_iter, EDGE, nrec=n_iter + 1,
                                      bodies=bodies_of(out['bodies']))
        out.update(traj=c['traj'], steps=c['steps'], work=c['work'], final=c['final'])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def live_records(ref):
    """Records with frac > 0: the samples of an image pass, the rows of a rows pass."""
    return int((ref['traj'][7] > 0).sum())


@functools.lru_cache(maxsize=None)
def image_reference(model, full, n, downcast, n_iter=N_ITER, seed=5, source='surface',
                    center=(0., 0.), width=(8., 8.)):
    """(image, counts) of the run of reference(...) with a 32 x 32 radiance image.  Plain and
    moons: the checker's own fused pass; re-emission: the checker's image of the NumPy oracle's
    live records."""
    ref = reference(model, full, n, n_iter, seed, source=source)
    f = ref['f']
    im = H.image_setup(f, 'radiance', dims=(32, 32), center=center, width=width)
    co = checker()
    desc = co.image_desc(im['M'], f.vrplanet, im['apix'], 'radiance', im['g_tables'],
                         im['xedges'], im['zedges'], downcast=downcast)
    if model == 'bounce':
        t = ref['traj']
        live = t[7] > 0
        image, counts = co.image(desc, t[1][live], t[2][live], t[3][live], t[5][live], t[7][live])
    else:
        c = co.integrate_const(f, ref['X0'], STEP, n_iter, EDGE, img=desc,
                               bodies=bodies_of(ref['bodies']))
        assert np.array_equal(c['steps'], ref['steps'])
        image, counts = c['image'], c['counts']
    image.setflags(write=False)
    counts.setflags(write=False)
    return im, image, counts


@functools.lru_cache(maxsize=None)
def rows_reference(model, full, n, narrow, n_iter=N_ITER, seed=5):
    """(rows (9, total), index, lengths) of integrate_const_rows over reference(...)'s packets:
    the oracle context's for plain and moons, the same compaction of the NumPy oracle's
    trajectory for re-emission."""
    ref = reference(model, full, n, n_iter, seed)
    if model == 'bounce':
        return compact_rows(ref['traj'], narrow)
    oc = OracleContext()
    H.set_ctx_forces(oc, ref['f'])
    oc.set_bodies(ref['bodies'])
    oc.upload_soa(ref['X0'].T)
    res = oc.integrate_const_rows(STEP, n_iter, EDGE, narrow=narrow, resident=True)
    rows, index = res['store'].download()
    return rows, index, res['lengths']


def trips_1x1(ref, by_steps=False):
    """(trips, lane, served) of one wave over reference(...)'s packets in the queue order after
    the upload, or (by_steps) in that of pass 2 of the rows protocol."""
    order = (M.steps_order(ref['steps'], ref['n_iter']) if by_steps
             else M.speed_order(ref['X0'])[0])
    return M.schedule(order, ref['steps'], len(order))


def trip_bounds(ref, waves):
    """(least, most) wave_trips of `waves` waves that race for one queue head.  A packet needs
    steps + 1 trips of a lane and a trip serves at most 64 lanes: at least ceil(sum / 64).  A
    wave makes no trip without a packet in a lane, so all trips together are at most that sum;
    the bound allows every wave its longest packet on top."""
    busy = int(np.sum(ref['steps'] + 1))
    return -(-busy//64), waves*(int(ref['steps'].max()) + 1) + busy


def distinct_bins(X0):
    """Smallest distance between the speed bins of two packets (the GPU tests want >= 2)."""
    bins = M.speed_order(X0)[1]
    return int(np.diff(np.sort(bins)).min()) if len(bins) > 1 else M.ORDER_BINS
