"""ModelDensity(moments=True) without a GPU: the host formulas (bulk velocity, covariance,
temperature, effective packets) on known answers and on a Maxwellian, a run shared by two ranks,
and the restatement the GPU tests lean on against a plain double loop.  The device is replaced by
a NumPy brute-force stand-in (MomentsContext below)."""
import contextlib
import inspect
import io
import multiprocessing as mp
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest

from tests.density_moments_restatement import MOMENT_COLUMNS, brute_force, products, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
COLUMNS = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')


def _stand_in():
    from tests.oracle_context import OracleContext

    class MomentsContext(OracleContext):
        """The density calls of hip_api.Context by brute force over every sample: membership in
        fp64, d = q - p, (dx*dx + dy*dy) + dz*dz <= dr*dr; the ten products of the restatement."""

        def density_set(self, points, cell_start, origin, h, dr, dims):
            self._dpoints, self._ddr = np.array(points, dtype=np.float64).reshape(-1, 3), float(dr)
            self._dsum = np.zeros(len(self._dpoints))
            self._dcount = np.zeros(len(self._dpoints))
            self._dmom = None

        def density_moments_enable(self, on=True):
            self._dmom = np.zeros((len(self._dpoints), 10)) if on else None

        def _add(self, cols, rows, moments):
            if rows is not None:
                store, first, count = rows
                r, _ = store.download(first, count, index=False)
                cols = r[1:8]
            x, y, z, vx, vy, vz, frac = (np.asarray(c).astype(np.float64) for c in cols)
            terms = products(vx, vy, vz, frac)
            for j, (qx, qy, qz) in enumerate(self._dpoints):
                dx, dy, dz = qx - x, qy - y, qz - z
                hit = (dx*dx + dy*dy) + dz*dz <= self._ddr*self._ddr
                self._dsum[j] += frac[hit].sum()
                self._dcount[j] += hit.sum()
                if moments:
                    self._dmom[j] += terms[hit].sum(axis=0)

        def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
            zero = None if rows is not None else np.zeros(len(x))
            self._add((x, y, z, zero, zero, zero, frac), rows, False)

        def density_moments_accumulate(self, x=None, y=None, z=None, vx=None, vy=None, vz=None,
                                       frac=None, rows=None):
            assert self._dmom is not None, 'density_moments_enable has not been called'
            self._add((x, y, z, vx, vy, vz, frac), rows, True)

        def density_download(self):
            return self._dsum.copy(), self._dcount.copy()

        def density_moments_download(self):
            return self._dmom.copy()
    return MomentsContext


def _fake_inputs(runs):
    from nexoclom_amd import Input
    inputs = Input(INPUT)
    inputs._catalogue = runs
    return inputs


def _run(columns, totalsource=1000.):
    X = pd.DataFrame({c: np.asarray(v, dtype=np.float64) for c, v in zip(COLUMNS, columns)})
    return types.SimpleNamespace(X=X, totalsource=totalsource, npackets=len(X), idnum=1, filename='a')


def _model(runs, pts, dr=0.1, **kwargs):
    from nexoclom_amd import ModelDensity
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        return ModelDensity(_fake_inputs(runs), pts[:, 0], pts[:, 1], pts[:, 2], dr=dr,
                            context=_stand_in()(), **kwargs)


def test_moments_keyword_exists():
    """The test that fails without the feature: ModelDensity takes ``moments``."""
    from nexoclom_amd import ModelDensity
    assert 'moments' in inspect.signature(ModelDensity.__init__).parameters
    run = _run(([1.0], [0.], [0.], [0.], [0.], [0.], [0.5]))
    d = _model([run], [[1.0, 0., 0.]], moments=True)        # TypeError on code without it
    assert d.moment_sums.shape == (1, 10) and len(MOMENT_COLUMNS) == 10
    plain = _model([run], [[1.0, 0., 0.]])
    assert not hasattr(plain, 'velocity') and not hasattr(plain, 'moment_sums')
    assert np.array_equal(plain.density, d.density) and np.array_equal(plain.packets, d.packets)


def test_known_answers():
    from nexoclom_amd import constants, Input
    R = float(Input(INPUT).geometry.planet.radius.value)
    m = constants.ATOMIC_MASS['Na'] * constants.AMU
    a = 2.0**-12                                            # R/s; every product below is exact
    # point 0: two rows of equal frac, v = (+-a, 0, 0); point 1: one row; point 2: none;
    # point 3: fracs 1 and 3
    cols = ([1.0, 1.02, 3.0, 7.0, 7.01], [0.]*5, [0.]*5,
            [a, -a, 3*a, a, a], [0., 0., -a, 0., 0.], [0., 0., 2*a, 0., 0.],
            [0.5, 0.5, 0.25, 1.0, 3.0])
    d = _model([_run(cols)], [[1.01, 0, 0], [3.0, 0, 0], [5.0, 0, 0], [7.0, 0, 0]], moments=True)
    assert np.array_equal(d.packets, [2, 1, 0, 2])
    ak = a*R
    np.testing.assert_allclose(d.velocity[0], [0, 0, 0], atol=0)
    want = np.zeros((3, 3))
    want[0, 0] = ak*ak
    np.testing.assert_allclose(d.velocity_covariance[0], want, rtol=1e-15, atol=0)
    np.testing.assert_allclose(d.temperature[0], m*(ak*1e3)**2/(3*constants.K_B), rtol=1e-14)
    assert d.effective_packets[0] == 2.0
    # one row: its own velocity, zero covariance and temperature, one packet
    np.testing.assert_allclose(d.velocity[1], [3*ak, -ak, 2*ak], rtol=1e-15)
    assert np.abs(d.velocity_covariance[1]).max() <= 4 * 2.0**-52 * (3*ak)**2
    assert abs(d.temperature[1]) <= m*1e6/(3*constants.K_B) * 12 * 2.0**-52 * (3*ak)**2
    assert d.effective_packets[1] == 1.0
    # no hits: NaN, NaN, NaN and 0; the density is 0 as before
    assert np.isnan(d.velocity[2]).all() and np.isnan(d.velocity_covariance[2]).all()
    assert np.isnan(d.temperature[2]) and d.effective_packets[2] == 0.0 and d.density[2] == 0.0
    # fracs 1 and 3: (1 + 3)^2 / (1 + 9)
    assert d.effective_packets[3] == 16/10
    assert d.velocity.shape == (4, 3) and d.velocity_covariance.shape == (4, 3, 3)
    assert d.temperature.shape == d.effective_packets.shape == (4,)
    assert np.array_equal(d.velocity_covariance, d.velocity_covariance.transpose(0, 2, 1),
                          equal_nan=True)
    # the sums are kept in the stated order
    np.testing.assert_array_equal(d.moment_sums[1], 0.25*np.array(
        [3*a, -a, 2*a, 9*a*a, a*a, 4*a*a, -3*a*a, 6*a*a, -2*a*a, 0.25]))


def test_maxwellian_is_recovered():
    """2e5 rows within dr of one point, velocities from a Maxwellian of 1200 K for Na plus 1 km/s
    along x.  The temperature estimate (3N degrees of freedom) has the standard error
    T sqrt(2 / (3N)); each bulk component sigma / sqrt(N) with sigma^2 = k_B T / m.  Equal fracs,
    so N is also the effective number of packets."""
    from nexoclom_amd import constants, Input
    R = float(Input(INPUT).geometry.planet.radius.value)
    m = constants.ATOMIC_MASS['Na'] * constants.AMU
    T, N = 1200., 200_000
    sigma = np.sqrt(constants.K_B*T/m) * 1e-3                # km/s per component
    rng = np.random.default_rng(31)
    v = rng.normal(0, sigma, (N, 3)) + [1.0, 0., 0.]
    xyz = 2.0 + rng.uniform(-0.02, 0.02, (N, 3))
    cols = (*xyz.T, *(v/R).T, np.full(N, 0.25))
    d = _model([_run(cols)], [[2.0, 2.0, 2.0]], moments=True)
    assert d.packets[0] == N
    np.testing.assert_allclose(d.effective_packets[0], N, rtol=1e-9)
    assert abs(d.temperature[0] - T) <= 4 * T*np.sqrt(2/(3*N))
    assert np.all(np.abs(d.velocity[0] - [1.0, 0., 0.]) <= 4 * sigma/np.sqrt(N))


def test_restatement_equals_a_double_loop():
    rng = np.random.default_rng(32)
    dr = 0.3
    cols = [rng.uniform(-1, 1, 300) for _ in range(3)] + \
           [rng.normal(1e-4, 1e-4, 300) for _ in range(3)] + [rng.uniform(0, 1, 300)]
    cols = [c.astype(np.float32) for c in cols]              # widened, as stored rows are
    pts = np.concatenate([rng.uniform(-1, 1, (37, 3)),
                          np.stack(cols[:3], axis=1)[:3].astype(np.float64)])
    want = restate(pts, dr, *cols)
    loop, terms = brute_force(pts, dr, *cols)
    assert np.array_equal(terms, products(*cols[3:]))        # bit-equal terms
    assert np.array_equal(want.counts, loop.counts) and want.counts.sum() > 100
    assert np.array_equal(want.bound, loop.bound) and np.array_equal(want.bound_s0, loop.bound_s0)
    assert np.all(np.abs(want.sums - loop.sums) <= want.bound)
    assert np.all(np.abs(want.s0 - loop.s0) <= want.bound_s0)


N, SIZE = 1000, 500                      # two Outputs of 500 packets: one per rank


def _points():
    rng = np.random.default_rng(11)
    return rng.uniform(-2, 2, 150), rng.uniform(-2, 2, 150), rng.uniform(-1, 1, 150)


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from nexoclom_amd import Input, ModelDensity
    from nexoclom_amd.distributed import ControlPlane
    cp = ControlPlane(world, rank, timeout=120)
    Ctx = _stand_in()

    def flow(cp_):
        inputs = Input(INPUT)
        inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
        ctx = Ctx()
        with contextlib.redirect_stdout(io.StringIO()):
            inputs.run(N, packs_per_it=SIZE, seed=5, context=ctx, cp=cp_)
            return inputs, ModelDensity(inputs, *_points(), dr=0.2, moments=True, cp=cp_,
                                        reduce='host', context=ctx)
    inputs, shared = flow(cp)
    assert len(inputs._catalogue) == 1                     # this rank's share
    if rank == 0:
        alone_inputs, alone = flow(None)
        assert len(alone_inputs._catalogue) == 2
        assert alone.packets.sum() > 100
        assert np.array_equal(shared.packets, alone.packets)
        np.testing.assert_allclose(shared.density, alone.density, rtol=1e-12, atol=0)
        # the sums, never the quotients
        np.testing.assert_allclose(shared.moment_sums, alone.moment_sums, rtol=1e-13, atol=0)
        hit = alone.packets > 0
        assert hit.sum() > 20 and np.isfinite(shared.temperature[hit]).all()
        assert np.isnan(shared.velocity[~hit]).all() and not shared.effective_packets[~hit].any()
        open(os.path.join(tmpdir, 'ok'), 'w').write('ok')
    cp.barrier()
    cp.close()


def test_two_ranks_equal_one_rank(tmp_path):
    port = 29300 + os.getpid() % 150
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / 'ok').exists()
