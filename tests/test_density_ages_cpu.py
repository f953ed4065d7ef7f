"""ModelDensity(ages=...) without a GPU: the restatement the GPU tests lean on against a plain
double loop, the sum identity of a point's planes, every refusal of ``ages=`` (raised before a
context is opened), ``transient_track`` / ``transient_design`` against direct evaluations, the new
exports, and the enable's argument check as a host program (plain and under the host sanitizers).
The device is replaced by a stand-in that answers the density calls with the restatement
(AgesContext below)."""
import contextlib
import inspect
import io
import os
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

from tests.age_cube_restatement import apply_ordered, planes
from tests.density_ages_restatement import brute_force, restate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
COLUMNS = ('time', 'x', 'y', 'z', 'frac')
ENTRIES = ('enable', 'accumulate', 'accumulate_f32', 'accumulate_rows', 'download', 'upload', 'apply')


def _stand_in():
    from tests.oracle_context import OracleContext

    class AgesContext(OracleContext):
        """The density calls of hip_api.Context answered by the restatement over every sample
        handed in (host columns only); the block's apply by ``apply_ordered``."""

        def density_set(self, points, cell_start, origin, h, dr, dims):
            self._dpoints, self._ddr = np.array(points, dtype=np.float64).reshape(-1, 3), float(dr)
            self._dcols, self._dages, self._dblock = [], None, None
            self.ages_owner = {}
            self.sets = getattr(self, 'sets', 0) + 1

        def density_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
            self._dages = (int(na), float(t0), float(a_lo), float(a_hi))
            self.ages_owner.pop('density', None)

        def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
            self._dcols.append((np.zeros(len(x)), x, y, z, frac))

        def density_ages_accumulate(self, time=None, x=None, y=None, z=None, frac=None, rows=None):
            assert self._dages is not None, 'density_ages_enable has not been called'
            self.ages_owner.pop('density', None)
            self._dcols.append((time, x, y, z, frac))

        def _restated(self):
            cols = [np.concatenate([np.asarray(c, dtype=np.float64) for c in col])
                    for col in zip(*self._dcols)] if self._dcols else [np.zeros(0)]*5
            return restate(self._dpoints, self._ddr, *(self._dages or (1, 0., 0., 1.)), *cols)

        def density_download(self):
            got = self._restated()
            return got.s0.copy(), got.counts.copy()

        def density_ages_download(self):
            return self._restated().sums.copy()

        def density_ages_upload(self, sums):
            self.ages_owner.pop('density', None)
            self._dblock = np.array(sums, dtype=np.float64)
            self.uploads = getattr(self, 'uploads', 0) + 1

        def density_ages_apply(self, K):
            block = self._dblock if self._dblock is not None else self._restated().sums
            return apply_ordered(block, K)
    return AgesContext


def _fake_inputs(runs=(), endtime=None):
    from nexoclom_amd import Input
    inputs = Input(INPUT)
    if endtime is not None:
        inputs.options.endtime = type(inputs.options.endtime)(float(endtime), 's')
    inputs._catalogue = list(runs)
    return inputs


def _run(columns, totalsource=1000.):
    X = pd.DataFrame({c: np.asarray(v, dtype=np.float64) for c, v in zip(COLUMNS, columns)})
    return types.SimpleNamespace(X=X, totalsource=totalsource, npackets=len(X), idnum=1, filename='a')


def _model(runs, pts, dr=0.1, endtime=600., context=None, **kwargs):
    from nexoclom_amd import ModelDensity
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        return ModelDensity(_fake_inputs(runs, endtime), pts[:, 0], pts[:, 1], pts[:, 2], dr=dr,
                            context=context or _stand_in()(), **kwargs)


NEW_ATTRIBUTES = ('age_sums', 'age_density', 'age_below', 'age_above', 'age_edges', 'age_axis',
                  'age_effective_packets')


def _cloud(rng, p, dtype=np.float32, sixteenths=False):
    """time (multiples of 30 s in [0, 600]), x, y, z, frac"""
    frac = rng.integers(0, 17, p)/16 if sixteenths else rng.uniform(0, 1, p)
    cols = [30.*rng.integers(0, 21, p)] + [rng.uniform(-1, 1, p) for _ in range(3)] + [frac]
    return [c.astype(dtype) for c in cols]                  # widened, as stored rows are


def test_ages_keyword_exists():
    """The test that fails without the feature: ModelDensity takes ``ages``; without it the
    object has none of the new attributes and the same density."""
    from nexoclom_amd import ModelDensity
    assert 'ages' in inspect.signature(ModelDensity.__init__).parameters
    run = _run(([510.], [1.0], [0.], [0.], [0.5]))
    d = _model([run], [[1.0, 0., 0.], [np.nan, 0., 0.]], ages=(60., 300., 8))
    assert d.age_sums.shape == (2, 10, 2) and d.age_density.shape == (2, 8)
    assert all(hasattr(d, name) for name in NEW_ATTRIBUTES)
    assert np.array_equal(d.age_sums[0, 2], [0.5, 0.25])            # age 90 s: bin 1, plane 2
    assert np.count_nonzero(d.age_sums) == 2 and not d.age_sums[1].any()   # the left-out point
    assert np.array_equal(d.age_edges, 60. + 30.*np.arange(9))
    plain = _model([run], [[1.0, 0., 0.], [np.nan, 0., 0.]])
    assert not any(hasattr(plain, name) for name in NEW_ATTRIBUTES)
    assert np.array_equal(plain.density, d.density) and np.array_equal(plain.packets, d.packets)
    for call in (lambda: plain.transient([0.], ([0.], [1.])),
                 lambda: plain.transient_track(([0.], [1.]), 0.),
                 lambda: plain.transient_design([0.], 0.)):
        with pytest.raises(ValueError, match='needs an object built with ages='):
            call()


@pytest.mark.parametrize('na', [1, 8])
def test_restatement_equals_a_double_loop(na):
    rng = np.random.default_rng(3)
    cols = _cloud(rng, 1500)
    cols[0][::50] = np.nan                                  # a time that is not a number
    pts = np.concatenate([rng.uniform(-1, 1, (12, 3)), np.stack(cols[1:4], axis=1)[:4]])
    axis = (na, 600., 60., 300.)
    want = restate(pts, 0.5, *axis, *cols)
    sums, s0, counts, rows_n = brute_force(pts, 0.5, *axis, *cols)
    assert counts.sum() > 300 and np.all(rows_n.sum(0) > 0)          # every plane is met
    assert np.array_equal(want.sums, sums) and np.array_equal(want.s0, s0)
    assert np.array_equal(want.counts, counts) and np.array_equal(want.rows, rows_n)
    assert np.array_equal(want.rows.sum(1), want.counts)
    # the planes themselves, on edges: 60 s is the first bin, 300 s = a_hi the top plane, NaN too
    k, _ = planes(np.array([600., 570., 540., 510., 330., 300., 270., np.nan]), 8, 600., 60., 300.)
    assert k.tolist() == [0, 0, 1, 2, 8, 9, 9, 9]


def test_the_planes_of_a_point_sum_to_its_s0():
    """Fractions in sixteenths: every sum is exact, so the identity holds to the bit."""
    rng = np.random.default_rng(4)
    cols = _cloud(rng, 3000, sixteenths=True)
    pts = rng.uniform(-1, 1, (40, 3))
    want = restate(pts, 0.25, 8, 600., 60., 300., *cols)
    assert want.counts.sum() > 500 and (cols[4] == 0).any()
    assert np.array_equal(want.sums[:, :, 0].sum(1), want.s0)
    d = _model([_run(cols)], pts, dr=0.25, ages=(60., 300., 8))
    assert np.array_equal(d.age_sums, want.sums) and np.array_equal(d.packets, want.counts)
    scale = d.atoms_per_packet/float(d.Vpix)
    assert np.array_equal(d.age_sums[:, :, 0].sum(1)*d.atoms_per_packet/float(d.Vpix), d.density)
    total = d.age_density.sum(1) + d.age_below + d.age_above
    np.testing.assert_allclose(total, d.density, rtol=10*2.0**-52, atol=0)
    filled = d.age_sums[:, 1:-1, 1] != 0
    assert np.array_equal(d.age_effective_packets[filled],
                          d.age_sums[:, 1:-1, 0][filled]**2/d.age_sums[:, 1:-1, 1][filled])
    assert not d.age_effective_packets[~filled].any()


BAD = [('two numbers', (0., 1.)), ('a string', 'all'), ('no bins', (0., 1., 0)),
       ('fractional bins', (0., 1., 2.5)), ('empty', (5., 5., 4)), ('reversed', (5., 1., 4)),
       ('NaN', (np.nan, 1., 4)), ('infinite', (0., np.inf, 4)), ('width overflows', (-1.7e308, 1.7e308, 4))]


@pytest.mark.parametrize('bad', [b[1] for b in BAD], ids=[b[0] for b in BAD])
def test_a_bad_axis_is_refused_before_a_context_is_opened(bad):
    """No context is given and this machine may have no device: a ValueError, nothing else."""
    from nexoclom_amd import ModelDensity
    with pytest.raises(ValueError, match='ages='):
        ModelDensity(_fake_inputs(), [0., 1., 2.], [0., 0., 0.], [0., 0., 0.], ages=bad)


def test_too_many_records_are_refused_before_a_context_is_opened():
    from nexoclom_amd import ModelDensity
    zero = np.zeros(2**11)
    with pytest.raises(ValueError, match='2\\^31'):
        ModelDensity(_fake_inputs(), zero, zero, zero, ages=(0., 1., 2**20 - 2))
    with pytest.raises(RuntimeError, match='No packets'):      # one record fewer passes the check
        ModelDensity(_fake_inputs(), zero[:-1], zero[:-1], zero[:-1], ages=(0., 1., 2**20 - 2))


@pytest.mark.parametrize('kw', [dict(moments=True), dict(spectrum=dict(speed=(0., 4., 8))),
                                dict(cp=object())], ids=['moments', 'spectrum', 'cp'])
def test_model_density_refuses_ages_with(kw):
    from nexoclom_amd import ModelDensity
    with pytest.raises(NotImplementedError) as err:
        ModelDensity(_fake_inputs(), [0.], [0.], [0.], ages=(0., 600., 4), **kw)
    assert 'ages=' in str(err.value) and next(iter(kw)) in str(err.value)


def test_an_adaptive_step_run_is_refused():
    from nexoclom_amd import ModelDensity
    inputs = _fake_inputs()
    inputs.options.step_size = 0
    with pytest.raises(NotImplementedError, match='step_size = 0'):
        ModelDensity(inputs, [0.], [0.], [0.], ages=(0., 600., 4))


@pytest.fixture(scope='module')
def track():
    """A model on 30 points with every plane of the axis met, and its scale."""
    rng = np.random.default_rng(5)
    cols = _cloud(rng, 4000, sixteenths=True)
    pts = rng.uniform(-1, 1, (30, 3))
    pts[7] = np.nan                                          # left out of the index
    d = _model([_run(cols)], pts, dr=0.3, ages=(60., 300., 8))
    assert np.all(d.age_sums[:, :, 1].sum(0) > 0) and not d.age_sums[7].any()
    return d, d.atoms_per_packet/float(d.Vpix)


def test_track_of_a_constant_history_is_the_sum_of_the_planes(track):
    d, scale = track
    times = np.linspace(-500., 2000., 30)
    got = d.transient_track(([0., 100.], [1., 1.]), times)
    assert got.kernel.shape == (10, 30) and np.all(got.kernel == 1.0)
    assert np.array_equal(got.times, times)
    want = np.zeros(30)
    for k in range(10):
        want = want + d.age_sums[:, k, 0]
    assert np.array_equal(got.density, want*scale)
    np.testing.assert_allclose(got.density, d.age_density.sum(1) + d.age_below + d.age_above,
                               rtol=10*2.0**-52, atol=0)
    np.testing.assert_allclose(got.density, d.density, rtol=10*2.0**-52, atol=0)
    filled = d.age_sums[:, :, 1].sum(1) != 0
    assert got.effective_packets[7] == 0 and np.all(got.effective_packets[filled] > 0)
    one = d.transient_track(([0.], [1.]), 50.)                # one number for all points
    assert np.array_equal(one.times, np.full(30, 50.)) and np.array_equal(one.density, got.density)
    for bad in (np.zeros(29), [np.nan]*30, None):
        with pytest.raises(ValueError, match='transient'):
            d.transient_track(([0.], [1.]), bad)


def test_track_of_a_step_history_is_the_partial_sum_of_the_younger_planes(track):
    """The source switches on at t = 0 (a 1e-3 s ramp): at the time t_q = 60 + 30 j the bins
    younger than t_q -- planes 0 .. j, whose launch intervals lie after the step -- count in
    full and the older ones not at all."""
    d, scale = track
    history = ([-1e-3, 0.], [0., 1.])
    j = np.arange(30) % 9                                    # edges 60 .. 300 s
    times = 60. + 30.*j
    got = d.transient_track(history, times)
    ramp = np.zeros(30)                # ... but for the ramp's share of the bin that ends at the step
    for q in range(30):
        assert np.all(got.kernel[:1 + j[q], q] == 1.0) and not got.kernel[2 + j[q]:, q].any()
        if j[q] < 8:
            np.testing.assert_allclose(got.kernel[1 + j[q], q], 0.5e-3/30., rtol=1e-9)
            ramp[q] = d.age_sums[q, 1 + j[q], 0]*got.kernel[1 + j[q], q]
    want = np.array([d.age_sums[q, :1 + j[q], 0].sum() for q in range(30)])   # sixteenths: exact
    assert np.count_nonzero(want) >= 28 and np.any(want < d.age_sums[:, :, 0].sum(1))
    # a direct evaluation with the kernel itself, in apply_ordered's order
    direct = apply_ordered(d.age_sums, got.kernel)[np.arange(30), np.arange(30), 0]
    assert np.array_equal(got.density, direct*scale)
    # the partial sum is exact, the ramp's term one product: one rounding in their sum, one in scaling
    np.testing.assert_allclose(got.density, (want + ramp)*scale, rtol=4*2.0**-52, atol=0)
    assert np.array_equal(got.density[j == 8], want[j == 8]*scale)      # no ramp in view: exact


def test_design_times_rates_is_the_track(track):
    d, scale = track
    rng = np.random.default_rng(6)
    nodes = np.array([-400., -250., -100., 0., 130., 400.])
    rates = rng.uniform(0, 2, len(nodes))
    times = rng.uniform(-100., 500., 30)
    A = d.transient_design(nodes, times)
    assert A.shape == (30, len(nodes))
    got = d.transient_track((nodes, rates), times).density
    # A @ rates adds the same products S[q][k] K_j[k][q] rates[j] in another order
    J = len(nodes)
    K = np.stack([d.transient_track((nodes, np.eye(J)[j]), times).kernel for j in range(J)])
    for j in range(J):
        assert np.array_equal(A[:, j], d.transient_track((nodes, np.eye(J)[j]), times).density)
    terms = np.abs(d.age_sums[:, :, 0].T[None]*K*rates[:, None, None]).sum((0, 1))*scale
    err = np.abs(A @ rates - got)
    filled = terms > 0
    print('transient_design: max error over its bound', float(np.max(err[filled]/(J*2.0**-52*terms[filled]))))
    assert np.all(err <= J*2.0**-52*terms)


def test_transient_uploads_once_after_losing_the_block(track):
    """transient() against apply_ordered in the input's point order; an object that lost the
    context's block sets its index up again and uploads age_sums[index.order] once."""
    d, scale = track
    ctx = d.context()
    epochs = np.array([0., 100., 250.])
    history = ([0., 200.], [0.5, 2.0])
    first = d.transient(epochs, history)
    assert first.density.shape == (3, 30) and getattr(ctx, 'uploads', 0) == 0
    want = apply_ordered(d.age_sums, first.kernel)
    assert np.array_equal(first.density, want[..., 0]*scale)
    filled = want[..., 1] != 0
    assert np.array_equal(first.effective_packets[filled], want[filled][:, 0]**2/want[filled][:, 1])
    sets = ctx.sets
    ctx.ages_owner.pop('density', None)                      # another product took the block
    again = d.transient(epochs, history)
    assert ctx.sets == sets + 1 and ctx.uploads == 1
    assert np.array_equal(ctx._dblock, d.age_sums[d._index.order])
    assert np.array_equal(again.density, first.density)
    d.transient(epochs, history)
    assert ctx.uploads == 1


def test_the_library_exports_the_new_entry_points():
    from nexoclom_amd import hip_api
    names = [f'nxc_density_ages_{what}' for what in ENTRIES]
    assert all(name in hip_api.EXPORTS for name in names)
    for what in ('enable', 'accumulate', 'download', 'upload', 'apply'):
        assert callable(getattr(hip_api.Context, f'density_ages_{what}'))
    header = open(os.path.join(ROOT, 'include', 'nexoclom_hip.h')).read()
    assert all(f'int {name}(' in header for name in names)
    assert hip_api.ABI_VERSION == 3


@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_argument_check_as_a_host_program(tmp_path, flags):
    """nxc_density_ages_enable's refusals are host-only code (nxc_ages_check.hpp);
    tests/tools/density_ages_check.cpp feeds it good arguments, one bad set per refusal and na one
    below and at the 2^31 record limit.  Built plainly and with the host sanitizers; both runs
    must pass."""
    exe = tmp_path / 'density_ages_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'density_ages_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    assert sum(' refused: ' in line for line in lines) >= 21
    assert sum(line.endswith(' accepted') for line in lines) >= 8
    assert not done.stderr.strip()
