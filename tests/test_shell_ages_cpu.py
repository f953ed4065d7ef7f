"""ShellMap(ages=...) without a GPU: the restatement the GPU tests lean on
(tests/shell_ages_restatement.py) against a plain double loop, the sum identities of a record's and
a cell's planes, every refusal of ``ages=`` (raised before a context is opened),
``shell_ages_from_sums`` and ``TransientShells`` against direct evaluation, the unchanged call
sequence of the plain ShellMap, the new exports, and the enable's argument check as a host program
(plain and under the host sanitizers).  The device is replaced by a stand-in that answers the shell
calls with the restatement (ShellContext below)."""
import bisect
import contextlib
import inspect
import io
import math
import os
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

from tests.age_cube_restatement import apply_ordered
from tests.shell_ages_restatement import bound, guards_hold, shell_ages
from tests.shell_map_restatement import edges, shell_map

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INPUT = os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input')
HEADER = os.path.join(ROOT, 'include', 'nexoclom_hip.h')
COLUMNS = ('time', 'x', 'y', 'z', 'vy', 'frac')
ENTRIES = ('enable', 'accumulate', 'accumulate_f32', 'accumulate_rows', 'download', 'upload', 'apply')
GOOD = dict(quantity='column', dims='8,6', altitude='0.5,2.5,4')
AGES = (60., 300., 8)
CONSTANT_G = [(np.array([-1e30, 1e30]), np.array([2.5, 2.5]))]
NEW_ATTRIBUTES = ('shell_age_sums', 'age_density', 'age_density_below', 'age_density_above',
                  'age_column_profile', 'age_column', 'age_column_below', 'age_column_above',
                  'age_edges', 'age_axis', 'age_density_effective_packets',
                  'age_column_effective_packets')


class ShellContext:
    """The shell calls of hip_api.Context answered by the restatement over every sample handed in
    (host columns only); the block's apply by ``apply_ordered`` per plane.  ``calls`` keeps the
    names of the calls in their order."""

    def __init__(self):
        self.calls, self.ages_owner = [], {}
        self.sets = self.uploads = 0
        self._cols, self._ages, self._block, self._last = [], None, None, 0

    def shell_set(self, vrplanet, quantity, lon_edges, mu_edges, r_lo, r_hi, nalt, g_tables=()):
        self.calls.append('shell_set')
        self._desc = (float(vrplanet), quantity, list(g_tables), len(lon_edges) - 1,
                      len(mu_edges) - 1, float(r_lo), float(r_hi), int(nalt))
        self._cols, self._ages, self._block = [], None, None
        self.ages_owner.pop('shell', None)
        self.sets += 1

    def shell_ages_enable(self, na, t0=0.0, a_lo=0.0, a_hi=0.0):
        self.calls.append('shell_ages_enable')
        self._ages = (int(na), float(t0), float(a_lo), float(a_hi))
        self._block = None
        self.ages_owner.pop('shell', None)

    def shell_accumulate(self, x=None, y=None, z=None, vy=None, frac=None, rows=None):
        self.calls.append('shell_accumulate')
        self._cols.append((np.zeros(len(x)), x, y, z, vy, frac))
        self._last = len(x)

    def shell_ages_accumulate(self, time=None, x=None, y=None, z=None, vy=None, frac=None,
                              rows=None):
        self.calls.append('shell_ages_accumulate')
        assert self._ages is not None, 'shell_ages_enable has not been called'
        self.ages_owner.pop('shell', None)
        self._cols.append((time, x, y, z, vy, frac))
        self._last = len(x)

    def counters(self):
        self.calls.append('counters')
        return {'samples': self._last, 'samples_binned': self._last, 'nonfinite': 0}

    def _restated(self):
        cols = [np.concatenate([np.asarray(c, dtype=np.float64) for c in col])
                for col in zip(*self._cols)] if self._cols else [np.zeros(0)]*6
        return shell_ages(*cols, *self._desc, *(self._ages or (1, 0., 0., 1.)))

    def shell_download(self):
        self.calls.append('shell_download')
        base = self._restated().base
        return base.column.copy(), base.counts.astype(np.uint64), base.sums.copy()

    def shell_ages_download(self):
        self.calls.append('shell_ages_download')
        return self._restated().block.copy()

    def shell_ages_upload(self, sums):
        self.calls.append('shell_ages_upload')
        self.ages_owner.pop('shell', None)
        self._block = np.array(sums, dtype=np.float64)
        self.uploads += 1

    def shell_ages_apply(self, K):
        self.calls.append('shell_ages_apply')
        block = self._block if self._block is not None else self._restated().block
        return np.stack([apply_ordered(block[plane], K) for plane in (0, 1)])


def _inputs(runs=(), endtime=600.):
    from nexoclom_amd import Input
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(float(endtime), 's')
    inputs._catalogue = list(runs)
    return inputs


def _run(columns, totalsource=1000.):
    X = pd.DataFrame({c: np.asarray(v, dtype=np.float64) for c, v in zip(COLUMNS, columns)})
    return types.SimpleNamespace(X=X, totalsource=totalsource, npackets=len(X), idnum=1,
                                 filename='a', aplanet=0.35, vrplanet=-8.0)


def _map(runs, params=GOOD, context=None, **kwargs):
    from nexoclom_amd import ShellMap
    with contextlib.redirect_stdout(io.StringIO()):
        return ShellMap(_inputs(runs), params, context=context or ShellContext(), **kwargs)


def _cloud(rng, p, sixteenths=True, extent=4.0):
    """time (multiples of 30 s in [0, 600]), x, y, z, vy, frac: float32 values widened, as stored
    rows are; fractions in sixteenths, zeros among them"""
    d = rng.normal(size=(p, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pos = d*rng.uniform(1.0, extent, p)[:, None]
    frac = rng.integers(0, 17, p)/16 if sixteenths else rng.uniform(0, 1, p)
    cols = [30.*rng.integers(0, 21, p), pos[:, 0], pos[:, 1], pos[:, 2],
            rng.uniform(-4e-3, 5e-3, p), frac]
    return [c.astype(np.float32).astype(np.float64) for c in cols]


def brute_force(cols, vrplanet, g, nlon, nlat, r_lo, r_hi, nalt, na, t0, a_lo, a_hi):
    """"ShellMap" steps 1 to 8 and "ShellMap ages" by a loop over the rows, every operation on
    Python floats, adding in row order: (block, rows per record).  ``g``: None for quantity
    'column', else the constant g-value of a one-line radiance."""
    lon_e, mu_e = (e.tolist() for e in edges(nlon, nlat))
    inv_dr, inv_da = float(nalt)/(r_hi - r_lo), float(na)/(a_hi - a_lo)
    block = np.zeros((2, nlon, nlat, nalt + 2, na + 2, 2))
    rows = np.zeros((nlon, nlat, nalt + 2, na + 2), dtype=np.int64)

    def bin_of(v, e):
        if not e[0] <= v <= e[-1]:
            return -1
        return len(e) - 2 if v == e[-1] else bisect.bisect_right(e, v) - 1

    for t, x, y, z, vy, f in zip(*([float(v) for v in c] for c in cols)):
        radvel = vy + vrplanet
        r2 = (x*x + y*y) + z*z
        r = math.sqrt(r2)
        if r == 0.0:
            continue
        mu = z/r
        lon = float(np.arctan2(x, -y))
        if lon < 0:
            lon = lon + 2*np.pi
        ix, iz = bin_of(lon, lon_e), bin_of(mu, mu_e)
        if ix < 0 or iz < 0:
            continue
        if g is None:
            w = f
        else:
            if not ((x*x + z*z > 1.0 + 2.0**-52) or y < 0):
                f = f*0.0
            w = (f*g)/1e6
        if not math.isfinite(w) or math.isnan(radvel):
            continue
        c = w/r2
        if not math.isfinite(c) or w == 0:
            continue
        u = (r - r_lo)*inv_dr
        k = 0 if u < 0 else 1 + int(u) if u < nalt else nalt + 1
        age = t0 - t
        u = (age - a_lo)*inv_da
        ka = 0 if u < 0 else 1 + int(u) if u < na else na + 1
        rows[ix, iz, k, ka] += 1
        block[0, ix, iz, k, ka] += (w, w*w)
        block[1, ix, iz, k, ka] += (c, c*c)
    return block, rows


def test_ages_keyword_exists():
    """The test that fails without the feature: ShellMap takes ``ages``; without it the object
    has none of the new attributes and the same map."""
    from nexoclom_amd import ShellMap
    assert 'ages' in inspect.signature(ShellMap.__init__).parameters
    # one sample at dusk, r = 2 (altitude 1.0: bin 1 of 4 over [0.5, 2.5)), age 90 s: age bin 1
    run = _run(([510.], [2.0], [0.], [0.], [1e-3], [0.5]))
    sm = _map([run], ages=AGES)
    assert sm.shell_age_sums.shape == (2, 8, 6, 6, 10, 2)
    assert all(hasattr(sm, name) for name in NEW_ATTRIBUTES)
    assert sm.age_density.shape == (8, 6, 4, 8) == sm.age_column_profile.shape
    assert sm.age_density_below.shape == (8, 6, 4) == sm.age_density_above.shape
    assert sm.age_column.shape == (8, 6, 8) and sm.age_column_below.shape == (8, 6)
    ix, iz = 2, 3                                     # lon pi/2 of 8 bins, mu 0 of 6 bands
    assert np.array_equal(sm.shell_age_sums[0, ix, iz, 2, 2], [0.5, 0.25])
    assert np.array_equal(sm.shell_age_sums[1, ix, iz, 2, 2], [0.125, 0.015625])
    assert np.count_nonzero(sm.shell_age_sums) == 4
    assert np.array_equal(sm.age_edges, 60. + 30.*np.arange(9))
    assert np.array_equal(sm.age_axis, 75. + 30.*np.arange(8))
    assert np.count_nonzero(sm.age_density) == 1 and sm.age_density[ix, iz, 1, 1] == sm.density[ix, iz, 1]
    assert sm.age_column[ix, iz, 1] == sm.column[ix, iz] > 0
    plain = _map([run])
    assert not any(hasattr(plain, name) for name in NEW_ATTRIBUTES) and plain.ages is None
    assert np.array_equal(plain.density, sm.density) and np.array_equal(plain.column, sm.column)
    assert np.array_equal(plain.shell_sums, sm.shell_sums) and np.array_equal(plain.packets, sm.packets)
    with pytest.raises(ValueError, match='needs an object built with ages='):
        plain.transient([0.], ([0.], [1.]))


@pytest.mark.parametrize('quantity', ['column', 'radiance'])
@pytest.mark.parametrize('na', [1, 8])
def test_restatement_equals_a_double_loop(na, quantity):
    rng = np.random.default_rng(3)
    cols = _cloud(rng, 3000, sixteenths=False)
    cols[0][::50] = np.nan                                   # a time that is not a number
    cols[5][::7] = 0.0                                       # not filed
    cols[1][11] = cols[2][11] = cols[3][11] = 0.0            # at the centre: not located
    cols[4][13] = np.nan                                     # radvel NaN: dropped
    grid, alt, axis = (5, 3), (1.5, 3.5, 4), (na, 600., 60., 300.)
    g = None if quantity == 'column' else 2.5
    want = shell_ages(*cols, 2e-4, quantity, CONSTANT_G if g else [], *grid, *alt, *axis)
    assert guards_hold(want)
    block, rows = brute_force(cols, 2e-4, g, *grid, *alt, *axis)
    assert rows.sum() > 1500 and np.all(rows.sum(axis=(0, 1, 2)) > 0)       # every age plane is met
    assert np.all(rows.sum(axis=(0, 1, 3)) > 0)                              # and every altitude record
    assert np.array_equal(want.rows, rows) and np.array_equal(want.block, block)
    assert want.base.binned - rows.sum() >= 3000//7 - 2                      # the zeros were binned, not filed
    # the base is the plain restatement's
    plain = shell_map(*cols[1:], 2e-4, quantity, CONSTANT_G if g else [], *grid, *alt)
    assert np.array_equal(want.base.sums, plain.sums) and np.array_equal(want.base.counts, plain.counts)


def test_the_planes_of_a_record_sum_to_the_record():
    """Fractions in sixteenths: sums of w and w w are exact, so plane A's identity holds to the
    bit; plane B's and the cell's column per age hold to the summation bound."""
    rng = np.random.default_rng(4)
    cols = _cloud(rng, 6000)
    grid, alt = (8, 6), (1.5, 3.5, 4)
    want = shell_ages(*cols, 2e-4, 'column', [], *grid, *alt, 8, 600., 60., 300.)
    assert guards_hold(want) and want.rows.sum() > 4000 and (cols[5] == 0).any()
    assert np.array_equal(want.block[0].sum(axis=-2), want.base.sums[0])
    assert np.all(want.rows.sum(axis=(2, 3)) <= want.base.counts)
    n = want.rows.sum(-1)
    limit = (n*2.0**-52)[..., None]*want.base.abs_sums[1]*2
    assert np.all(np.abs(want.block[1].sum(axis=-2) - want.base.sums[1]) <= limit)
    per_cell = want.block[1, ..., 0].sum(axis=(2, 3))
    np.testing.assert_allclose(per_cell, want.base.column, rtol=1e-12, atol=0)
    # bound(): nothing for a record of one row or none, (n - 1) 2^-52 sum |term| otherwise
    b = bound(want)
    assert b.shape == want.block.shape and not b[:, want.rows <= 1].any()
    many = want.rows > 1
    assert np.array_equal(b[0][many][:, 0], (want.rows[many] - 1)*2.0**-52*want.abs_block[0][many][:, 0])


BAD = [('two numbers', (0., 1.)), ('a string', 'all'), ('no bins', (0., 1., 0)),
       ('fractional bins', (0., 1., 2.5)), ('empty', (5., 5., 4)), ('reversed', (5., 1., 4)),
       ('NaN', (np.nan, 1., 4)), ('infinite', (0., np.inf, 4)), ('width overflows', (-1.7e308, 1.7e308, 4))]


def _refused(params=GOOD, inputs=None, **kw):
    """No context is given and this machine may have no device: the refusal, nothing else."""
    from nexoclom_amd import ShellMap
    return ShellMap(inputs or _inputs(), params, **kw)


@pytest.mark.parametrize('bad', [b[1] for b in BAD], ids=[b[0] for b in BAD])
def test_a_bad_axis_is_refused_before_a_context_is_opened(bad):
    with pytest.raises(ValueError, match='ages='):
        _refused(ages=bad)


def test_too_many_records_are_refused_before_a_context_is_opened():
    params = dict(GOOD, dims='64,64', altitude='0,1,126')             # 2^19 records
    with pytest.raises(ValueError, match='2\\^31'):
        _refused(params, ages=(0., 1., 2**12 - 2))
    sm = _map([], params, context=object(), ages=(0., 1., 1))          # well below: built
    assert sm.shell_age_sums.shape == (2, 64, 64, 128, 3, 2)


@pytest.mark.parametrize('kw', [dict(moments=True), dict(npackets=1000), dict(cp=object()),
                                dict(shard=(0, 10))], ids=['moments', 'npackets', 'cp', 'shard'])
def test_shell_map_refuses_ages_with(kw):
    with pytest.raises(NotImplementedError) as err:
        _refused(ages=AGES, **kw)
    text = str(err.value)
    if 'moments' in kw:
        assert 'ages=' in text and 'moments' in text and 'make two objects' in text
        assert 'image' not in text
    if 'moments' not in kw:
        with pytest.raises(NotImplementedError):           # ... and without ages, as before
            _refused(**kw)
    with pytest.raises(TypeError):
        _refused(ages=AGES, no_such_keyword=1)


def test_an_adaptive_step_run_is_refused():
    inputs = _inputs()
    inputs.options.step_size = 0
    with pytest.raises(NotImplementedError, match='step_size = 0'):
        _refused(inputs=inputs, ages=AGES)


def test_a_moon_that_takes_no_part_is_refused_as_before():
    with pytest.raises(NotImplementedError):
        _map([], dict(GOOD, origin='Io'), context=object(), ages=AGES)


def test_the_plain_call_sequence_is_unchanged():
    rng = np.random.default_rng(5)
    run = _run(_cloud(rng, 500))
    ctx = ShellContext()
    _map([run], context=ctx)
    assert ctx.calls == ['shell_set', 'shell_accumulate', 'counters', 'shell_download']
    aged = ShellContext()
    _map([run], context=aged, ages=AGES)
    assert aged.calls == ['shell_set', 'shell_ages_enable', 'shell_ages_accumulate', 'counters',
                          'shell_download', 'shell_ages_download']
    assert aged._ages == (8, 600., 60., 300.)                # the epoch is the run's endtime


@pytest.fixture(scope='module')
def aged_map():
    rng = np.random.default_rng(6)
    cols = _cloud(rng, 8000)
    sm = _map([_run(cols)], ages=AGES)
    want = shell_ages(*cols, sm._ctx._desc[0], 'column', [], 8, 6, 1.5, 3.5, 4, 8, 600., 60., 300.)
    assert guards_hold(want) and np.all(want.rows.sum(axis=(0, 1, 2)) > 0)
    return sm, want


def test_published_arrays_against_direct_evaluation(aged_map):
    from nexoclom_amd.ShellMap import shell_ages_from_sums
    sm, want = aged_map
    assert np.array_equal(sm.shell_age_sums, want.block)
    A, B = want.block
    R_cm = sm.unit_km*1e5
    per_area = sm.atoms_per_packet/(sm.solid_angle*R_cm**2)
    V = sm._volume*R_cm**3
    assert np.array_equal(sm.age_density, A[:, :, 1:-1, 1:-1, 0]*sm.atoms_per_packet/V[:, None])
    assert np.array_equal(sm.age_density_below, A[:, :, 1:-1, 0, 0]*sm.atoms_per_packet/V)
    assert np.array_equal(sm.age_density_above, A[:, :, 1:-1, -1, 0]*sm.atoms_per_packet/V)
    assert np.array_equal(sm.age_column_profile, B[:, :, 1:-1, 1:-1, 0]*per_area)
    cell = np.zeros((8, 6, 10, 2))
    for k in range(6):
        cell = cell + B[:, :, k]
    assert np.array_equal(sm.age_column, cell[:, :, 1:-1, 0]*per_area)
    assert np.array_equal(sm.age_column_below, cell[:, :, 0, 0]*per_area)
    assert np.array_equal(sm.age_column_above, cell[:, :, -1, 0]*per_area)
    filled = A[:, :, 1:-1, 1:-1, 1] != 0
    assert filled.sum() > 500 and not sm.age_density_effective_packets[~filled].any()
    assert np.array_equal(sm.age_density_effective_packets[filled],
                          A[:, :, 1:-1, 1:-1, 0][filled]**2/A[:, :, 1:-1, 1:-1, 1][filled])
    cfilled = cell[:, :, 1:-1, 1] != 0
    assert np.array_equal(sm.age_column_effective_packets[cfilled],
                          cell[:, :, 1:-1, 0][cfilled]**2/cell[:, :, 1:-1, 1][cfilled])
    assert not sm.age_column_effective_packets[~cfilled].any()
    # the pure function gives the same from the same sums
    again = shell_ages_from_sums(want.block, sm.atoms_per_packet, sm.solid_angle, sm._volume, R_cm,
                                 60., 300.)
    assert set(again) == set(NEW_ATTRIBUTES) - {'shell_age_sums'}
    assert all(np.array_equal(again[name], getattr(sm, name)) for name in again)
    # the identities, to rounding: the planes and the plain sums add the same terms in two orders
    total = sm.age_density.sum(-1) + sm.age_density_below + sm.age_density_above
    assert np.array_equal(want.block[0, ..., 0].sum(-1), want.base.sums[0, ..., 0])      # sixteenths
    np.testing.assert_allclose(total, sm.density, rtol=16*2.0**-52, atol=0)
    total = sm.age_column.sum(-1) + sm.age_column_below + sm.age_column_above
    np.testing.assert_allclose(total, sm.column, rtol=1e-12, atol=0)
    assert (sm.column > 0).all()


def test_a_constant_history_returns_the_steady_state(aged_map):
    sm, want = aged_map
    epochs = np.array([-500., 0., 100., 2000.])
    got = sm.transient(epochs, ([0., 100.], [1., 1.]))
    assert got.kernel.shape == (10, 4) and np.all(got.kernel == 1.0)
    assert np.array_equal(got.epochs, epochs)
    assert got.density.shape == (4, 8, 6, 4) == got.column_profile.shape
    assert got.column.shape == (4, 8, 6) == got.column_effective_packets.shape
    for e in range(4):
        np.testing.assert_allclose(got.density[e], sm.density, rtol=16*2.0**-52, atol=0)
        np.testing.assert_allclose(got.column[e], sm.column, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got.column_profile[e], sm.column_profile, rtol=1e-12, atol=0)
    inside = want.base.sums[0, ..., 1:-1, 0].sum()                    # sixteenths: exact
    np.testing.assert_allclose(got.content, sm.atoms_per_packet*inside, rtol=16*2.0**-52, atol=0)
    assert np.all(got.density_effective_packets[0][sm.density > 0] >= 1 - 1e-12)


def test_transient_against_direct_evaluation_and_one_upload(aged_map):
    from nexoclom_amd.transient import TransientShells, response_matrix
    sm, want = aged_map
    ctx = sm.context()
    epochs, history = np.array([0., 100., 250.]), ([-1e-3, 0.], [0., 1.])     # switched on at t = 0
    uploads = ctx.uploads
    first = sm.transient(epochs, history)
    assert ctx.uploads == uploads                  # the resident sums are this object's
    K = response_matrix(sm.age_edges, epochs, history)
    assert np.array_equal(first.kernel, K)
    direct = np.stack([apply_ordered(want.block[plane], K) for plane in (0, 1)])
    R_cm = sm.unit_km*1e5
    per_area = sm.atoms_per_packet/(sm.solid_angle*R_cm**2)
    assert np.array_equal(first.density,
                          direct[0][..., 1:-1, 0]*sm.atoms_per_packet/(sm._volume*R_cm**3))
    assert np.array_equal(first.column_profile, direct[1][..., 1:-1, 0]*per_area)
    cell = np.zeros((3, 8, 6, 2))
    for k in range(6):
        cell = cell + direct[1][:, :, :, k]
    assert np.array_equal(first.column, cell[..., 0]*per_area)
    filled = cell[..., 1] != 0
    assert np.array_equal(first.column_effective_packets[filled], cell[..., 0][filled]**2/cell[..., 1][filled])
    assert np.array_equal(first.content, sm.atoms_per_packet*direct[0][..., 1:-1, 0].sum(axis=(1, 2, 3)))
    # at t = 100 s only the ages below 100 s count: planes 0 and 1 in full, plane 2 in part
    young = want.block[0, ..., 1:-1, :2, 0].sum()
    assert sm.atoms_per_packet*young <= first.content[1] < first.content[2] < sm.atoms_per_packet*want.block[0, ..., 1:-1, :, 0].sum()
    assert first.content[0] < first.content[1]
    emission = TransientShells(epochs, K, direct, sm.atoms_per_packet, sm.solid_angle, sm._volume,
                               R_cm, 'radiance')
    assert emission.content is None and np.array_equal(emission.density, first.density)
    # another product took the block: set up again, one upload, the same bits
    sets = ctx.sets
    ctx.ages_owner.pop('shell', None)
    again = sm.transient(epochs, history)
    assert ctx.sets == sets + 1 and ctx.uploads == uploads + 1
    assert np.array_equal(ctx._block, sm.shell_age_sums)
    assert np.array_equal(again.density, first.density) and np.array_equal(again.column, first.column)
    sm.transient(epochs, history)
    assert ctx.uploads == uploads + 1
    empty = _map([], context=object(), ages=AGES).transient(epochs, history)
    assert empty.density.shape == (3, 8, 6, 4) and not empty.density.any() and not empty.content.any()


def test_the_library_exports_the_new_entry_points():
    import ctypes as C

    from nexoclom_amd import hip_api
    from tests.test_abi import header_signatures
    header = header_signatures(open(HEADER).read())
    names = [f'nxc_shell_ages_{what}' for what in ENTRIES]
    for name in names:
        assert name in hip_api.EXPORTS and name in hip_api.SIGNATURES
        assert header[name] == (C.c_int, hip_api.SIGNATURES[name]), name
    assert len(hip_api.SIGNATURES['nxc_shell_ages_accumulate']) == 8          # h, p, six columns
    for what in ('enable', 'accumulate', 'download', 'upload', 'apply'):
        assert callable(getattr(hip_api.Context, f'shell_ages_{what}'))
    assert hip_api.ABI_VERSION == 3


@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_argument_check_as_a_host_program(tmp_path, flags):
    """nxc_shell_ages_enable's refusals are host-only code (nxc_ages_check.hpp);
    tests/tools/shell_ages_check.cpp feeds it good arguments, one bad set per refusal and
    R (na + 2) one below and at the 2^31 record limit.  Built plainly and with the host
    sanitizers; both runs must pass."""
    exe = tmp_path / 'shell_ages_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'shell_ages_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    lines = done.stdout.splitlines()
    assert sum(' refused: ' in line for line in lines) >= 21
    assert sum(line.endswith(' accepted') for line in lines) >= 8
    for word in ('na must be at least 1', 't0 must be finite', 'below a_hi', 'a_hi - a_lo',
                 'nlon * nlat * (nalt + 2) * (na + 2) must be below 2^31'):
        assert any(word in line for line in lines), word
    at = [line for line in lines if line.startswith('1 record, 2^31')]
    assert len(at) == 2 and at[0].endswith(' accepted') and ' refused: ' in at[1]
    assert not done.stderr.strip()
