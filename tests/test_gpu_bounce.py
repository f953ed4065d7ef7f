"""Surface re-emission (bounce_packet / bispev3 / apply_fate<BOUNCE>) on the GPU, one impact at a
time and through every kernel variant that carries BOUNCE.

Single impacts: gravity, radiation pressure and loss are off, so one step of integrate_const moves
a packet by h v and the state entering bounce_packet is chosen by the test: the state before the
step is corrected until the C oracle's rk5 step (bit-identical to the kernel's) lands on the wanted
doubles (frac goes through log and exp in the step: the golden rows carry 1, which it hands on
unchanged).  Record 1 is compared with the rows of the reference's own bouncepackets()
(tests/golden/g12_bounce.npz) where the step landed exactly, and with np_oracle.bounce_packets on
the state that did enter everywhere.

Tolerance.  Time, position after the move back to the surface (x + v t: IEEE operations only) and
frac with constant sticking are compared bit for bit.  Velocity and temperature-dependent frac go
through asin, sin, cos, atan2, exp and |.|^0.25 (sqrt(sqrt()) on the device): ``libm_rows``
re-runs the restatement with every one of those results moved one ulp up, one ulp down, and by
random signs, and takes the largest change per row, relative to the speed for the velocity
columns and to frac for frac.  One ulp of atan2 is not small: the impact longitude
(atan2 + 2 pi) % 2 pi is rounded to the doubles around 2.5 pi, 8.9e-16 apart, and an ulp of atan2
can move it by a whole one; cos(longitude) then changes by 8.9e-16 tan(longitude), and the
temperature and the sticking coefficient with it.  Only within four such doubles of a terminator
is atan2 left alone: there the longitude decides the day / night branch, which has to be the
reference's (those rows sit in the middle of their longitude's run of inputs, away from the
rounding tie, so that the last bit of atan2 does not decide it).  Measured on the CPU over the
random rows of the golden file, largest per column (LIBM_SPREAD; tests/test_bounce_cpu.py
re-measures it):
    position 0      velocity / speed 2.0e-15      frac (temperature dependent) 1.7e-14
(frac is the larger because 1 - stickcoef cancels where the coefficient is close to 1.)  The GPU
tolerance of a row is 4x the larger of that figure and the row's own spread (device routines are
documented to a few ulp, not to one).  The row's own spread matters where the operation itself
is ill-conditioned: cos(asin(z)) a few 1e-8 from a pole turns one ulp of asin into 1e-8 of
cos(lat), 2e-9 of the temperature excess.  Everywhere else the bound is 8e-15 for velocities and
6.8e-14 for frac, five to six orders below the 1e-8 of the whole-trajectory comparison in
test_gpu_api.py.
"""
import contextlib
import io
import os

import numpy as np
import pytest

from nexoclom_amd import hip_api
from oracle import np_oracle as O
from tests import bounce_cases as B
from tests import helpers as H

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LIBM_SPREAD = (0.0, 2.0e-15, 1.7e-14)           # position, velocity / speed, frac
STEP = 1.0
EDGE = 50.


# ---- the libm harness (CPU) ---------------------------------------------------------------------
class _PowNudged(np.ndarray):
    def __pow__(self, e):
        return self._nudge(np.asarray(self)**e)


class _NudgedNumpy:
    """numpy, except that the libm routines of bounce_packets return their result one ulp away."""

    def __init__(self, mode, rng):
        self.mode, self.rng = mode, rng

    def __getattr__(self, name):
        return getattr(np, name)

    def _nudge(self, v):
        v = np.asarray(v, dtype=np.float64)
        sign = self.mode if self.mode in (-1, 1) else self.rng.choice([-1., 1.], size=v.shape)
        return np.nextafter(v, sign*np.inf)

    def arcsin(self, x):
        return self._nudge(np.arcsin(x))

    def sin(self, x):
        return self._nudge(np.sin(x))

    def cos(self, x):
        return self._nudge(np.cos(x))

    def exp(self, x):
        return self._nudge(np.exp(x))

    def arctan2(self, y, x):
        a = np.arctan2(y, x)
        lon = (a + 2*np.pi) % (2*np.pi)
        branch = np.minimum(np.abs(lon - np.pi/2), np.abs(lon - 3*np.pi/2)) < 4*8.9e-16
        return np.where(branch, a, self._nudge(a))

    def abs(self, x):
        out = np.abs(x).view(_PowNudged)
        out._nudge = self._nudge
        return out


def libm_rows(X, cfg, ids, nb, hit=None, draws=6):
    """(n, 3): per row, the largest change of position (absolute), velocity (relative to the
    speed) and frac (relative) over the nudged runs of the restatement."""
    with np.errstate(all='ignore'):
        base = B.restate(X, cfg, ids, nb, hit)
        rng = np.random.default_rng(5)
        worst = np.zeros((len(base), 3))
        speed = np.linalg.norm(base[:, 4:7], axis=1)
        for mode in [1, -1] + [0]*draws:
            O.np = _NudgedNumpy(mode, rng)
            try:
                got = B.restate(X, cfg, ids, nb, hit)
            finally:
                O.np = np
            d = np.abs(got - base)
            vel = np.divide(d[:, 4:7].max(1), speed, out=np.zeros(len(base)), where=speed > 0)
            frac = np.divide(d[:, 7], base[:, 7], out=np.zeros(len(base)), where=base[:, 7] > 0)
            worst = np.maximum(worst, np.stack([d[:, 1:4].max(1), vel, frac], 1))
    return worst


def libm_spread(g, name):
    """Largest libm_rows figure per column over the random rows of golden case ``name``."""
    cfg = B.golden_config(g, name)
    rows = libm_rows(g[f'{name}_X'], cfg, g[f'{name}_ids'], g[f'{name}_nb'], g[f'{name}_hit'])
    return rows[g[f'{name}_edge'] == 0].max(0)


# ---- one impact on the GPU ----------------------------------------------------------------------
def free_flight(GM):
    return O.Forces(GM=GM, vrplanet=0.0, gravity=False, radpres=False, lifetime=0., photo=None,
                    v_tab=np.zeros(2), a_tab=np.zeros(2))


def after_fate(X, r0_before, outeredge=EDGE):
    X = X.copy()
    X[r0_before > outeredge, 7] = 0
    X[X[:, 7] < 1e-10, 7] = 0.
    X[X[:, 7] == 0, 0] = 0.
    return X


def single_impact(ctx, coracle, cfg, target, first_index=0):
    """One step that ends on ``target`` (n, 8) wherever the doubles allow.  Returns (entered,
    record1): the state that did enter apply_fate (the C oracle's step) and the GPU's record 1."""
    f = free_flight(cfg['GM'])
    pre = np.array(target, dtype=np.float64)
    pre[:, 0] += STEP
    pre[:, 1:4] -= STEP*target[:, 4:7]
    for _ in range(8):
        entered, _ = coracle.rk5(f, pre, STEP)
        miss = target[:, 1:4] - entered[:, 1:4]
        if not miss.any():
            break
        pre[:, 1:4] += miss
    entered, _ = coracle.rk5(f, pre, STEP)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(cfg)
    try:
        ctx.upload_packets(pre)
        ctx.set_first_index(first_index)
        traj = ctx.integrate_const(STEP, 1, EDGE, nrec=2)['traj']
        assert ctx.counters()['nonfinite'] == 0
    finally:
        ctx.set_bounce(None)
        ctx.set_first_index(0)
    assert np.array_equal(traj[:, 0, :].T, pre)
    return entered, np.ascontiguousarray(traj[:, 1, :].T)


def check_rows(got, want, spread, cfg, label):
    """``got`` against ``want`` at the module's tolerances; prints the figures first."""
    speed = np.linalg.norm(want[:, 4:7], axis=1)
    tol_v = 4*np.maximum(spread[:, 1], LIBM_SPREAD[1])
    tol_f = 4*np.maximum(spread[:, 2], LIBM_SPREAD[2]) if cfg['temp_dependent'] else np.zeros(len(got))
    dv = np.abs(got[:, 4:7] - want[:, 4:7]).max(1)
    rel_v = np.divide(dv, speed, out=np.zeros(len(got)), where=speed > 0)
    rel_f = np.divide(np.abs(got[:, 7] - want[:, 7]), want[:, 7], out=np.zeros(len(got)),
                      where=want[:, 7] > 0)
    print(f'{label}: {len(got)} rows, position differs on {int(np.any(got[:, :4] != want[:, :4], axis=1).sum())}, '
          f'velocity/speed max {rel_v.max():.3g} (largest bound {tol_v.max():.3g}, smallest '
          f'{tol_v.min():.3g}, worst ratio {np.max(rel_v/tol_v):.3g}), frac max {rel_f.max():.3g}')
    for k in np.nonzero(rel_v > tol_v)[0][:12]:
        print(f'  row {k}: longitude {np.arctan2(want[k, 1], -want[k, 2]) % (2*np.pi)!r}, z '
              f'{want[k, 3]!r}, velocity/speed off by {rel_v[k]:.3g} (bound {tol_v[k]:.3g})')
    assert np.array_equal(got[:, :4], want[:, :4]), label
    assert np.all(rel_v <= tol_v), (label, np.nonzero(rel_v > tol_v)[0][:10])
    assert np.all(dv[speed == 0] == 0)
    assert np.all(rel_f <= tol_f) and np.array_equal(got[:, 7] == 0, want[:, 7] == 0), label
    assert np.all(np.isfinite(got))


def check_against_restatement(ctx, coracle, cfg, target, first_index, label, expect_hits=64):
    entered, rec = single_impact(ctx, coracle, cfg, target, first_index)
    ids = np.uint64(first_index) + np.arange(len(target), dtype=np.uint64)
    nb = np.zeros(len(target), dtype=np.int64)
    r0 = np.sqrt((entered[:, 1]**2 + entered[:, 2]**2) + entered[:, 3]**2)
    hit = (r0 - 1.) < 0
    assert hit.sum() >= expect_hits and (~hit).sum() >= 8, (label, hit.sum())
    want = after_fate(B.restate(entered, cfg, ids, nb), r0)
    assert np.array_equal(rec[~hit], entered[~hit])          # the others just flew on
    check_rows(rec[hit], want[hit], libm_rows(entered, cfg, ids, nb)[hit], cfg, label)
    return entered, rec, want, hit


def with_bystanders(target):
    """Every third packet lifted above the surface: it does not impact."""
    target = np.array(target)
    target[2::3, 1:4] *= 1.3
    return target


@pytest.fixture(scope='module')
def golden():
    return np.load(B.GOLDEN, allow_pickle=False)


# ---- 2a: against the reference's rows -----------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', list(B.CASES))
def test_single_impacts_match_the_reference_rows(ctx, coracle, golden, name):
    g = golden
    cfg = B.golden_config(g, name)
    X, ids, nb, hit = (g[f'{name}_{k}'] for k in ('X', 'ids', 'nb', 'hit'))
    first = int(ids[0])
    assert np.array_equal(ids, np.uint64(first) + np.arange(len(ids), dtype=np.uint64))
    entered, rec = single_impact(ctx, coracle, cfg, X, first)
    assert np.array_equal(rec[~hit], entered[~hit])
    # rows whose entering state is the golden one to the bit and whose stored bounce number is
    # the launch's (0): the reference's own rows
    exact = hit & (nb == 0) & np.all(entered[:, 1:8] == X[:, 1:8], axis=1)
    # (a coordinate whose value before the step lies in the binade above moves on a grid twice as
    # coarse and reaches only every other double: some rows cannot be landed on)
    assert exact.sum() >= 0.75*(hit & (nb == 0)).sum(), (exact.sum(), (hit & (nb == 0)).sum())
    want = g[f'{name}_out'].copy()
    want[:, 0] = entered[:, 0]
    want = after_fate(want, g[f'{name}_r0'])
    spread = libm_rows(X, cfg, ids, nb, hit)
    check_rows(rec[exact], want[exact], spread[exact], cfg, f'{name} vs reference rows')
    for fam in range(1, len(g['edge_names'])):
        assert (exact & (g[f'{name}_edge'] == fam)).sum() >= 1, g['edge_names'][fam]
    # every row against the restatement at the state that did enter, bounce number 0
    zero = np.zeros(len(X), dtype=np.int64)
    rest = after_fate(B.restate(entered, cfg, ids, zero, hit), g[f'{name}_r0'])
    check_rows(rec[hit], rest[hit], libm_rows(entered, cfg, ids, zero, hit)[hit], cfg,
               f'{name} vs restatement')


# ---- 2b: edges against the restatement ----------------------------------------------------------
def family_rows(fam, unit_km, n_hits=66):
    rows = [r for r in B.edge_rows(unit_km) if r[0] == fam]
    n = 3*((n_hits*3//2)//3 + 1)
    X = np.zeros((n, 8))
    for i in range(n):
        X[i, 1:4], X[i, 4:7] = rows[i % len(rows)][1], rows[i % len(rows)][2]
    X[:, 0] = 500. + np.arange(n)
    X[:, 7] = np.linspace(0.2, 1.0, n)
    return with_bystanders(X)


@gpu
@pytest.mark.parametrize('fam', range(1, 10))
def test_edge_families(ctx, coracle, golden, fam):
    """Terminators, longitude 0, near the poles, grazing, clamped impact energy, sub-solar point,
    night side, outward-moving: each family of bounce_cases.edge_rows repeated over more than a
    wave (every packet its own uniforms), two of three packets impacting."""
    g = golden
    for name in ('const', 'tempdep', 'elastic_stick'):
        cfg = B.golden_config(g, name)
        check_against_restatement(ctx, coracle, cfg, family_rows(fam, cfg['unit_km']), 0,
                                  f"{g['edge_names'][fam]} / {name}")


def radial_impacts(n, seed, unit_km, day_only=False):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-1.4, 1.4, n) if day_only else rng.uniform(0, 2*np.pi, n)
    lat = np.arcsin(rng.uniform(-0.95, 0.95, n))
    p = np.stack([np.sin(lon)*np.cos(lat), -np.cos(lon)*np.cos(lat), np.sin(lat)], 1)
    X = np.zeros((n, 8))
    X[:, 0] = 700.
    X[:, 1:4] = p*(1 - 10**rng.uniform(-6, -2, n))[:, None]
    X[:, 4:7] = -p*(rng.uniform(0.5, 3.0, n)/unit_km)[:, None]
    X[:, 7] = rng.uniform(0.1, 1.0, n)
    return X


@gpu
def test_temperature_and_probability_on_spline_knots(ctx, coracle, golden):
    """T equal to tx[3] (night side), tx[nx-4] (sub-solar point) and to interior knots, p in the
    first and last knot interval: a spline whose temperature grid is made of the impacts' own
    temperatures."""
    from scipy import interpolate
    g = golden
    GM, unit_km = float(g['GM']), float(g['unit_km'])
    base = B.config(1.3, 0.5, 1, 0.0, B.DEFAULT_A, GM, unit_km, 5)
    X = radial_impacts(150, 3, unit_km, day_only=True)
    X[100:120] = radial_impacts(20, 4, unit_km)[:, :]                       # some on the night side
    X[120:126, 1:4] = [0.0, -(1 - 1e-4), 0.0]
    X[120:126, 4:7] = [0.0, 1.5/unit_km, 0.0]                               # sub-solar
    X = with_bystanders(X)
    seen = []
    probe = dict(base, surf=type('S', (), {'v_interp': staticmethod(
        lambda T, p: (seen.append(np.array(T)), np.ones_like(T))[1])})())
    ids = np.arange(len(X), dtype=np.uint64)
    B.restate(X, probe, ids, np.zeros(len(X), dtype=np.int64))
    T = np.unique(seen[0])
    grid = np.unique(np.concatenate([[base['t0'], base['t0'] + base['t1']], T[::3],
                                     np.linspace(base['t0'], base['t0'] + base['t1'], 12)]))
    grid = grid[np.concatenate([[True], np.diff(grid) > 1e-3])]
    pgrid = np.linspace(0, 1, 21)
    values = np.sqrt(grid)[:, None]*(0.02 + 0.1*pgrid[None, :]**1.5)        # km/s, smooth
    spline = interpolate.RectBivariateSpline(grid, pgrid, values)
    cfg = B.config(1.3, 0.5, 1, 0.0, B.DEFAULT_A, GM, unit_km, 5, spline=spline)
    entered, rec, want, hit = check_against_restatement(ctx, coracle, cfg, X, 0, 'spline knots')
    seen.clear()
    B.restate(entered, dict(probe, tx=cfg['tx']), ids, np.zeros(len(X), dtype=np.int64))
    T = seen[0]
    tx = cfg['tx']
    assert (T == tx[3]).sum() >= 3 and (T == tx[-4]).sum() >= 3
    assert np.isin(T, tx[4:-4]).sum() >= 10
    p = B.uniforms(ids[hit], np.zeros(hit.sum(), dtype=np.int64), 5)[2]
    assert (p < cfg['ty'][4]).sum() >= 1 and (p >= cfg['ty'][-5]).sum() >= 1


@gpu
@pytest.mark.parametrize('A,what', [((0., 0., 1.5), 'above 1'), ((0., 0., -0.2), 'below 0'),
                                    ((0., 0., 0.), 'exactly 0'), ((0., 0., 1.), 'exactly 1'),
                                    ((2.0, -0.004, -0.3), 'both clamps over the surface')])
def test_sticking_clamps(ctx, coracle, golden, A, what):
    g = golden
    cfg = B.config(1.3, 0.2, 1, 0.0, A, float(g['GM']), float(g['unit_km']), 9)
    X = with_bystanders(radial_impacts(120, 8, cfg['unit_km']))
    entered, rec, want, hit = check_against_restatement(ctx, coracle, cfg, X, 0, f'sticking {what}')
    f_in, f_out = entered[hit, 7], rec[hit, 7]
    if what in ('above 1', 'exactly 1'):
        assert np.all(f_out == 0) and np.all(rec[hit, 0] == 0)
    elif what in ('below 0', 'exactly 0'):
        assert np.array_equal(f_out, f_in)
    else:
        assert (f_out == 0).sum() > 5 and (f_out == f_in).sum() > 5 and \
            ((f_out > 0) & (f_out < f_in)).sum() > 5


@gpu
def test_frac_either_side_of_the_threshold(ctx, coracle, golden):
    """frac (1 - stickcoef) just under and just over 1e-10: dead with its time zeroed, or alive."""
    g = golden
    cfg = B.golden_config(g, 'const')
    X = with_bystanders(radial_impacts(150, 2, cfg['unit_km']))
    X[:, 7] = (1e-10/0.7)*(1 + np.linspace(-12, 12, len(X))*2.2e-16)
    X[2::3, 7] = 0.5
    entered, rec, want, hit = check_against_restatement(ctx, coracle, cfg, X, 0, 'frac threshold')
    dead = rec[:, 7] == 0
    assert 10 < dead[hit].sum() < hit.sum() - 10 and np.all(rec[dead, 0] == 0)
    assert np.all(rec[~dead, 0] == entered[~dead, 0]) and np.all(rec[hit & ~dead, 7] >= 1e-10)


@gpu
@pytest.mark.parametrize('first', [0, 2**32 - 1, 2**32 - 40, 2**32, 2**33 + 5])
def test_first_index_reaches_both_counter_words(ctx, coracle, golden, first):
    g = golden
    cfg = B.golden_config(g, 'tempdep')
    X = with_bystanders(radial_impacts(120, 6, cfg['unit_km']))
    entered, rec, want, hit = check_against_restatement(ctx, coracle, cfg, X, first, f'first_index {first}')
    if first:                               # and the draws are not those of first_index 0
        other = B.restate(entered, cfg, np.arange(len(X), dtype=np.uint64), np.zeros(len(X), dtype=np.int64))
        assert np.all(np.any(other[hit, 4:7] != want[hit, 4:7], axis=1))


@gpu
def test_fifty_bounces_in_fifty_steps(ctx, golden):
    """Gravity strong enough to bring every packet back within a step: 50 impacts per packet, each
    with its own Philox block.  Each impact puts the packet back on the surface and re-draws its
    direction, and only (1 - accomfactor) = 1/2 of the impact energy is carried over, so the
    differences between the device's and glibc's routines do not compound: the bound is a small
    multiple of a single impact's 8e-15 -- 1e-12 here, with the clamped impact energy
    (v_old2 = a + PE close to 0, absolute differences of 1e-16 relative to nothing) under atol."""
    g = golden
    GM, unit_km = -5e-4, float(g['unit_km'])
    cfg = B.config(0.5, 0.5, 0, 0.3, (0., 0., 0.), GM, unit_km, 21)
    f = O.Forces(GM=GM, vrplanet=0.0, gravity=True, radpres=False, lifetime=0., photo=None,
                 v_tab=np.zeros(2), a_tab=np.zeros(2))
    n, step, n_iter = 96, 30., 50
    X0 = radial_impacts(n, 13, unit_km)
    X0[:, 1:4] *= (1.0001/np.linalg.norm(X0[:, 1:4], axis=1))[:, None]
    X0[:, 4:7] = 0.0
    X0[:, 0], X0[:, 7] = step*n_iter, 1.0
    first = 2**32 - 48
    res, nb, work = O.constant_step_driver_bounce(f, X0, step*n_iter, step, 15., cfg, first_index=first)
    assert np.all(nb == n_iter) and work == n*n_iter
    u = np.stack([B.uniforms(np.full(n_iter, first + 3, dtype=np.uint64), np.arange(n_iter), 21)])
    assert len(np.unique(u[0, 0])) == n_iter and len(np.unique(u[0, 2])) == n_iter
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(cfg)
    try:
        ctx.upload_packets(X0)
        ctx.set_first_index(first)
        traj = ctx.integrate_const(step, n_iter, 15., nrec=n_iter + 1)['traj']
        ctr = ctx.counters()
    finally:
        ctx.set_bounce(None)
        ctx.set_first_index(0)
    got = np.transpose(traj, (2, 0, 1))                       # (n, 8, nrec)
    err = np.abs(got - res)/np.maximum(np.abs(res), 1e-300)
    print('fifty bounces: largest relative difference', err[np.abs(res) > 1e-9].max())
    assert ctr['particle_steps'] == work and ctr['nonfinite'] == 0
    np.testing.assert_allclose(got, res, rtol=1e-12, atol=1e-15)
    # frac = 0.7^k, but through log and exp in every step (rk5.py): a last bit of log(frac), up
    # to 18 in size, is 2e-15 of frac, fifty times over
    np.testing.assert_allclose(got[:, 7], res[:, 7], rtol=1e-13, atol=0)
    r = np.sqrt(np.sum(got[:, 1:4, 1:]**2, axis=1))
    np.testing.assert_allclose(r, 1.0, rtol=0, atol=1e-15)    # every record is an impact point


@gpu
def test_bounce_in_the_step_before_escape(ctx, golden):
    """Impact and escape cannot coincide (outeredge > 1): packets that re-emit and then leave."""
    g = golden
    cfg = B.golden_config(g, 'elastic')
    f = free_flight(cfg['GM'])
    n, step, n_iter = 96, 30., 60
    X0 = radial_impacts(n, 17, cfg['unit_km'])
    X0[:, 1:4] *= (1.004/np.linalg.norm(X0[:, 1:4], axis=1))[:, None]
    X0[:, 4:7] *= (2.0/cfg['unit_km']/np.linalg.norm(X0[:, 4:7], axis=1))[:, None]
    X0[:, 0] = step*n_iter
    res, nb, work = O.constant_step_driver_bounce(f, X0, step*n_iter, step, 1.03, cfg)
    assert np.all(nb == 1) and np.all(res[:, 7, -1] == 0)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(cfg)
    try:
        ctx.upload_packets(X0)
        ctx.set_first_index(0)
        out = ctx.integrate_const(step, n_iter, 1.03, want_final=True, want_steps=True)
        ctr = ctx.counters()
    finally:
        ctx.set_bounce(None)
    life = (res[:, 7, :] > 0).sum(1)                           # records alive = steps taken
    assert np.array_equal(out['steps'], life) and ctr['particle_steps'] == work
    assert life.min() >= 2 and len(np.unique(life)) > 3
    last = res[np.arange(n), :, life]
    assert np.all(out['final'][:, 7] == 0) and np.all(out['final'][:, 0] == 0)
    np.testing.assert_allclose(out['final'], last, rtol=1e-13, atol=0)


# ---- 2c: impacts without a finite re-emission ---------------------------------------------------
@gpu
def test_polar_and_resting_impacts_are_absorbed_and_counted(ctx, coracle, golden):
    """Exactly on the polar axis (east vector 0/0) and at rest inside the planet (move-back 0/0)
    the reference asserts.  Contract here: the launch returns, the packet is absorbed where it is
    (frac = 0, time = 0, finite state), nxc_counters.nonfinite counts it, its neighbours in the
    wave are what they are without it, and nothing non-finite reaches the image."""
    g = golden
    cfg = B.golden_config(g, 'tempdep')
    f = free_flight(cfg['GM'])
    v = 1.5/cfg['unit_km']
    X = with_bystanders(radial_impacts(128, 23, cfg['unit_km']))
    X[:, 0] = 700.
    bad = np.array([4, 67, 9, 100])
    clean = X.copy()
    X[4, 1:7] = [0., 0., 1 - 1e-3 + STEP*v, 0., 0., -v]
    X[67, 1:7] = [0., 0., -(1 - 1e-5) - STEP*v, 0., 0., v]
    X[9, 1:7] = [0.3, 0.4, 0.5, 0., 0., 0.]
    X[100, 1:7] = [0., 0., 0.99, 0., 0., 0.]
    clean[bad, 1:4] *= 3.0
    im = H.image_setup(H.mercury_forces('Na', 1.3), 'column', dims=(32, 32), width=(4., 4.))
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(cfg)
    try:
        runs = {}
        for key, packets in (('bad', X), ('clean', clean)):
            ctx.upload_packets(packets)
            ctx.set_first_index(0)
            traj = ctx.integrate_const(STEP, 1, EDGE, nrec=2)['traj']
            dense_ctr = ctx.counters()
            ctx.upload_packets(packets)
            fin = ctx.integrate_const(STEP, 1, EDGE, want_final=True, want_steps=True)
            fin_ctr = ctx.counters()
            ctx.set_image(im['M'], 0.0, im['apix'], 'column', im['xedges'], im['zedges'], [])
            ctx.upload_packets(packets)
            ctx.integrate_const(STEP, 1, EDGE, image=True)
            img_ctr = ctx.counters()
            runs[key] = (traj, dense_ctr, fin, fin_ctr, ctx.image_download(), img_ctr)
    finally:
        ctx.set_bounce(None)
    traj, dense_ctr, fin, fin_ctr, (image, counts), img_ctr = runs['bad']
    ctraj, cdense, cfin, cfin_ctr, (cimage, ccounts), cimg_ctr = runs['clean']
    assert dense_ctr['nonfinite'] == fin_ctr['nonfinite'] == img_ctr['nonfinite'] == len(bad)
    assert cdense['nonfinite'] == cfin_ctr['nonfinite'] == cimg_ctr['nonfinite'] == 0
    rec = traj[:, 1, :].T
    assert np.all(np.isfinite(traj)) and np.all(np.isfinite(fin['final'])) and np.all(np.isfinite(image))
    assert np.all(rec[bad, 7] == 0) and np.all(rec[bad, 0] == 0)
    entered, _ = coracle.rk5(f, X, STEP)
    assert np.array_equal(rec[bad, 1:7], entered[bad, 1:7])          # absorbed where it was
    assert np.array_equal(fin['final'], rec) and np.all(fin['steps'] == 1)
    others = np.setdiff1d(np.arange(len(X)), bad)
    assert np.array_equal(traj[:, :, others], ctraj[:, :, others])
    assert np.array_equal(fin['final'][others], cfin['final'][others])
    assert counts.sum() > 100 and img_ctr['samples'] == cimg_ctr['samples'] - len(bad)
    # the Python drivers raise on the counter, as they do for the others
    from nexoclom_amd.Output import Output
    with pytest.raises(AssertionError):
        Output._raise_on_counters(type('Bare', (), {})(), dict(nonfinite=1))


# ---- 3: every kernel variant that carries BOUNCE ------------------------------------------------
def low_and_slow(name, g, n=3000):
    taa = B.CASES[name][0]
    f = H.mercury_forces('Na', taa, True, name != 'const', 0.0)
    cfg = B.config(*B.CASES[name], f.GM, f.R_km, 41)
    endtime, step = 3600., 30.
    X0 = H.sample_x0(n, 19, endtime, vprob=1.2, delv=0.8, R_km=f.R_km)
    nsteps, n_iter = O.n_output_steps(endtime, step)
    return dict(f=f, cfg=cfg, X0=X0, step=step, n_iter=n_iter, nsteps=nsteps, edge=15., n=n,
                endtime=endtime)


@pytest.fixture(scope='module', params=['tempdep', 'const'])
def bouncing(request, ctx, golden):
    """A few thousand packets launched low and slow (most bounce several times), their dense
    trajectory from the GPU and the restatement's bookkeeping."""
    c = low_and_slow(request.param, golden)
    H.set_ctx_forces(ctx, c['f'])
    ctx.set_bounce(c['cfg'])
    try:
        ctx.upload_packets(c['X0'])
        ctx.set_first_index(0)
        c['dense'] = ctx.integrate_const(c['step'], c['n_iter'], c['edge'], nrec=c['nsteps'])['traj']
    finally:
        ctx.set_bounce(None)
    return c


def run_with_bounce(ctx, c, call):
    H.set_ctx_forces(ctx, c['f'])
    ctx.set_bounce(c['cfg'])
    try:
        ctx.upload_packets(c['X0'])
        ctx.set_first_index(0)
        return call()
    finally:
        ctx.set_bounce(None)


@gpu
def test_trajectory_finals_and_rows_are_the_same_arithmetic(ctx, bouncing):
    c = bouncing
    dense = c['dense']
    frac = dense[7].T
    live = frac > 0
    _, nb, work = O.constant_step_driver_bounce(c['f'], c['X0'], c['endtime'], c['step'], c['edge'],
                                                c['cfg'])
    assert (nb >= 3).mean() > 0.2 and nb.max() >= 5       # (cold ground keeps what lands on it)
    fin = run_with_bounce(ctx, c, lambda: ctx.integrate_const(
        c['step'], c['n_iter'], c['edge'], want_final=True, want_steps=True))
    assert ctx.counters()['particle_steps'] == work and ctx.counters()['nonfinite'] == 0
    last = np.minimum(fin['steps'], c['nsteps'] - 1)
    assert np.array_equal(fin['final'], np.transpose(dense, (2, 0, 1))[np.arange(c['n']), :, last])
    wide = run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(c['step'], c['n_iter'], c['edge']))
    assert ctx.counters()['unfinished'] == 0
    assert np.array_equal(wide['lengths'], live.sum(1))
    for col in range(8):
        assert np.array_equal(wide['rows'][col], dense[col].T[live])
    lossfrac = np.zeros_like(frac)
    for ct in range(1, c['nsteps']):
        act = frac[:, ct-1] > 0
        lossfrac[act, ct] = (lossfrac[act, ct-1] + frac[act, ct-1]) - frac[act, ct]
    assert np.array_equal(wide['rows'][8], lossfrac[live])
    narrow = run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(
        c['step'], c['n_iter'], c['edge'], narrow=True))
    assert np.array_equal(narrow['rows'], wide['rows'].astype(np.float32))
    res = run_with_bounce(ctx, c, lambda: ctx.integrate_const_rows(
        c['step'], c['n_iter'], c['edge'], resident=True))
    try:
        rows, index = res['store'].download()
        assert np.array_equal(rows, wide['rows'])
        assert np.array_equal(index, np.repeat(np.arange(c['n']), wide['lengths']))
    finally:
        res['store'].free()


@gpu
@pytest.mark.parametrize('quantity', ['radiance', 'column'])
@pytest.mark.parametrize('downcast', [False, True])
def test_fused_image_with_bounce(ctx, bouncing, quantity, downcast):
    """k_const_fused<IMAGE = 1 | 2, BOUNCE = true>: the image of the fused pass against
    nxc_image_accumulate over the frac > 0 records of the GPU's own dense trajectory."""
    c = bouncing
    f = c['f']
    im = H.image_setup(f, quantity, dims=(48, 48), width=(6., 6.))
    args = (im['M'], f.vrplanet, im['apix'], quantity, im['xedges'], im['zedges'], im['g_tables'])

    def fused():
        ctx.set_image(*args, downcast_f32=downcast)
        ctx.integrate_const(c['step'], c['n_iter'], c['edge'], image=True)
        return ctx.image_download(), ctx.counters()
    (image, counts), ctr = run_with_bounce(ctx, c, fused)
    live = c['dense'][7] > 0                                   # (nsteps, n)
    cols = [np.ascontiguousarray(c['dense'][k][live]) for k in (1, 2, 3, 5, 7)]
    if downcast:
        cols = [col.astype(np.float32).astype(np.float64) for col in cols]
    ctx.set_image(*args, downcast_f32=False)
    ctx.image_accumulate(*cols)
    image2, counts2 = ctx.image_download()
    assert ctr['samples'] == live.sum() and ctr['nonfinite'] == 0 and counts.sum() > 10000
    assert np.array_equal(counts, counts2)
    np.testing.assert_allclose(image, image2, rtol=1e-11, atol=0)


@gpu
@pytest.mark.parametrize('infile', ['Bounce.const.input', 'Bounce.tempdep.input'])
def test_streaming_model_image_with_bounce(ctx, infile):
    from nexoclom_amd import Input, ModelImage
    params = {'quantity': 'column', 'dims': '40,40', 'width': '6,6'}
    with contextlib.redirect_stdout(io.StringIO()):
        inputs = Input(os.path.join(HERE, 'inputfiles', infile))
        inputs.run(3000, packs_per_it=3000, seed=37, context=ctx)
        stored = inputs.produce_image(params, context=ctx)
        streamed = ModelImage(inputs, params, npackets=3000, packs_per_it=3000, seed=37, context=ctx)
    ctx.set_bounce(None)
    assert stored.packet_image.sum() > 10000
    assert np.array_equal(streamed.packet_image, stored.packet_image)
    np.testing.assert_allclose(streamed.image, stored.image, rtol=1e-11, atol=0)


@gpu
def test_order_of_set_up_calls_and_clearing(ctx, coracle, bouncing):
    """set_bounce before set_forces, between set_forces and set_image, after both: identical
    finals; set_bounce(None) afterwards restores bit parity with the C oracle."""
    c = bouncing
    f = c['f']
    im = H.image_setup(f, 'column', dims=(16, 16))
    X0 = c['X0'][:1024]

    def forces():
        H.set_ctx_forces(ctx, f)

    def image():
        ctx.set_image(im['M'], f.vrplanet, im['apix'], 'column', im['xedges'], im['zedges'], [])

    def bounce():
        ctx.set_bounce(c['cfg'])
    finals = []
    try:
        for order in ((bounce, forces, image), (forces, bounce, image), (forces, image, bounce)):
            ctx.set_bounce(None)
            for call in order:
                call()
            ctx.upload_packets(X0)
            ctx.set_first_index(0)
            finals.append(ctx.integrate_const(c['step'], c['n_iter'], c['edge'], want_final=True)['final'])
    finally:
        ctx.set_bounce(None)
    assert np.array_equal(finals[0], finals[1]) and np.array_equal(finals[0], finals[2])
    ctx.upload_packets(X0)
    plain = ctx.integrate_const(c['step'], c['n_iter'], c['edge'], want_final=True, want_steps=True)
    ref = coracle.integrate_const(f, X0, c['step'], c['n_iter'], c['edge'], threads=4)
    assert np.array_equal(plain['final'], ref['final']) and np.array_equal(plain['steps'], ref['steps'])
    assert not np.array_equal(plain['final'], finals[0])


# ---- 4: refusals at the C ABI -------------------------------------------------------------------
@gpu
def test_bounce_refusals_leave_the_context_usable(ctx, coracle, golden):
    g = golden
    f = H.mercury_forces('Na', 1.3)
    good = B.config(*B.CASES['tempdep'], f.GM, f.R_km, 3)
    tx, ty, coef = good['tx'], good['ty'], good['coef']

    def changed(a, k, value):
        a = a.copy()
        a[k] = value
        return a

    bad = {
        'nan coefficient': dict(good, coef=changed(coef, (3, 4), np.nan)),
        'inf coefficient': dict(good, coef=changed(coef, (0, 0), np.inf)),
        'decreasing tx': dict(good, tx=changed(tx, 50, tx[49] - 1.0)),
        'repeated interior ty': dict(good, ty=changed(ty, 50, ty[49])),
        'nan knot': dict(good, tx=changed(tx, 0, np.nan)),
        'too few knots': dict(good, tx=tx[:7], coef=coef[:3]),
        'dummy tables with accommodation': dict(good, tx=np.zeros(8), ty=np.zeros(8),
                                                coef=np.zeros((4, 4))),
    }
    X0 = H.sample_x0(2000, 3, 3000.)
    H.set_ctx_forces(ctx, f)
    ctx.set_bounce(None)
    try:
        for what, cfg in bad.items():
            with pytest.raises(hip_api.HipError) as err:
                ctx.set_bounce(cfg)
                pytest.fail(f'{what}: accepted')
            assert err.value.code == hip_api.NXC_ERR_ARG, what
        # a refused description changes nothing: still perfect sticking, bit-equal to the oracle
        ctx.upload_packets(X0)
        plain = ctx.integrate_const(30., 100, 15., want_final=True)
        ref = coracle.integrate_const(f, X0, 30., 100, 15., threads=4)
        assert np.array_equal(plain['final'], ref['final'])
        # without accommodation the zero-filled dummy tables stay accepted
        elastic = B.config(*B.CASES['elastic_stick'], f.GM, f.R_km, 3)
        assert not elastic['tx'].any()
        ctx.set_bounce(elastic)
        ctx.set_bounce(good)
        # the adaptive driver has no re-emission: it refuses, and the handle goes on working
        ctx.upload_packets(X0)
        with pytest.raises(hip_api.HipError) as err:
            ctx.integrate_var(1e-4, 15.)
        assert err.value.code == hip_api.NXC_ERR_STATE
        # so does the streamed pass ...
        with pytest.raises(hip_api.HipError) as err:
            ctx.integrate_const_streamed(np.ascontiguousarray(X0.T), 30., 100, 15., image=False)
            ctx.synchronize()
        assert err.value.code == hip_api.NXC_ERR_STATE
        # ... and moons together with re-emission
        ctx.upload_packets(X0)
        ctx.set_bodies(dict(moons=[dict(gm=f.GM*1e-3, radius=0.1, a=5.0, omega=1e-4, phi=0.0)], t0=0.0))
        with pytest.raises(hip_api.HipError) as err:
            ctx.integrate_const(30., 10, 15., want_final=True)
        assert err.value.code == hip_api.NXC_ERR_STATE
        ctx.set_bodies(None)
        ctx.upload_packets(X0)
        bounced = ctx.integrate_const(30., 100, 15., want_final=True)['final']
        assert np.all(np.isfinite(bounced)) and not np.array_equal(bounced, ref['final'])
        ctx.set_bounce(None)
        ctx.upload_packets(X0)
        final, hs = ctx.integrate_var(1e-4, 15.)
        assert np.all(np.isfinite(final))
    finally:
        ctx.set_bounce(None)
        ctx.set_bodies(None)
