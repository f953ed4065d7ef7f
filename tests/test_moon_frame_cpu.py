"""The moon-centred frame without a GPU: the restatement (tests/moon_frame_restatement.py) against
the definition's own consequences and against an oracle run from Io, MoonFrame.from_inputs, what
the products refuse and what they hand a (fake) context with a moon origin, the slabs of
sample_pass, the host-only argument check as a stand-alone program, and the ABI."""
import contextlib
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import nexoclom_amd
from nexoclom_amd import Input, hip_api
from nexoclom_amd.Output import Output
from nexoclom_amd.frames import MoonFrame
from oracle import np_oracle as O
from tests import moon_frame_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles')
IO_INPUT = os.path.join(FILES, 'Na.io.torus.input')
MERCURY_INPUT = os.path.join(FILES, 'Na.mercury.bench.input')
# Io around Jupiter in Jupiter radii, roughly; the tests of the restatement need no more
IO = dict(rad=0.0255, a=5.9, omega=4.11e-5, phi=1.0)


def io_inputs(endtime=6000., vprob=None, delv=None):
    inputs = Input(IO_INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(endtime, 's')
    if vprob is not None:          # launch speeds below Io's escape speed
        inputs.speeddist.vprob = type(inputs.speeddist.vprob)(vprob, 'km/s')
        inputs.speeddist.delv = type(inputs.speeddist.delv)(delv, 'km/s')
    return inputs


def cloud(n, seed, dtype=np.float64, t_max=2e5):
    rng = np.random.default_rng(seed)
    cols = [rng.uniform(0, t_max, n)] + [rng.uniform(-7, 7, n) for _ in range(3)] + \
           [rng.uniform(-3e-4, 3e-4, n) for _ in range(3)]
    return [c.astype(dtype) for c in cols]


# ---- 1. the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_identity_returns_the_input(dtype):
    cols = cloud(1000, 1, dtype)
    got = R.move_rows(R.IDENTITY, *cols)
    assert got.dtype == dtype
    for k in range(6):
        assert np.array_equal(got[k], cols[k + 1])


def test_a_point_that_stands_still_in_the_moons_frame():
    """Rows of one co-rotating point over three orbits all map to that point."""
    frame = R.moon_frame(**IO)
    d, u = np.array([1.3, -0.4, 0.7]), np.array([2e-4, -5e-4, 1e-4])       # moon radii (per s)
    t = np.linspace(0, 3*2*np.pi/IO['omega'], 4001)
    cols = R.corotating_rows(IO['a'], IO['omega'], IO['phi'], IO['rad'], d, u, t)
    assert frame.omega*t[-1] > 6*np.pi - 1e-9
    got = R.move_rows(frame, *cols)
    pos, vel = R.bounds(frame, cols[1], cols[2], cols[4], cols[5])
    worst = 0.0
    for k in range(2):
        worst = max(worst, np.max(np.abs(got[k] - d[k])/pos), np.max(np.abs(got[3 + k] - u[k])/vel))
    print(f'worst error / bound {worst:.3f}')
    for k in range(2):
        assert np.all(np.abs(got[k] - d[k]) <= pos)
        assert np.all(np.abs(got[3 + k] - u[k]) <= vel)
    np.testing.assert_allclose(got[2], d[2], rtol=4e-16, atol=0)
    np.testing.assert_allclose(got[5], u[2], rtol=4e-16, atol=0)
    # and the point moves with the moon: its distance from the moon of each row's time is |d|
    moon, _ = R.moon_at(IO['a'], IO['omega'], IO['phi'], t)
    dist = np.linalg.norm(np.stack(cols[1:4], -1) - moon, axis=1)/IO['rad']
    np.testing.assert_allclose(dist, np.linalg.norm(d), rtol=1e-11)


def test_an_epoch_row_is_shifted_and_scaled():
    frame = R.moon_frame(**IO)
    _, x, y, z, vx, vy, vz = cloud(100, 2)
    got = R.move_rows(frame, np.zeros(100), x, y, z, vx, vy, vz)
    want = [(x - frame.M[0])*frame.scale, (y - frame.M[1])*frame.scale, z*frame.scale,
            (vx - frame.U[0])*frame.scale, (vy - frame.U[1])*frame.scale, vz*frame.scale]
    for k in range(6):
        assert np.array_equal(got[k], want[k])


def oracle_rows(inputs, npackets, seed):
    """(out, rows (n, 8) with frac > 0, launch rows (npackets, 8)) of the NumPy oracle's
    constant-step run of ``inputs`` with moons."""
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, npackets, seed=seed, integrate=False, save=False)
    bd = out._bodies
    moons = bd['moons']
    b = O.Bodies(**{key: tuple(m[key] for m in moons) for key in ('gm', 'radius', 'a', 'omega', 'phi')},
                 t0=bd['t0'], chx_on=True, chx_k0=bd['chx']['k0'], chx_rho0=bd['chx']['rho0'],
                 chx_width=bd['chx']['width'], chx_height=bd['chx']['height'],
                 chx_omega=bd['chx']['omega'])
    kw = out.forces_kwargs()
    f = O.Forces(GM=kw['GM'], vrplanet=kw['vrplanet'], gravity=kw['gravity'], radpres=kw['radpres'],
                 lifetime=kw['lifetime'], photo=kw['photo'], v_tab=kw['v_tab'], a_tab=kw['a_tab'])
    X0 = out.X0[['time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac']].values
    opt = inputs.options
    res, _ = O.constant_step_driver_bodies(f, b, X0, opt.endtime.value, float(opt.step_size),
                                           opt.outeredge)
    rows = res.transpose(0, 2, 1).reshape(-1, 8)
    return out, rows[rows[:, 7] > 0], res[:, :, 0]


def test_the_rows_of_a_run_from_io_stay_at_io():
    """The physical pin.  Packets launched from Io's exobase below its escape speed (0.8 - 1.2
    km/s) stay bound to Io: in Io's frame every launch row lies at 1.3 R_Io and every stored row
    within [1, 2] R_Io (energy alone bounds 1.2 km/s at 1.82 R_Io), while the same rows read in the
    planet's frame at the epoch lie tens of Io radii from Io -- and with the rotation's sign
    reversed further still."""
    inputs = io_inputs(6000., vprob=1.0, delv=0.2)
    out, rows, launch = oracle_rows(inputs, 200, 5)
    io_moon = out._bodies['moons'][0]
    frame = R.moon_frame(io_moon['radius'], io_moon['a'], io_moon['omega'], io_moon['phi'])
    assert len(rows) > 5000
    at_launch = R.move_rows(frame, *launch[:, :7].T)
    np.testing.assert_allclose(np.linalg.norm(at_launch[:3], axis=0), 1.3, rtol=1e-9)
    r = np.linalg.norm(R.move_rows(frame, *rows[:, :7].T)[:3], axis=0)
    print(f'{len(rows)} rows, {r.min():.4f} .. {r.max():.4f} R_Io from Io in its frame')
    assert 1.0 <= r.min() and r.max() <= 2.0
    still = R.Frame(0.0, frame.M, frame.U, frame.scale)
    unmoved = np.linalg.norm(R.move_rows(still, *rows[:, :7].T)[:3], axis=0)
    assert unmoved.min() > 20
    wrong = R.Frame(-frame.omega, frame.M, frame.U, frame.scale)
    assert np.linalg.norm(R.move_rows(wrong, *rows[:, :7].T)[:3], axis=0).min() > 40


# ---- 2. MoonFrame.from_inputs -----------------------------------------------------------------------
def test_moon_frame_from_inputs():
    inputs = io_inputs()
    by_name = MoonFrame.from_inputs(inputs, 'Io')
    io_body = next(m for m in inputs.geometry.planet.moons if m.object == 'Io')
    by_object = MoonFrame.from_inputs(inputs, io_body)
    for frame in (by_name, by_object, MoonFrame.from_inputs(inputs, ' io ')):
        assert frame.origin == io_body and frame.unit == 'R_Io'
        assert frame.unit_km == io_body.radius.value
        assert np.array_equal(frame.M, by_name.M) and np.array_equal(frame.U, by_name.U)
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, 50, seed=3, integrate=False, save=False)
    moon = out._bodies['moons'][0]
    want = R.moon_frame(moon['radius'], moon['a'], moon['omega'], moon['phi'])
    assert by_name.omega == want.omega and by_name.scale == want.scale
    assert np.array_equal(by_name.M, want.M) and np.array_equal(by_name.U, want.U)
    jupiter_km = inputs.geometry.planet.radius.value
    assert by_name.radvel_shift_kms == want.U[1]*jupiter_km
    # against _launch_from_moon at t = 0: a packet at the moon's centre, at rest on it
    out.X0 = {key: np.zeros(1) for key in ('time', 'x', 'y', 'z', 'vx', 'vy', 'vz')}
    out._launch_from_moon()
    np.testing.assert_allclose([out.X0['x'][0], out.X0['y'][0]], by_name.M[:2], rtol=1e-15)
    np.testing.assert_allclose([out.X0['vx'][0], out.X0['vy'][0]], by_name.U[:2], rtol=1e-15)
    europa = MoonFrame.from_inputs(inputs, 'Europa')
    assert europa.unit == 'R_Europa' and europa.omega < by_name.omega
    np.testing.assert_allclose(np.hypot(*europa.M[:2])*jupiter_km, 671100, rtol=2e-3)


def test_moon_frame_refuses_what_is_not_a_moon_of_the_run():
    inputs = io_inputs()
    for origin in ('Ganymede', 'Jupiter', inputs.geometry.planet, 'Mercury'):
        with pytest.raises(ValueError, match='not a moon'):
            MoonFrame.from_inputs(inputs, origin)
    mercury = Input(MERCURY_INPUT)
    for origin in ('Mercury', 'Io'):
        with pytest.raises(ValueError, match='not a moon'):
            MoonFrame.from_inputs(mercury, origin)


def test_the_moon_table_is_what_the_run_integrates_with():
    from nexoclom_amd.frames import moon_table
    inputs = io_inputs()
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, 10, seed=3, integrate=False, save=False)
    assert out._bodies['moons'] == moon_table(inputs.geometry, out.unit_km)
    assert [m['phi'] for m in out._bodies['moons']] == [1.0, 4.0]


# ---- 3. the products with a moon origin, on a fake context ------------------------------------------
class FakeStore:
    narrow = True

    def __init__(self, ctx, total):
        self.ctx, self.total, self._r, self.freed = ctx, total, object(), 0

    def free(self):
        self.freed += 1
        self._r = None


class FakeContext:
    """Records what the products hand the device; the downloads are zeros of the right shape."""
    _h = True

    def __init__(self):
        self.calls, self.moved, self.sets = [], [], {}

    def make_room(self, need):
        self.calls.append(('make_room', need))

    def frame_rows(self, frame, store, first, count):
        moved = FakeStore(self, count)
        self.moved.append(moved)
        self.calls.append(('frame_rows', frame, store, first, count))
        return moved

    def counters(self):
        return dict(samples=1, samples_binned=1, nonfinite=0)

    def set_image(self, M, vr, apix, quantity, xedges, zedges, g_tables=(), downcast_f32=True):
        self.sets['image'] = dict(vr=vr, apix=apix, g_tables=g_tables)
        self.shape = (len(xedges) - 1, len(zedges) - 1)

    def camera_set(self, observer, basis, vr, pix_area, quantity, uedges, vedges, g_tables=()):
        self.sets['camera'] = dict(vr=vr, apix=pix_area, g_tables=g_tables, observer=observer)
        self.shape = (len(uedges) - 1, len(vedges) - 1)

    def shell_set(self, vr, quantity, lon_edges, mu_edges, r_lo, r_hi, nalt, g_tables=()):
        self.sets['shell'] = dict(vr=vr, g_tables=g_tables, r_lo=r_lo, r_hi=r_hi)
        self.shape = (len(lon_edges) - 1, len(mu_edges) - 1, nalt)

    def density_set(self, points, cell_start, origin, h, dr, dims):
        self.sets['density'] = dict(points=points, dr=dr)

    def _accumulate(self, *args, rows=None, **samples):
        self.calls.append(('accumulate', rows))

    image_accumulate_rows = lambda self, *rows: self._accumulate(rows=rows)        # noqa: E731
    image_moments_accumulate = image_cube_accumulate = camera_accumulate = _accumulate
    camera_moments_accumulate = camera_cube_accumulate = shell_accumulate = _accumulate
    density_accumulate = density_moments_accumulate = density_spectrum_accumulate = _accumulate

    def image_download(self):
        return np.zeros(self.shape), np.zeros(self.shape, dtype=np.uint64)

    camera_download = image_download

    def shell_download(self):
        cells = self.shape[:2]
        return (np.zeros(cells), np.zeros(cells, dtype=np.uint64),
                np.zeros((2,) + cells + (self.shape[2] + 2, 2)))

    def density_download(self):
        n = len(self.sets['density']['points'])
        return np.zeros(n), np.zeros(n)


APLANET, VR_KMS = 5.2, 0.37


def catalogued(inputs, ctx, rows=250):
    """One run with ``rows`` rows resident on ``ctx`` in the catalogue of ``inputs``."""
    run = Output.__new__(Output)
    run._store, run._row0, run._nrows, run._packet0 = FakeStore(ctx, rows + 7), 7, rows, 0
    run.aplanet, run.vrplanet, run.totalsource, run.npackets = APLANET, VR_KMS, 1000., 10
    run.idnum, run.filename, run._ctx = 1, None, ctx
    inputs._catalogue.append(run)
    return run


def quiet(make, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return make(*args, **kw)


IMAGE = dict(quantity='radiance', origin='Io', dims='16,16', width='12,12')
CAMERA = dict(quantity='radiance', origin='Io', observer='0,-6,1', fov='40,40', dims='8,8')
SHELL = dict(quantity='radiance', origin='Io', dims='8,6', altitude='0,4,4')


def products():
    from nexoclom_amd import CameraImage, ModelDensity, ModelImage, ShellMap
    points = np.array([[1.5, 0., 0.], [0., -2., 0.5]]).T
    return {'image': lambda inputs, **kw: ModelImage(inputs, IMAGE, **kw),
            'camera': lambda inputs, **kw: CameraImage(inputs, CAMERA, **kw),
            'shell': lambda inputs, **kw: ShellMap(inputs, SHELL, **kw),
            'density': lambda inputs, **kw: ModelDensity(inputs, *points, dr=0.1, origin='Io', **kw)}


@pytest.mark.parametrize('kind', ['image', 'camera', 'shell', 'density'])
def test_a_moon_origin_reaches_the_device_as_the_moons_unit(kind):
    from nexoclom_amd.atomicdata import gValue
    inputs, ctx = io_inputs(), FakeContext()
    run = catalogued(inputs, ctx)
    obj = quiet(products()[kind], inputs, context=ctx)
    frame = MoonFrame.from_inputs(inputs, 'Io')
    io_km = frame.unit_km
    assert obj.origin.object == 'Io' and obj.unit == 'R_Io' and obj.frame.name == 'Io'
    assert 1800 < io_km < 1850
    # the rows went through the frame: one slab, moved, read from row 0 and freed
    assert [c[0] for c in ctx.calls] == ['make_room', 'frame_rows', 'accumulate']
    assert ctx.calls[0][1] == 250*40
    assert ctx.calls[1][1].name == 'Io' and ctx.calls[1][2:] == (run._store, 7, 250)
    assert ctx.calls[2][1] == (ctx.moved[0], 0, 250) and ctx.moved[0].freed == 1
    assert run._store.freed == 0
    got = ctx.sets[kind]
    if kind == 'density':
        assert got['dr'] == 0.1 and float(obj.dr) == 0.1                # moon radii, as given
        assert sorted(got['points'][:, 0]) == [0., 1.5]
        np.testing.assert_allclose(float(obj.Vpix), 4/3/np.pi*0.1**3*(io_km*1e5)**3, rtol=1e-14)
        return
    assert obj.unit_km == io_km
    assert got['vr'] == (VR_KMS + frame.radvel_shift_kms)/io_km
    assert abs(frame.radvel_shift_kms) > 5.0                           # Io moves at 17 km/s
    for (v, g), line in zip(got['g_tables'], (5891, 5897)):
        table = gValue('Na', line, APLANET)
        assert np.array_equal(v, table.velocity/io_km) and np.array_equal(g, table.g)
    if kind == 'image':
        assert got['apix'] == (12/16)**2*(io_km*1e5)**2
        assert float(obj.width[0]) == 12 and obj.width[0].unit == 'R_Io'
    if kind == 'camera':
        assert np.array_equal(got['observer'], [0., -6., 1.])
        assert got['apix'] == obj.du*obj.dv*(io_km*1e5)**2
    if kind == 'shell':
        assert (got['r_lo'], got['r_hi']) == (1.0, 5.0)
        np.testing.assert_allclose(obj.altitude_edges_km, np.linspace(0, 4, 5)*io_km)


@pytest.mark.parametrize('kind', ['image', 'camera', 'shell', 'density'])
def test_without_an_origin_nothing_is_moved(kind):
    inputs, ctx = io_inputs(), FakeContext()
    run = catalogued(inputs, ctx)
    from nexoclom_amd import CameraImage, ModelDensity, ModelImage, ShellMap
    strip = lambda params: {k: v for k, v in params.items() if k != 'origin'}      # noqa: E731
    make = {'image': lambda: ModelImage(inputs, strip(IMAGE), context=ctx),
            'camera': lambda: CameraImage(inputs, dict(strip(CAMERA), origin='Jupiter'), context=ctx),
            'shell': lambda: ShellMap(inputs, strip(SHELL), context=ctx),
            'density': lambda: ModelDensity(inputs, [1.5], [0.], [0.], dr=0.1, context=ctx)}[kind]
    obj = quiet(make)
    assert obj.frame is None and 'Jupiter' in obj.unit
    assert ctx.calls == [('accumulate', (run._store, 7, 250))]
    if kind != 'density':
        jupiter_km = inputs.geometry.planet.radius.value
        assert obj.unit_km == jupiter_km and ctx.sets[kind]['vr'] == VR_KMS/jupiter_km


def test_sample_pass_moves_a_span_slab_by_slab():
    """250 rows in slabs of 97: 97 + 97 + 56, each moved store read from its row 0 and freed before
    the next is made."""
    from nexoclom_amd import ModelImage
    inputs, ctx = io_inputs(), FakeContext()
    run = catalogued(inputs, ctx)
    img = quiet(ModelImage, inputs, IMAGE, context=ctx, slab_rows=97)
    want, at = [], 7
    for k, n in enumerate((97, 97, 56)):
        want += [('make_room', n*40), ('frame_rows', img.frame, run._store, at, n),
                 ('accumulate', (ctx.moved[k], 0, n))]
        at += n
    assert ctx.calls == want and [m.freed for m in ctx.moved] == [1, 1, 1]
    assert img.counters['samples'] == 3 and img.totalsource == 1000.
    # the per-run path of create_image cuts the same slabs
    ctx.calls.clear(), ctx.moved.clear()
    quiet(img.create_image, run)
    assert [c[-1] for c in ctx.calls if c[0] == 'frame_rows'] == [97, 97, 56]
    assert [m.freed for m in ctx.moved] == [1, 1, 1] and img.counters['samples'] == 3
    with pytest.raises(ValueError, match='slab_rows'):
        quiet(ModelImage, inputs, IMAGE, context=ctx, slab_rows=0)


def test_a_run_without_resident_rows_goes_through_frame_columns():
    from nexoclom_amd.catalogue import framed_columns
    import pandas as pd
    rng = np.random.default_rng(4)
    names = ('time', 'x', 'y', 'z', 'vx', 'vy', 'vz', 'frac', 'lossfrac')
    run = Output.__new__(Output)
    run._X = pd.DataFrame({c: rng.uniform(0, 1, 9).astype(np.float32) for c in names})
    seen = {}

    class Ctx:
        def frame_columns(self, frame, *cols):
            seen['frame'], seen['cols'] = frame, cols
            return np.arange(54, dtype=np.float32).reshape(6, 9)

    got = framed_columns(Ctx(), 'the frame', run, Output.IMAGE_COLS)          # x, y, z, vy, frac
    assert seen['frame'] == 'the frame' and len(seen['cols']) == 7
    for col, name in zip(seen['cols'], names[:7]):
        assert np.array_equal(col, run._X[name].values)
    for k, moved_row in enumerate((0, 1, 2, 4)):
        assert np.array_equal(got[k], np.arange(54, dtype=np.float32).reshape(6, 9)[moved_row])
    assert np.array_equal(got[4], run._X['frac'].values)
    # a restored run (float32 values, widened) is moved as the float32 rows it was; rows that
    # never were float32 go over as they are
    stored = run._X
    run._X = Output.upcast(stored)
    framed_columns(Ctx(), 'the frame', run, Output.IMAGE_COLS)
    assert all(c.dtype == np.float32 for c in seen['cols'])
    assert all(np.array_equal(c, stored[name].values) for c, name in zip(seen['cols'], names))
    run._X = run._X.assign(y=run._X['y'] + 1e-12)
    framed_columns(Ctx(), 'the frame', run, Output.IMAGE_COLS)
    assert all(c.dtype == np.float64 for c in seen['cols'])
    run._X = pd.DataFrame()
    assert framed_columns(Ctx(), 'the frame', run, Output.IMAGE_COLS) is None


@pytest.mark.parametrize('kind', ['image', 'camera', 'shell'])
@pytest.mark.parametrize('kw', [dict(npackets=100), dict(shard=(0, 10)), dict(cp=object())],
                         ids=['npackets', 'shard', 'cp'])
def test_a_moon_origin_refuses_streaming_shards_and_shared_runs(kind, kw):
    inputs, ctx = io_inputs(), FakeContext()
    if kind == 'image' and 'cp' in kw:
        make = lambda: inputs.produce_image(IMAGE, cp=kw['cp'], context=ctx)        # noqa: E731
    else:
        make = lambda: products()[kind](inputs, context=ctx, **kw)                  # noqa: E731
    with pytest.raises(NotImplementedError) as err:
        quiet(make)
    assert len(str(err.value)) > 30 and not ctx.calls and not ctx.sets


def test_model_density_refuses_a_shared_run_and_a_stranger():
    from nexoclom_amd import ModelDensity
    inputs, ctx = io_inputs(), FakeContext()
    with pytest.raises(NotImplementedError, match='cp='):
        ModelDensity(inputs, [1.], [0.], [0.], origin='Io', cp=object(), context=ctx)
    with pytest.raises(ValueError, match='not a moon'):
        ModelDensity(inputs, [1.], [0.], [0.], origin='Ganymede', context=ctx)
    assert not ctx.calls and not ctx.sets


def test_an_origin_outside_the_run_is_refused():
    from nexoclom_amd import CameraImage, ModelImage, ShellMap
    inputs, ctx = io_inputs(), FakeContext()
    for cls, params in ((ModelImage, IMAGE), (CameraImage, CAMERA), (ShellMap, SHELL)):
        with pytest.raises(NotImplementedError, match='not a moon'):
            quiet(cls, inputs, dict(params, origin='Ganymede'), context=ctx)
    assert not ctx.calls and not ctx.sets


def test_los_result_does_not_take_an_origin():
    import inspect
    from nexoclom_amd.LOSResult import LOSResult
    assert 'origin' not in inspect.signature(LOSResult.__init__).parameters


# ---- 4. the C side's argument check, as a host program -----------------------------------------------
@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_argument_check_as_a_host_program(tmp_path, flags):
    """The refusals of nxc_frame_rows / nxc_frame_columns are host-only code
    (nxc_frame_check.hpp); tests/tools/frame_check.cpp feeds it good descriptions, ranges and
    columns and one bad one per refusal, plainly and under the host sanitizers."""
    exe = tmp_path / 'frame_check'
    subprocess.check_call(['g++', '-std=c++17', *flags, '-Wall', '-Werror',
                           os.path.join(HERE, 'tools', 'frame_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    assert not done.stderr
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 25 and sum(' accepted' in line for line in lines) >= 11
    for word in ('description is null', 'omega must be finite', 'M must be finite',
                 'U must be finite', 'scale must be finite', 'scale must be above 0',
                 'first lies outside', 'count reaches outside', 'column is null',
                 'must not be negative'):
        assert any(word in line for line in refused), word


# ---- 5. the ABI ------------------------------------------------------------------------------------
def test_the_descriptor_mirrors_the_header(tmp_path):
    header = os.path.join(HERE, '..', 'include', 'nexoclom_hip.h')
    fields = [name for name, _ in hip_api.nxc_frame_desc._fields_]
    assert fields == ['omega', 'M', 'U', 'scale']
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.abspath(header)}"',
             'int main(void){', 'printf("%zu", sizeof(nxc_frame_desc));']
    lines += [f'printf(" %zu", offsetof(nxc_frame_desc, {name}));' for name in fields]
    lines.append('return 0;}')
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    size, *offsets = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(hip_api.nxc_frame_desc) == 64
    assert offsets == [getattr(hip_api.nxc_frame_desc, name).offset for name in fields]
    assert offsets == [0, 8, 32, 56]


def test_the_library_exports_the_three_entry_points():
    names = ['nxc_frame_rows', 'nxc_frame_columns', 'nxc_frame_columns_f32']
    assert all(name in hip_api.EXPORTS for name in names)
    with open(os.path.join(HERE, '..', 'include', 'nexoclom_hip.h')) as f:
        header = f.read()
    assert 'Moon-centred frame' in header and all(f'int {name}(' in header for name in names)
    lib = hip_api.load_library()
    assert all(hasattr(lib, name) for name in names)
    assert lib.nxc_abi_version() == hip_api.ABI_VERSION == 3
    # no handle: refused by the library, loudly
    desc = hip_api.nxc_frame_desc(0.0, (C.c_double*3)(), (C.c_double*3)(), 1.0)
    assert lib.nxc_frame_columns(None, C.byref(desc), 0, *[None]*8) != 0
    assert b'null' in lib.nxc_last_error_string()


def test_frame_desc_of_a_moon_frame():
    frame = MoonFrame.from_inputs(io_inputs(), 'Io')
    desc = hip_api.Context.frame_desc(frame)
    assert isinstance(desc, hip_api.nxc_frame_desc) and hip_api.Context.frame_desc(desc) is desc
    assert (desc.omega, desc.scale) == (frame.omega, frame.scale)
    assert list(desc.M) == list(frame.M) and list(desc.U) == list(frame.U)
