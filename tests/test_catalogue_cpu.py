"""The catalogue walk every stored-sample consumer shares (nexoclom_amd/catalogue.py), without a
GPU: sample_spans over stand-in runs, shared_context, and the calls ModelImage._from_resident,
ModelDensity._accumulate, CameraImage._from_catalogue and ShellMap._from_catalogue make on a
recording context for the same catalogues, plain and with their velocity products."""
import contextlib
import io
import types

import numpy as np
import pandas as pd
import pytest

from nexoclom_amd import hip_api
from nexoclom_amd.catalogue import sample_spans, shared_context

# A catalogue as a list of runs: (store name, first row, row count[, key]) for rows in HBM,
# ('host', rows[, key]) for a run whose samples are on the host.
KEY = 7.0
CASES = {
    'adjacent': [('A', 0, 10), ('A', 10, 5), ('A', 15, 7)],
    'gap': [('A', 0, 10), ('A', 12, 5)],
    'two_stores': [('A', 0, 10), ('B', 10, 5)],
    'host_between': [('A', 0, 10), ('host', 4), ('A', 10, 5)],
    'empty_slice_between': [('A', 0, 10), ('A', 10, 0), ('A', 10, 5)],
    'empty_slice_alone': [('A', 3, 0)],
    'keys': [('A', 0, 10, 1.0), ('A', 10, 5, 2.0)],
    'empty': [],
}
# what sample_spans yields without a key ('run': the host run's row count)
SPANS = {
    'adjacent': [('rows', 'A', 0, 22)],
    'gap': [('rows', 'A', 0, 10), ('rows', 'A', 12, 5)],
    'two_stores': [('rows', 'A', 0, 10), ('rows', 'B', 10, 5)],
    'host_between': [('rows', 'A', 0, 10), ('run', 4), ('rows', 'A', 10, 5)],
    'empty_slice_between': [('rows', 'A', 0, 15)],
    'empty_slice_alone': [],
    'keys': [('rows', 'A', 0, 15)],
    'empty': [],
}


def key_of(spec):
    extra = spec[2:] if spec[0] == 'host' else spec[3:]
    return extra[0] if extra else KEY


class StandIn:
    """What sample_spans asks of a run"""

    def __init__(self, spec, stores):
        self.spec, self.key = spec, key_of(spec)
        self.view = None if spec[0] == 'host' else (stores[spec[0]], spec[1], spec[2], 0)

    def resident_rows(self, ctx):
        return self.view


def stand_ins(case):
    stores = {name: types.SimpleNamespace(name=name) for name in 'AB'}
    return [StandIn(spec, stores) for spec in CASES[case]]


def flat(items):
    out = []
    for kind, value in items:
        if kind == 'rows':
            out.append(('rows', value[0].name, value[1], value[2]))
        elif kind == 'run':
            out.append(('run', value.spec[1]))
        else:
            out.append(('key', value))
    return out


# ---- 1. sample_spans ------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_spans_without_a_key(case):
    assert flat(sample_spans(stand_ins(case), object())) == SPANS[case]


def test_keys_split_spans_and_are_announced_first():
    got = flat(sample_spans(stand_ins('keys'), object(), key=lambda run: run.key))
    assert got == [('key', 1.0), ('rows', 'A', 0, 10), ('key', 2.0), ('rows', 'A', 10, 5)]
    # one key: announced once, in front of everything, and the walk is the keyless one
    for case in sorted(CASES):
        got = flat(sample_spans(stand_ins(case), object(), key=lambda run: KEY))
        assert got == ([('key', KEY)] if CASES[case] else []) + SPANS[case]


def test_a_key_change_on_a_host_run_is_announced_before_it():
    runs = stand_ins('host_between')
    runs[1].key = 9.0
    got = flat(sample_spans(runs, object(), key=lambda run: run.key))
    assert got == [('key', KEY), ('rows', 'A', 0, 10), ('key', 9.0), ('run', 4), ('key', KEY),
                   ('rows', 'A', 10, 5)]


def test_runs_are_consumed_one_at_a_time():
    """What the caller does per run (a generator around the catalogue) happens in catalogue order
    and in front of the span that run ends."""
    seen = []

    def announced():
        for k, run in enumerate(stand_ins('gap')):
            seen.append(k)
            yield run

    walk = sample_spans(announced(), object())
    assert flat([next(walk)]) == [('rows', 'A', 0, 10)] and seen == [0, 1]
    assert flat(walk) == [('rows', 'A', 12, 5)]


# ---- 2. shared_context ----------------------------------------------------------------------------
def test_shared_context_is_the_last_live_one(monkeypatch):
    live_a, live_b = types.SimpleNamespace(_h=True), types.SimpleNamespace(_h=True)
    closed = types.SimpleNamespace(_h=None)
    run = lambda ctx: types.SimpleNamespace(_ctx=ctx)                     # noqa: E731
    monkeypatch.setattr(hip_api, 'Context', lambda device: ('new', device))
    inputs = types.SimpleNamespace(_catalogue=[run(live_a), run(None), run(live_b), run(closed)])
    assert shared_context(inputs, 3) is live_b
    assert shared_context(types.SimpleNamespace(_catalogue=[run(None), run(closed)]), 3) == ('new', 3)
    assert shared_context(types.SimpleNamespace(_catalogue=[]), 1) == ('new', 1)
    assert shared_context(types.SimpleNamespace(), 2) == ('new', 2)       # no catalogue at all


@pytest.mark.parametrize('module, name', [('ModelImage', 'ModelImage'), ('ModelDensity', 'ModelDensity'),
                                          ('CameraImage', 'CameraImage'), ('LOSResult', 'LOSResult')])
def test_every_class_finds_and_keeps_that_context(monkeypatch, module, name):
    import importlib
    cls = getattr(importlib.import_module('nexoclom_amd.' + module), name)
    live = types.SimpleNamespace(_h=True)
    made = []
    monkeypatch.setattr(hip_api, 'Context', lambda device: made.append(device) or ('new', device))
    obj = cls.__new__(cls)
    obj._ctx, obj._device = None, 5
    obj.inputs = types.SimpleNamespace(_catalogue=[types.SimpleNamespace(_ctx=live)])
    assert obj.context() is live and obj.context() is live and not made
    obj = cls.__new__(cls)
    obj._ctx, obj._device = None, 5
    obj.inputs = types.SimpleNamespace(_catalogue=[])
    assert obj.context() == ('new', 5) and obj.context() == ('new', 5) and made == [5]
    given = object()
    obj._ctx = given
    assert obj.context() is given


# ---- 3. the classes on a recording context ----------------------------------------------------------
CUBE = (-3., 3., 3)                               # a cube= argument: km/s, km/s, bins
VELOCITY_COLS = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')


class Recorder:
    """Answers the Context methods the walks call and records them: ``calls`` is what the walks
    are pinned by, ``names`` the Context method behind every call (``counters`` included).  Like
    the C entries it treats a rows call without rows as nothing at all.

    A plain accumulate entry records ('rows', store, first, count) or ('host', rows); a moments,
    cube or spectrum entry appends its name, and to a host call the number of columns it was sent:
    ('rows', store, first, count, 'cube'), ('host', rows, 'cube', 7)."""
    _h = True

    def __init__(self, dims=(2, 2)):
        self.calls, self.names = [], []
        self.dims, self.nv = tuple(dims), 0

    def _samples(self, name, cols, rows, entry=()):
        self.names.append(name)
        if rows is None:
            assert all(len(c) == len(cols[0]) for c in cols)             # None: a column not sent
            self.calls.append(('host', len(cols[0])) + ((entry, len(cols)) if entry else ()))
        elif rows[2]:
            self.calls.append(('rows', rows[0].name, rows[1], rows[2]) + ((entry,) if entry else ()))

    def _said(self, name, call):
        self.names.append(name)
        self.calls.append(call)

    def counters(self):
        self.names.append('counters')
        return dict(samples=1, nonfinite=0)

    def _pair(self, name):
        self._said(name, 'download')
        return np.zeros(self.dims), np.zeros(self.dims, dtype=np.uint64)

    # the image
    def set_image(self, M, vrplanet, *rest, **options):
        self._said('set_image', ('set', vrplanet))

    def image_accumulate_rows(self, store, first=0, count=None):
        self._samples('image_accumulate_rows', None, (store, first, count))

    def image_download(self):
        return self._pair('image_download')

    # the density
    def density_set(self, *args):
        self._said('density_set', 'set')

    def density_accumulate(self, x=None, y=None, z=None, frac=None, rows=None):
        self._samples('density_accumulate', (x, y, z, frac), rows)

    def density_download(self):
        self._said('density_download', 'download')
        return np.zeros(0), np.zeros(0)

    # the camera
    def camera_set(self, observer, basis, vrplanet, *rest):
        self._said('camera_set', ('set', vrplanet))

    def camera_accumulate(self, x=None, y=None, z=None, vy=None, frac=None, rows=None):
        self._samples('camera_accumulate', (x, y, z, vy, frac), rows)

    def camera_download(self):
        return self._pair('camera_download')

    # the shell map
    def shell_set(self, vrplanet, *rest):
        self._said('shell_set', ('set', vrplanet))

    def shell_accumulate(self, x=None, y=None, z=None, vy=None, frac=None, rows=None):
        self._samples('shell_accumulate', (x, y, z, vy, frac), rows)

    def shell_download(self):
        column, counts = self._pair('shell_download')
        return column, counts, np.zeros((2,) + self.dims + (3, 2))

    def __getattr__(self, name):
        """<image|camera|density>_<moments|cube|spectrum>_<enable|accumulate|download>"""
        prefix, _, rest = name.partition('_')
        what, _, op = rest.partition('_')
        if prefix not in ('image', 'camera', 'density') or what not in ('moments', 'cube', 'spectrum') \
                or op not in ('enable', 'accumulate', 'download'):
            raise AttributeError(name)

        def enable(*args):
            self.nv = args[0] if what != 'moments' else 0
            self._said(name, (what + '_enable',) + args[:3] if args else what + '_enable')

        def accumulate(x=None, y=None, z=None, vx=None, vy=None, vz=None, frac=None, rows=None):
            self._samples(name, (x, y, z, vx, vy, vz, frac), rows, entry=what)

        def download():
            self._said(name, what + '_download')
            pixels = (0,) if prefix == 'density' else self.dims
            return np.zeros({'moments': pixels + (10 if prefix == 'density' else 4,),
                             'cube': pixels + (self.nv + 2, 2),
                             'spectrum': (2,) + pixels + (self.nv + 2, 2)}[what])

        return {'enable': enable, 'accumulate': accumulate, 'download': download}[op]

    def only(self, *prefixes, counters=True):
        """Every call went to an entry of these prefixes (and, if ``counters``, to counters())."""
        ok = [n for n in self.names if n.startswith(prefixes) or (counters and n == 'counters')]
        return ok == self.names


def outputs(case, ctx):
    """The case's catalogue (its name, or the list itself) as Outputs: rows in ``ctx``'s HBM, or a
    frame on the host."""
    from nexoclom_amd.Output import Output
    stores = {name: types.SimpleNamespace(name=name, ctx=ctx, _r=object()) for name in 'AB'}
    runs = []
    for k, spec in enumerate(CASES[case] if isinstance(case, str) else case):
        out = Output.__new__(Output)
        out.filename, out.totalsource = f'run{k}', 2.0
        out.aplanet, out.vrplanet = 0.4, key_of(spec)
        if spec[0] == 'host':
            out.X = pd.DataFrame({c: np.zeros(spec[1], dtype=np.float32)
                                  for c in ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')})
        else:
            out._X = None
            out._store, out._row0, out._nrows = stores[spec[0]], spec[1], spec[2]
        runs.append(out)
    return runs


def walked(obj, method, *args):
    with contextlib.redirect_stdout(io.StringIO()) as said:
        result = method(*args)
    return result, said.getvalue().splitlines()


def rows_and_hosts(calls):
    """(rows covered per store as merged ranges, host calls in order): what a sum that does not
    depend on the order of its terms sees of a call sequence."""
    covered = {}
    for call in calls:
        if call[0] == 'rows':
            covered.setdefault(call[1], []).append((call[2], call[2] + call[3]))
    merged = {}
    for name, ranges in covered.items():
        out = []
        for lo, hi in sorted(ranges):
            if out and out[-1][1] == lo:
                out[-1] = (out[-1][0], hi)
            else:
                out.append((lo, hi))
        merged[name] = out
    return merged, [call for call in calls if call[0] == 'host']


def expected(case):
    return [(kind, *rest) if kind == 'rows' else ('host', *rest) for kind, *rest in SPANS[case]]


@pytest.mark.parametrize('case', sorted(CASES))
def test_model_image_walk(case):
    """_from_resident takes a catalogue only when every run is resident under one (aplanet,
    vrplanet); then: set, one rows call per span, one download."""
    from nexoclom_amd.ModelImage import ModelImage
    ctx = Recorder()
    img = ModelImage.__new__(ModelImage)
    img._ctx, img.inputs, img.unit_km, img.totalsource = ctx, None, 2440., 0.
    img.image = img.packet_image = np.zeros((2, 2))
    img.xedges = img.zedges = np.arange(3.)
    img._set_image = lambda c, aplanet, vr, downcast: c.calls.append(('set', vr*img.unit_km))
    runs = outputs(case, ctx)
    took, said = walked(img, img._from_resident, runs)
    if case in ('host_between', 'keys', 'empty'):
        assert not took and ctx.calls == [] and img.totalsource == 0.
        return
    assert took
    assert ctx.calls[0][0] == 'set' and ctx.calls[0][1] == pytest.approx(KEY)
    assert ctx.calls[1:] == expected(case) + ['download'] and ctx.only('image_')
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert img.totalsource == 2.0*len(runs)
    assert img.counters == ({} if case == 'empty_slice_alone' else
                            dict(samples=len(SPANS[case]), nonfinite=0))


@pytest.mark.parametrize('case', sorted(CASES))
def test_model_density_walk(case):
    """Every sample once, whatever the launches: the per-point sums do not depend on the order of
    their terms, so what is pinned is which rows and which host frames go in (the walk of before
    this module carried a span across a host run; sample_spans ends it there)."""
    from nexoclom_amd.ModelDensity import ModelDensity
    ctx = Recorder()
    dens = ModelDensity.__new__(ModelDensity)
    dens._ctx, dens.totalsource = ctx, 0.
    runs = outputs(case, ctx)
    dens.inputs = types.SimpleNamespace(_catalogue=runs)
    index = types.SimpleNamespace(points=np.zeros((0, 3)), cell_start=np.zeros(2, dtype=np.int32),
                                  origin=np.zeros(3), h=1., dr=.5, dims=(1, 1, 1))
    _, said = walked(dens, dens._accumulate, index)
    assert ctx.calls[0] == 'set' and ctx.calls[-1] == 'download'
    assert ctx.only('density_', counters=False)
    assert rows_and_hosts(ctx.calls[1:-1]) == rows_and_hosts(expected(case))
    assert len(ctx.calls) - 2 <= len(CASES[case])
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert dens.totalsource == 2.0*len(runs)


@pytest.mark.parametrize('case', sorted(CASES))
def test_camera_image_walk(case):
    """set per stretch of one (aplanet, vrplanet), the spans and host runs of that stretch in
    order, download at its end."""
    from nexoclom_amd.CameraImage import CameraImage
    ctx = Recorder()
    cam = CameraImage.__new__(CameraImage)
    cam._ctx, cam.unit_km, cam.totalsource = ctx, 2440., 0.
    cam.observer = cam.basis = cam.uedges = cam.vedges = None
    cam.pix_area_cm2, cam.quantity = 1., 'column'
    cam.g_tables = lambda aplanet: []
    cam.image = np.zeros((2, 2))
    cam.packet_image = np.zeros((2, 2))
    runs = outputs(case, ctx)
    cam.inputs = types.SimpleNamespace(_catalogue=runs)
    _, said = walked(cam, cam._from_catalogue)
    if case == 'empty':
        assert ctx.calls == [] and said == ['No model outputs found for these inputs.']
        return
    if case == 'keys':
        want = [('set', 1.0/2440.), ('rows', 'A', 0, 10), 'download',
                ('set', 2.0/2440.), ('rows', 'A', 10, 5), 'download']
    else:
        want = [('set', KEY/2440.)] + expected(case) + ['download']
    assert ctx.calls == want and ctx.only('camera_')
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert cam.totalsource == 2.0*len(runs)
    launches = sum(1 for call in want if call[0] in ('rows', 'host'))
    assert cam.counters == ({} if not launches else dict(samples=launches, nonfinite=0))


# ---- 4. the same walks with the velocity products, a shell map, an .npz run, an empty host run ------
ENABLE = {'moments': 'moments_enable', 'cube': ('cube_enable', CUBE[2], CUBE[0]/2440., CUBE[1]/2440.)}


def keyed_walk(case, entry=None):
    """What a keyed consumer calls for a catalogue: per stretch of one key the set (with
    ``entry``, 'moments' or 'cube': and its enable), the stretch's spans and host runs in order
    (through that entry, a host run with seven columns), the download (and the entry's)."""
    stretches = [(1.0, [('rows', 'A', 0, 10)]), (2.0, [('rows', 'A', 10, 5)])] if case == 'keys' \
        else [(KEY, expected(case))]
    want = []
    for key, calls in stretches:
        want.append(('set', key/2440.))
        if entry:
            calls = [call + ((entry,) if call[0] == 'rows' else (entry, 7)) for call in calls]
            want.append(ENABLE[entry])
        want += calls + ['download'] + ([entry + '_download'] if entry else [])
    return want


def launches_in(calls):
    return sum(1 for call in calls if call[0] in ('rows', 'host'))


def with_velocity(obj, entry):
    obj.moments, obj.cube = entry == 'moments', CUBE if entry == 'cube' else None
    obj.moment_sums = np.zeros((2, 2, 4))
    obj.cube_sums = np.zeros((2, 2, CUBE[2] + 2, 2))
    return obj


def new_camera(ctx, runs, entry=None):
    from nexoclom_amd.CameraImage import CameraImage
    cam = CameraImage.__new__(CameraImage)
    cam._ctx, cam.unit_km, cam.totalsource = ctx, 2440., 0.
    cam.observer = cam.basis = cam.uedges = cam.vedges = None
    cam.pix_area_cm2, cam.quantity = 1., 'column'
    cam.g_tables = lambda aplanet: []
    cam.image = np.zeros((2, 2))
    cam.packet_image = np.zeros((2, 2))
    cam.inputs = types.SimpleNamespace(_catalogue=runs)
    return with_velocity(cam, entry)


def new_density(ctx, runs):
    from nexoclom_amd.ModelDensity import ModelDensity
    dens = ModelDensity.__new__(ModelDensity)
    dens._ctx, dens.totalsource, dens.counters = ctx, 0., {}
    dens.inputs = types.SimpleNamespace(_catalogue=runs)
    dens.origin = types.SimpleNamespace(radius=types.SimpleNamespace(value=2440.))
    dens._spectrum = dict(speed=(1., 4., 3), cos_half=-1., all_sky=True)
    index = types.SimpleNamespace(points=np.zeros((0, 3)), cell_start=np.zeros(2, dtype=np.int32),
                                  origin=np.zeros(3), h=1., dr=.5, dims=(1, 1, 1))
    return dens, index


VELOCITY_CASES = ['adjacent', 'gap', 'two_stores', 'host_between', 'keys', 'empty_slice_alone']


@pytest.mark.parametrize('entry', ['moments', 'cube'])
@pytest.mark.parametrize('case', VELOCITY_CASES)
def test_camera_image_walk_with_velocity_products(case, entry):
    """The enable follows every set, spans and host runs go through the entry asked for (a host
    run with seven columns), its download follows every image download."""
    ctx = Recorder()
    runs = outputs(case, ctx)
    cam = new_camera(ctx, runs, entry)
    _, said = walked(cam, cam._from_catalogue)
    want = keyed_walk(case, entry)
    assert ctx.calls == want and ctx.only('camera_')
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert cam.totalsource == 2.0*len(runs)
    launches = launches_in(want)
    assert ctx.names.count('counters') == launches
    assert cam.counters == ({} if not launches else dict(samples=launches, nonfinite=0))


@pytest.mark.parametrize('entry', [None, 'moments', 'cube'])
@pytest.mark.parametrize('case', VELOCITY_CASES)
def test_model_image_walk_through_set_image(case, entry):
    """_from_resident with the _set_image of the class: set_image, then the enable; the rows
    through the entry asked for; the entry's download after the image's."""
    from nexoclom_amd.ModelImage import ModelImage
    ctx = Recorder()
    img = with_velocity(ModelImage.__new__(ModelImage), entry)
    img._ctx, img.inputs, img.unit_km, img.totalsource = ctx, None, 2440., 0.
    img.image, img.packet_image = np.zeros((2, 2)), np.zeros((2, 2))
    img.xedges = img.zedges = np.arange(3.)
    img.subobslongitude, img.subobslatitude, img.Apix, img.quantity = 0., np.pi/2, 1., 'column'
    img.g_tables = lambda aplanet: []
    runs = outputs(case, ctx)
    took, said = walked(img, img._from_resident, runs)
    if case in ('host_between', 'keys'):
        assert not took and ctx.names == [] and said == [] and img.totalsource == 0.
        return
    want = keyed_walk(case, entry)
    assert took and ctx.calls == want and ctx.only('set_image', 'image_')
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert img.totalsource == 2.0*len(runs)
    assert ctx.names.count('counters') == launches_in(want)
    assert img.counters == ({} if not launches_in(want) else
                            dict(samples=launches_in(want), nonfinite=0))


@pytest.mark.parametrize('case', sorted(CASES))
def test_shell_map_walk(case):
    """set per stretch of one (aplanet, vrplanet), the spans and host runs of that stretch in
    order, download at its end."""
    from nexoclom_amd.ShellMap import ShellMap
    ctx = Recorder()
    runs = outputs(case, ctx)
    shell = ShellMap.__new__(ShellMap)
    shell._ctx, shell.unit_km, shell.totalsource, shell.quantity = ctx, 2440., 0., 'column'
    shell.lon_edges = shell.mu_edges = None
    shell.r_edges, shell.altitude = np.array([1., 2.]), (0., 1., 1)
    shell.g_tables = lambda aplanet: []
    shell._column_sum, shell.packets = np.zeros((2, 2)), np.zeros((2, 2))
    shell.shell_sums = np.zeros((2, 2, 2, 3, 2))
    shell.inputs = types.SimpleNamespace(_catalogue=runs)
    _, said = walked(shell, shell._from_catalogue)
    if case == 'empty':
        assert ctx.names == [] and said == ['No model outputs found for these inputs.']
        return
    want = keyed_walk(case)
    assert ctx.calls == want and ctx.only('shell_')
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert shell.totalsource == 2.0*len(runs)
    launches = launches_in(want)
    assert ctx.names.count('counters') == launches
    assert shell.counters == ({} if not launches else dict(samples=launches, nonfinite=0))


@pytest.mark.parametrize('entry', [None, 'moments', 'spectrum'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_model_density_walk_never_reads_the_counters(case, entry):
    """set, the entry's enable, then the walk through that entry (a host run with seven columns),
    the entry's download and the density's; no counters() at all, and ``counters`` stays {}."""
    ctx = Recorder()
    runs = outputs(case, ctx)
    dens, index = new_density(ctx, runs)
    frames = np.zeros((0, 8)) if entry == 'spectrum' else None
    result, said = walked(dens, dens._accumulate, index, entry == 'moments', frames)
    enable = {None: [], 'moments': ['moments_enable'],
              'spectrum': [('spectrum_enable', 3, 1./2440., 4./2440.)]}[entry]
    tail = ([entry + '_download'] if entry else []) + ['download']
    assert ctx.calls[:1 + len(enable)] == ['set'] + enable and ctx.calls[-len(tail):] == tail
    walk = ctx.calls[1 + len(enable):-len(tail)]
    if entry:
        assert all(call[4 if call[0] == 'rows' else 2:] == ((entry,) if call[0] == 'rows' else
                                                           (entry, 7)) for call in walk)
        walk = [call[:4 if call[0] == 'rows' else 2] for call in walk]
    assert rows_and_hosts(walk) == rows_and_hosts(expected(case))
    assert ctx.only('density_', counters=False) and dens.counters == {}
    assert said == [f'Output filename: run{k}' for k in range(len(runs))]
    assert dens.totalsource == 2.0*len(runs)
    assert len(result) == 3 and (result[2] is None) == (entry is None)


def npz_run(tmp_path):
    """An .npz run with just what the walks read: four float32 rows under key KEY"""
    path = str(tmp_path / 'stored.npz')
    np.savez(path, totalsource=3.0, aplanet=0.4, vrplanet_kms=KEY,
             **{'X.' + c: np.zeros(4, dtype=np.float32) for c in VELOCITY_COLS})
    return path


def test_camera_image_walk_takes_an_npz_path(tmp_path):
    ctx = Recorder()
    runs = outputs(CASES['host_between'], ctx)
    runs[1] = npz_run(tmp_path)
    cam = new_camera(ctx, runs)
    _, said = walked(cam, cam._from_catalogue)
    assert ctx.calls == keyed_walk('host_between') and ctx.only('camera_')
    assert said == ['Output filename: run0', f'Output filename: {runs[1]}', 'Output filename: run2']
    assert cam.totalsource == 2.0 + 3.0 + 2.0
    assert cam.counters == dict(samples=3, nonfinite=0)


def test_model_density_walk_takes_an_npz_path(tmp_path):
    """Through the shared pass the density reads a stored run like the images do (its own walk
    took Outputs only)."""
    ctx = Recorder()
    runs = outputs(CASES['host_between'], ctx)
    runs[1] = npz_run(tmp_path)
    dens, index = new_density(ctx, runs)
    _, said = walked(dens, dens._accumulate, index)
    assert ctx.calls == ['set'] + expected('host_between') + ['download']
    assert ctx.only('density_', counters=False) and dens.counters == {}
    assert said == ['Output filename: run0', f'Output filename: {runs[1]}', 'Output filename: run2']
    assert dens.totalsource == 2.0 + 3.0 + 2.0


@pytest.mark.parametrize('consumer', ['camera', 'density'])
def test_an_empty_host_run_is_skipped(consumer):
    """An Output whose X is empty: announced and counted in totalsource, but no accumulate call
    and no counters read for it."""
    ctx = Recorder()
    runs = outputs([('A', 0, 10), ('host', 0), ('A', 10, 5)], ctx)
    if consumer == 'camera':
        cam = new_camera(ctx, runs)
        _, said = walked(cam, cam._from_catalogue)
        assert ctx.calls == [('set', KEY/2440.), ('rows', 'A', 0, 10), ('rows', 'A', 10, 5), 'download']
        assert ctx.names.count('counters') == 2 and cam.counters == dict(samples=2, nonfinite=0)
        assert cam.totalsource == 6.0
    else:
        dens, index = new_density(ctx, runs)
        _, said = walked(dens, dens._accumulate, index)
        assert ctx.calls == ['set', ('rows', 'A', 0, 10), ('rows', 'A', 10, 5), 'download']
        assert 'counters' not in ctx.names and dens.totalsource == 6.0
    assert said == [f'Output filename: run{k}' for k in range(3)]
