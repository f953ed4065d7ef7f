"""What every consumer of a catalogue's stored samples (ModelImage, ModelDensity, CameraImage,
ShellMap, LOSResult) does around its own kernel: find the device the runs were made on, and walk
the catalogue so that rows still in HBM are read where they are, in as few launches as they allow
(``sample_pass``: the whole pass of the four that sum over a catalogue)."""
import numpy as np

from .Output import Output


def shared_context(inputs, device):
    """The context of the last catalogued run whose context is alive -- its rows are still in that
    device's HBM, and a new handle costs 0.1 s -- else a new one on ``device``."""
    shared = [getattr(run, '_ctx', None) for run in getattr(inputs, '_catalogue', ())]
    shared = [ctx for ctx in shared if ctx is not None and getattr(ctx, '_h', True)]
    if shared:
        return shared[-1]
    from . import hip_api
    return hip_api.Context(device)


def sample_spans(runs, ctx, key=None):
    """The catalogue ``runs`` in order, as ``(kind, value)``:

    ``('rows', (store, first, count))``: a maximal stretch of consecutive runs whose rows sit in
    ``ctx``'s HBM as adjacent slices of one store (and share ``key(run)``): one launch.  Stretches
    without rows are left out.
    ``('run', run)``: a run without resident rows (a restored Output, an .npz path): the caller
    uploads its columns.
    ``('key', k)``: with ``key``, in front of the first item of every stretch of equal keys.

    ``runs`` is consumed one run at a time: what the caller does per run (a generator around the
    catalogue) happens in catalogue order, in front of the items that run ends."""
    span = None                                   # (store, first row, row count)
    current = first_key = object()

    def flush():
        nonlocal span
        done, span = span, None
        if done is not None and done[2]:
            yield 'rows', done

    for run in runs:
        rows = getattr(run, 'resident_rows', None)
        view = rows(ctx) if rows is not None else None
        if key is not None:
            k = key(run)
            if current is first_key or k != current:
                yield from flush()
                current = k
                yield 'key', k
        if view is None:
            yield from flush()
            yield 'run', run
            continue
        store, first, count = view[:3]
        if span is not None and span[0] is store and span[1] + span[2] == first:
            span = (store, span[1], span[2] + count)
        else:
            yield from flush()
            span = (store, first, count)
    yield from flush()


def run_totalsource(run):
    """totalsource of a catalogued Output or an .npz path"""
    if not isinstance(run, Output.PATH):
        return run.totalsource
    with np.load(run, allow_pickle=False) as data:
        return float(data['totalsource'])


def run_g_values(run):
    """(aplanet [au], vrplanet [km/s]) of a catalogued Output or an .npz path: what the g-values
    of a run depend on"""
    if not isinstance(run, Output.PATH):
        return float(run.aplanet), float(run.vrplanet)
    with np.load(run, allow_pickle=False) as data:
        return float(data['aplanet']), float(data['vrplanet_kms'])


FRAME_COLS = ('time', 'x', 'y', 'z', 'vx', 'vy', 'vz')      # what moving a row into a frame reads


def framed_columns(ctx, frame, source, columns):
    """The sample ``columns`` of a stored run without resident rows (a catalogued Output or an
    .npz path) with its positions and velocities moved into ``frame``: time and the six state
    columns go through ``ctx.frame_columns`` in the width they are stored in, the rest is handed
    on as it is.  A restored Output holds save()'s float32 values widened (Output.py:555-570): it
    is moved as the float32 rows it was, so that a run gives the same moved rows from HBM, from
    its file and restored.  None: the run holds no trajectory."""
    names = FRAME_COLS + tuple(c for c in columns if c not in FRAME_COLS)
    samples = Output.sample_columns(source, names)
    if samples is None or not len(samples[0]):
        return None
    table = dict(zip(names, samples))
    state = [np.asarray(table[c]) for c in FRAME_COLS]
    if all(c.dtype == np.float64 for c in state):
        with np.errstate(over='ignore'):
            narrow = [c.astype(np.float32) for c in state]
        if all(np.array_equal(n, c) for n, c in zip(narrow, state)):
            state = narrow
    moved = ctx.frame_columns(frame, *state)
    table.update(zip(FRAME_COLS[1:], moved))
    return [table[c] for c in columns]


def framed_slabs(ctx, frame, rows, slab_rows):
    """``rows = (store, first, count)`` moved into ``frame`` slab by slab: yields ``(moved, 0, n)``
    with ``moved`` a store of at most ``slab_rows`` rows that is freed when the caller comes back
    for the next one, so the extra HBM is one slab whatever the size of the catalogue."""
    store, first, count = rows
    per_row = 40 if store.narrow else 80
    for at in range(0, count, slab_rows):
        n = min(slab_rows, count - at)
        ctx.make_room(n*per_row)
        if store._r is None:
            raise MemoryError('no room on the device for a slab of moved rows beside the rows '
                              'they are moved from; pass a smaller slab_rows')
        moved = ctx.frame_rows(frame, store, first + at, n)
        try:
            yield moved, 0, n
        finally:
            moved.free()


def sample_pass(product, runs, accumulate, columns, set_up=None, collect=None, counters=True,
                frame=None, slab_rows=1 << 26):
    """Every stored sample of the catalogue ``runs`` through one consumer, on
    ``product.context()``.

    Each run is announced and its totalsource added to ``product.totalsource``, in catalogue
    order.  Rows in HBM go to ``accumulate(ctx, rows=(store, first, count))``, one launch per
    stretch of adjacent slices of a store; any other run that holds a trajectory uploads its
    host ``columns``: ``accumulate(ctx, x=..., ...)``.
    ``set_up(ctx, aplanet, vr_kms)`` runs in front of every stretch of runs of equal (aplanet
    [au], vrplanet [km/s]) -- the sums stay on the device over such a stretch -- and
    ``collect(ctx)`` at the end of each.
    ``counters``: the consumer's kernels clear the context's counters, so they are read after
    every launch, totalled into ``product.counters`` and must show no non-finite weight.
    ``frame`` (a frames.MoonFrame): every row is moved into that frame first (k_frame_rows) and
    the consumer runs unchanged on the moved rows -- resident spans in slabs of ``slab_rows``
    rows (``framed_slabs``), other runs through ``framed_columns``.  None: nothing is moved, and
    the pass is the same launches as ever."""
    if not runs:
        print('No model outputs found for these inputs.')
        return
    ctx = product.context()
    totals = {}

    def launch(**samples):
        accumulate(ctx, **samples)
        if counters:
            for key, v in ctx.counters().items():
                totals[key] = totals.get(key, 0) + v

    def announced():
        for run in runs:
            print(f'Output filename: {getattr(run, "filename", run)}')
            product.totalsource += run_totalsource(run)
            yield run

    is_set = False
    for kind, item in sample_spans(announced(), ctx, key=run_g_values if set_up else None):
        if kind == 'key':
            if is_set and collect:
                collect(ctx)
            set_up(ctx, *item)
            is_set = True
            continue
        if kind == 'rows' and frame is None:
            launch(rows=item)
        elif kind == 'rows':
            for moved in framed_slabs(ctx, frame, item, slab_rows):
                launch(rows=moved)
        else:
            samples = Output.sample_columns(item, columns) if frame is None else \
                framed_columns(ctx, frame, item, columns)
            if samples is None or not len(samples[0]):
                continue
            launch(**dict(zip(columns, samples)))
    if collect:
        collect(ctx)
    if counters:
        product.counters = totals
        assert totals.get('nonfinite', 0) == 0, 'Non-finite weights'
