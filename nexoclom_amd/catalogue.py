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


def sample_pass(product, runs, accumulate, columns, set_up=None, collect=None, counters=True):
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
    every launch, totalled into ``product.counters`` and must show no non-finite weight."""
    if not runs:
        print('No model outputs found for these inputs.')
        return
    ctx = product.context()
    totals = {}

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
        if kind == 'rows':
            accumulate(ctx, rows=item)
        else:
            samples = Output.sample_columns(item, columns)
            if samples is None or not len(samples[0]):
                continue
            accumulate(ctx, **dict(zip(columns, samples)))
        if counters:
            for key, v in ctx.counters().items():
                totals[key] = totals.get(key, 0) + v
    if collect:
        collect(ctx)
    if counters:
        product.counters = totals
        assert totals.get('nonfinite', 0) == 0, 'Non-finite weights'
