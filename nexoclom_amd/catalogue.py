"""What every consumer of a catalogue's stored samples (ModelImage, ModelDensity, CameraImage,
LOSResult) does before its own kernel runs: find the device the runs were made on, and walk the
catalogue so that rows still in HBM are read where they are, in as few launches as they allow."""


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
