"""k_frame_rows over the resident rows of Input.run(1e6) (1.3e8 float32 rows in HBM), against a
streaming copy of the same bytes: 40 B per row read and 40 B written (nine float32 columns and the
int32 index).  The rows are moved as catalogue.sample_pass moves them, in slabs of 2^26 rows, into
a frame with Io's rate and offsets (the bench input has no moon; the kernel does not care whose
numbers they are).  One process; 1 warm-up round and 5 timed ones; a round's figure is the
HIP-event time (nxc_last_kernel_ms) summed over the slabs.  One JSON line (appended to
``--out FILE``): median [min, max] ms, the copy's rate and its time for the same bytes, their
ratio, and whether the slabs took the 16-byte path (every column of source and destination on a
16-byte boundary) or one row per thread.  No time is a gate.

    python tools/gpu_exp_frame_rows.py [--out FILE] [N]          (default: 1e6)
"""
import contextlib
import io
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                            # noqa: E402
from nexoclom_amd import Input, hip_api                        # noqa: E402
from nexoclom_amd.catalogue import sample_spans                # noqa: E402

SLAB = 1 << 26
WARMUP, ROUNDS = 1, 5
FRAME = types.SimpleNamespace(omega=4.11e-5, M=(-4.96, 3.19, 0.0), U=(-1.1e-4, -2.1e-4, 0.0),
                              scale=39.2)


def main():
    args = sys.argv[1:]
    out_path = None
    if '--out' in args:
        out_path = args[args.index('--out') + 1]
        del args[args.index('--out'):args.index('--out') + 2]
    n = float(args[0]) if args else 1e6
    ctx = hip_api.Context(0)
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
    spans = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in spans)
    assert all(store.narrow for store, _, _ in spans)
    slabs = [(store, first + at, min(SLAB, count - at))
             for store, first, count in spans for at in range(0, count, SLAB)]
    wide = [store.total % 4 == 0 and first % 4 == 0 and count % 4 == 0
            for store, first, count in slabs]
    times = []
    for rnd in range(WARMUP + ROUNDS):
        ms = 0.0
        for store, first, count in slabs:
            moved = ctx.frame_rows(FRAME, store, first, count)
            ms += ctx.last_kernel_ms()
            moved.free()
        if rnd >= WARMUP:
            times.append(ms)
    copy_gbs = ctx.stream_copy_gbs(nbytes=40*max(s[2] for s in slabs), reps=5)
    copy_ms = 80*rows/(copy_gbs*1e9)*1e3
    med = float(np.median(times))
    line = json.dumps({
        'npackets': n, 'rows': rows, 'slabs': len(slabs), 'sixteen_byte_path': wide,
        'k_frame_rows_ms': [round(med, 3), round(min(times), 3), round(max(times), 3)],
        'bytes': 80*rows, 'k_frame_rows_gbs': round(80*rows/(med*1e-3)/1e9, 1),
        'stream_copy_gbs': round(copy_gbs, 1), 'stream_copy_ms_same_bytes': round(copy_ms, 3),
        'frame_over_copy': round(med/copy_ms, 3)})
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
