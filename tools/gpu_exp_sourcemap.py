"""LOSResult.make_source_map over the catalogue of Input.run(N), default grid (180 x 90 points,
10 deg smear radius, 100 / 23 / 45 speed / altitude / azimuth bins): wall time of one call that
builds both maps (source + available), the (point, packet) hits per packet, and the time of the
device's source map of the first few Outputs.  Prints one JSON line per size.  The NumPy
restatement's time on the same Outputs is added by
tests/tools/gpu_exp_sourcemap_restatement.py, which runs this with a hook.  Per-kernel times: run
it under `rocprofv3 --kernel-trace --stats -d DIR --` (k_smap_prep, k_smap_points, k_smap_gridsum).

    python tools/gpu_exp_sourcemap.py [N ...]          (default: 1e6 1e7)
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nexoclom_amd import Input, LOSResult, hip_api                    # noqa: E402

FEW = 3                    # Outputs the device's source-only map is timed on


def timed(fn):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn()
    return (time.perf_counter() - t0)*1e3, out


def result(inputs, ctx, catalogue):
    res = LOSResult.__new__(LOSResult)
    res.inputs = type('Inputs', (), {})()
    res.inputs._catalogue = catalogue
    res.unit_km, res.sourcerate, res._ctx = inputs.geometry.planet.radius.value, 1.0, ctx
    return res


def main(sizes=None, extra=None):
    """``extra(few)``: more fields for each line, from the LOSResult over the first FEW Outputs."""
    sizes = sizes or [float(a) for a in sys.argv[1:]] or [1e6, 1e7]
    ctx = hip_api.Context(0)
    for n in sizes:
        inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
        with contextlib.redirect_stdout(io.StringIO()):
            inputs.run(n, seed=7, context=ctx)
        res = result(inputs, ctx, inputs._catalogue)
        ms = [timed(res.make_source_map)[0] for _ in range(2)]
        _, (source, _) = timed(res.make_source_map)
        packets = sum(len(run.X0) for run in inputs._catalogue)
        few = result(inputs, ctx, inputs._catalogue[:FEW])
        dev_ms, _ = timed(lambda: few.make_source_map(do_available=False))
        line = dict(npackets=n, outputs=len(inputs._catalogue), x0_packets=int(packets),
                    hits_per_packet=round(float(source.n_total.sum())/packets, 2),
                    make_source_map_ms=[round(v, 1) for v in ms],
                    few_outputs=FEW, device_source_only_ms=round(dev_ms, 1))
        if extra is not None:
            line.update(extra(few))
        print(json.dumps(line), flush=True)
        for run in inputs._catalogue:
            if getattr(run, '_store', None) is not None:
                run._store.free()
        inputs._catalogue = []
    ctx.close()


if __name__ == '__main__':
    main()
