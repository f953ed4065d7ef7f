"""LOSResultFitted over the catalogue of Input.run(N) (rows resident in HBM), 512 spectra around the
planet, dphi = 1 deg: wall times of simulate_data_from_inputs and of determine_source_from_data
(its own unfitted pair pass included), the number of used pairs and of fitted rows.  Prints one
JSON line per size.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR --`
(k_fit_packets, k_fit_norm, k_fit_radiance, k_fit_rows_count, k_fit_rows_write next to k_los*).

    python tools/gpu_exp_fitted.py [N ...]          (default: 1e6 1e7)
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                    # noqa: E402
from nexoclom_amd import Input, LOSResult, LOSResultFitted, SpacecraftData, hip_api   # noqa: E402

NSPEC = 512


def spacecraft(**columns):
    rng = np.random.default_rng(13)
    th = np.linspace(0, 2*np.pi, NSPEC, endpoint=False)
    r = 1.6 + 1.2*rng.random(NSPEC)
    pos = np.stack([0.3*r*np.cos(th), r*np.sin(th)*0.6 - 0.4, r*np.sin(th)*0.8], 1)
    look = rng.normal(size=(NSPEC, 3))
    look[::3] = -pos[::3] + 0.9*rng.normal(size=(len(pos[::3]), 3))
    look /= np.linalg.norm(look, axis=1)[:, None]
    return SpacecraftData(*pos.T, *look.T, **columns)


def timed(fn):
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        fn()
    return (time.perf_counter() - t0)*1e3


def main():
    sizes = [float(a) for a in sys.argv[1:]] or [1e6, 1e7]
    ctx = hip_api.Context(0)
    for n in sizes:
        inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
        with contextlib.redirect_stdout(io.StringIO()):
            inputs.run(n, seed=7, context=ctx)
        rows = sum(run.resident_rows(ctx)[2] for run in inputs._catalogue)
        probe = LOSResult(spacecraft(), inputs, dphi=np.radians(1.), context=ctx)
        sim_ms = [timed(lambda: probe.simulate_data_from_inputs(spacecraft())) for _ in range(2)]
        rng = np.random.default_rng(3)
        sc = spacecraft(radiance=probe.radiance.values*rng.uniform(0.5, 1.5, NSPEC),
                        sigma=np.ones(NSPEC))
        los = LOSResult(sc, inputs, dphi=np.radians(1.), context=ctx, label='unfit')
        with contextlib.redirect_stdout(io.StringIO()):
            los.simulate_data_from_inputs(sc)
        los.determine_source_rate(sc, use_weight=False)
        sc.add_model_result(los, 'unfit')
        fit_ms, fitted = [], None
        for rep in range(2):
            fitted = LOSResultFitted(sc, 'unfit', dphi=np.radians(1.), context=ctx)
            fit_ms.append(timed(lambda: fitted.determine_source_from_data(sc, use_weight='dist')))
            if rep == 0:
                for run in fitted.inputs._catalogue:       # the first call's fitted rows go
                    if run._store is not None:
                        run._store.free()
        pairs = int(sum(it['n_pairs'] for it in fitted.iterations))
        bound = int(sum(int(it['npackets'].sum()) for it in los.iterations))
        fitted_rows = sum(run._nrows for run in fitted.inputs._catalogue)
        print(json.dumps(dict(
            npackets=n, outputs=len(inputs._catalogue), rows=rows, spectra=NSPEC,
            used_pairs=pairs, pair_bound=bound, fitted_rows=int(fitted_rows),
            simulate_ms=[round(v, 1) for v in sim_ms],
            determine_source_from_data_ms=[round(v, 1) for v in fit_ms],
            finite=bool(all(np.isfinite(it['multiplier']).all() for it in fitted.iterations)))),
            flush=True)
        for result in (fitted.inputs, inputs):
            for run in result._catalogue:
                if run._store is not None:
                    run._store.free()
            result._catalogue = []
    ctx.close()


if __name__ == '__main__':
    main()
