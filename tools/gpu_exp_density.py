"""ModelDensity over the catalogue of Input.run(N) (rows resident in HBM): wall time of the
whole call and k_density's own time (HIP events, summed over its launches), for a 1e4-point
trajectory and a 128^3 grid over [-4, 4]^3, dr = 0.05.  Prints one JSON line per case with the
two floors of DESIGN.md section 3: reading the rows (16 B per float32 row at 6.3 TB/s) and the
hits at 2.4e10 atomic requests/s (profiles/r01_ubench_atomics.txt).

    python tools/gpu_exp_density.py [N ...]          (default: 1e6 1e7)

``--moments [--out FILE]``: over the resident rows of Input.run(1e6), k_density and
k_density_moments alternated in one process on both point sets, 3 warm-up and 9 timed rounds each,
HIP-event time summed over the launches.  One JSON line per point set (appended to FILE) with the
moments' two floors: 28 B per float32 row at the box's k_stream_copy rate, and 6 requests per hit
at 2.4e10 requests/s.
"""
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                            # noqa: E402
from nexoclom_amd import Input, ModelDensity, hip_api          # noqa: E402
from nexoclom_amd.ModelDensity import DensityIndex             # noqa: E402
from nexoclom_amd.catalogue import sample_spans                # noqa: E402

HBM_BPS = 6.3e12
ATOMIC_RPS = 2.4e10
DR = 0.05


def point_sets():
    t = np.linspace(0, 1, 10_000)
    traj = np.stack([-4 + 8*t, -3 + 7*t, 0.8*np.sin(5*t)], axis=1)
    g = np.linspace(-4, 4, 128)
    grid = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing='ij')], axis=1)
    return {'trajectory_1e4': traj, 'grid_128^3': grid}


def spans(inputs, ctx):
    """The row ranges the classes launch over (adjacent slices of a store merged)."""
    return [span for _, span in sample_spans(inputs._catalogue, ctx)]


def kernel_ms(ctx, launches, accumulate):
    ms = 0.0
    for span in launches:
        accumulate(rows=span)
        ms += ctx.last_kernel_ms()
    return ms


def moments_leg(out_path, warm=3, timed=9):
    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs() * 1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(1e6, seed=7, context=ctx)
    launches = spans(inputs, ctx)
    rows = sum(s[2] for s in launches)
    for name, pts in point_sets().items():
        index = DensityIndex(pts, DR)
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                        index.dims)
        ctx.density_moments_enable()
        plain, moments = [], []
        for rep in range(warm + timed):
            a = kernel_ms(ctx, launches, ctx.density_accumulate)
            b = kernel_ms(ctx, launches, ctx.density_moments_accumulate)
            if rep >= warm:
                plain.append(a)
                moments.append(b)
        hits = float(ctx.density_download()[1].sum()) / (2*(warm + timed))
        line = json.dumps(dict(
            npackets=1e6, points=name, rows=rows, launches=len(launches), hits=hits,
            k_density_ms=[round(v, 3) for v in plain],
            k_density_moments_ms=[round(v, 3) for v in moments],
            stream_copy_gbs=round(copy_bps/1e9, 1),
            floor_rows_ms=round(rows*28/copy_bps*1e3, 3),
            floor_atomics_ms=round(6*hits/ATOMIC_RPS*1e3, 3)))
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')
    ctx.close()


def main():
    if '--moments' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
        return moments_leg(out)
    sizes = [float(a) for a in sys.argv[1:]] or [1e6, 1e7]
    ctx = hip_api.Context(0)
    for n in sizes:
        inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
        with contextlib.redirect_stdout(io.StringIO()):
            inputs.run(n, seed=7, context=ctx)
        launches = spans(inputs, ctx)
        rows = sum(s[2] for s in launches)
        for name, pts in point_sets().items():
            index = DensityIndex(pts, DR)
            ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                            index.dims)
            kernel_ms = []
            for rep in range(3):
                ms = 0.0
                for span in launches:
                    ctx.density_accumulate(rows=span)
                    ms += ctx.last_kernel_ms()
                kernel_ms.append(ms)
            hits = float(ctx.density_download()[1].sum())/3
            walls = []
            for rep in range(2):
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    d = ModelDensity(inputs, pts[:, 0], pts[:, 1], pts[:, 2], dr=DR, context=ctx)
                walls.append((time.perf_counter() - t0)*1e3)
            assert d.packets.sum() == hits
            print(json.dumps(dict(
                npackets=n, points=name, rows=rows, launches=len(launches), hits=hits,
                cells=int(np.prod(index.dims)), kernel_ms=[round(v, 3) for v in kernel_ms],
                modeldensity_ms=[round(v, 1) for v in walls],
                floor_rows_ms=round(rows*16/HBM_BPS*1e3, 3),
                floor_atomics_ms=round(hits/ATOMIC_RPS*1e3, 3))), flush=True)
        for run in inputs._catalogue:
            if run._store is not None:
                run._store.free()
        inputs._catalogue = []
    ctx.close()


if __name__ == '__main__':
    main()
