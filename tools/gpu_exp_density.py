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

``--spectrum [--out FILE]``: the same with k_density, k_density_moments and k_density_spectrum
alternated: the trajectory seen through a ram cone of 30 degrees (the spacecraft flies along it at
3 km/s) in 32 bins, the grid with the whole sky in 16 bins (2.1e6 x 18 x 32 B = 1.2 GB of records).
Median and [min, max] per kernel, and the spectrum's two floors: 28 B per row plus 64 B per hit (the
frame record) at the k_stream_copy rate, and one request per hit plus two per seen hit at 2.4e10
requests/s.  The seen hits of the cone are counted by one more pass over the same rows with
frac = 1 (downloaded and handed back as host columns), where plane 0 of the spectrum holds them.

``--ages [--out FILE]``: the same with k_density, k_density_spectrum (whole sky, 16 bins) and
k_density_ages (16 age bins over the run) alternated, and on the grid k_ages_apply for 1 and 64
epochs (2 warm-up and 5 timed calls).  The ages' floors: 12 B of position per float32 row and 20 B
where the cull passes it, at the k_stream_copy rate, and two requests per hit at 2.4e10 requests/s.
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


def spread(values):
    return dict(median=round(float(np.median(values)), 3), min=round(min(values), 3),
                max=round(max(values), 3))


def spectrum_cases(unit_km):
    """Per point set: (nv, s_lo, s_hi [R/s], cos_half, all_sky, frames in the points' order)."""
    sets = point_sets()
    traj = sets['trajectory_1e4']
    tangent = np.gradient(traj, axis=0)
    u = 3.0/unit_km * tangent/np.linalg.norm(tangent, axis=1)[:, None]
    ram = np.zeros((len(traj), 8))
    ram[:, 0:3] = u
    ram[:, 4:7] = u/np.linalg.norm(u, axis=1)[:, None]
    return {'trajectory_1e4': (32, 0.0, 8.0/unit_km, float(np.cos(np.radians(30.))), False, ram),
            'grid_128^3': (16, 0.0, 8.0/unit_km, -1.0, True, np.zeros((len(sets['grid_128^3']), 8)))}


def seen_hits(ctx, launches, chunk=1 << 23):
    """Rows seen per point and plane, summed: the enabled (zeroed) spectrum after a pass over the
    rows of ``launches`` with frac = 1, handed over as host columns chunk by chunk."""
    for store, first, count in launches:
        for off in range(0, count, chunk):
            n = min(chunk, count - off)
            rows, _ = store.download(first + off, n, index=False)
            ctx.density_spectrum_accumulate(*rows[1:7], np.ones(n, dtype=rows.dtype))
    return float(ctx.density_spectrum_download()[0, :, :, 0].sum())


def spectrum_leg(out_path, warm=3, timed=9):
    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs() * 1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(1e6, seed=7, context=ctx)
    launches = spans(inputs, ctx)
    rows = sum(s[2] for s in launches)
    cases = spectrum_cases(float(inputs.geometry.planet.radius.value))
    for name, pts in point_sets().items():
        index = DensityIndex(pts, DR)
        nv, s_lo, s_hi, cos_half, all_sky, frames = cases[name]
        enable = lambda: ctx.density_spectrum_enable(nv, s_lo, s_hi, cos_half, all_sky,  # noqa: E731
                                                     frames[index.order])
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                        index.dims)
        ctx.density_moments_enable()
        enable()
        times = {'k_density': [], 'k_density_moments': [], 'k_density_spectrum': []}
        passes = (ctx.density_accumulate, ctx.density_moments_accumulate,
                  ctx.density_spectrum_accumulate)
        for rep in range(warm + timed):
            for key, accumulate in zip(times, passes):
                ms = kernel_ms(ctx, launches, accumulate)
                if rep >= warm:
                    times[key].append(ms)
        hits = float(ctx.density_download()[1].sum()) / (3*(warm + timed))
        ctx.density_moments_enable(False)
        if all_sky:
            seen = hits
        else:
            enable()
            seen = seen_hits(ctx, launches)
        record = dict(npackets=1e6, points=name, rows=rows, launches=len(launches), hits=hits,
                      seen_hits=seen, nv=nv, all_sky=all_sky,
                      record_bytes=2*len(index.points)*(nv + 2)*16,
                      stream_copy_gbs=round(copy_bps/1e9, 1),
                      floor_bytes_ms=round((rows*28 + hits*64)/copy_bps*1e3, 3),
                      floor_atomics_ms=round((hits + 2*seen)/ATOMIC_RPS*1e3, 3))
        for key, values in times.items():
            record[key + '_ms'] = [round(v, 3) for v in values]
            record[key] = spread(values)
        line = json.dumps(record)
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')
        ctx.density_spectrum_enable(0)
    ctx.close()


def ages_leg(out_path, warm=3, timed=9, na=16):
    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs() * 1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(1e6, seed=7, context=ctx)
    launches = spans(inputs, ctx)
    rows = sum(s[2] for s in launches)
    t0 = float(inputs.options.endtime.value)
    unit_km = float(inputs.geometry.planet.radius.value)
    for name, pts in point_sets().items():
        index = DensityIndex(pts, DR)
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                        index.dims)
        ctx.density_spectrum_enable(na, 0.0, 8.0/unit_km)            # the whole sky, 16 bins
        ctx.density_ages_enable(na, t0, 0.0, t0)
        times = {'k_density': [], 'k_density_spectrum': [], 'k_density_ages': []}
        passes = (ctx.density_accumulate, ctx.density_spectrum_accumulate,
                  ctx.density_ages_accumulate)
        for rep in range(warm + timed):
            for key, accumulate in zip(times, passes):
                ms = kernel_ms(ctx, launches, accumulate)
                if rep >= warm:
                    times[key].append(ms)
        hits = float(ctx.density_download()[1].sum()) / (3*(warm + timed))
        ctx.density_spectrum_enable(0)
        record = dict(npackets=1e6, points=name, rows=rows, launches=len(launches), hits=hits,
                      na=na, record_bytes=len(index.points)*(na + 2)*16,
                      stream_copy_gbs=round(copy_bps/1e9, 1),
                      # 12 B of position per float32 row, 20 B where the cull passes it
                      floor_bytes_ms=[round(rows*b/copy_bps*1e3, 3) for b in (12, 20)],
                      floor_atomics_ms=round(2*hits/ATOMIC_RPS*1e3, 3))
        for key, values in times.items():
            record[key + '_ms'] = [round(v, 3) for v in values]
            record[key] = spread(values)
        if name.startswith('grid'):            # transient(): the block contracted for 1 and 64 epochs
            for ne in (1, 64):
                K = np.ones((na + 2, ne))
                apply_ms = []
                for rep in range(2 + 5):
                    ctx.density_ages_apply(K)
                    if rep >= 2:
                        apply_ms.append(ctx.last_kernel_ms())
                record[f'k_ages_apply_{ne}_ms'] = [round(v, 3) for v in apply_ms]
                record[f'k_ages_apply_{ne}'] = spread(apply_ms)
        line = json.dumps(record)
        print(line, flush=True)
        if out_path:
            with open(out_path, 'a') as f:
                f.write(line + '\n')
        ctx.density_ages_enable(0)
    ctx.close()


def main():
    if '--ages' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
        return ages_leg(out)
    if '--spectrum' in sys.argv:
        out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
        return spectrum_leg(out)
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
