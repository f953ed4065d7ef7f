"""k_shell against k_image_moments over the same resident rows: the catalogue of Input.run(1e6)
(1.3e8 float32 rows in HBM); ShellMap radiance on 72 x 36 cells with 32 altitude bins over 0..4 R,
ModelImage radiance with moments on 512 x 512 pixels (8 x 8 R).  Both kernels make one atomic
request per binned sample and two more for a binned sample with w != 0.  One process; the two
kernels are alternated, 3 warm-up rounds and 9 timed ones; a round's figure is the HIP-event time
(nxc_last_kernel_ms) summed over the launches.  One JSON line (appended to ``--out FILE``) with
median [min, max] per kernel, the requests each makes, its requests/s, and k_shell's two floors:

  bytes    20 B per float32 row at the box's k_stream_copy rate measured in the same run;
  atomics  its requests at the 2.4e10 requests/s of profiles/r01_ubench_atomics.txt.

The samples with w != 0 are counted on the host from the rows' positions, in float32, as
tools/gpu_exp_image_moments.py does.  The line also says how unevenly the shell map's requests
fall on its records (the share of the busiest cell and of the busiest record), and k_shell's time
over the same rows on a finer grid (720 x 360 x 32) and on coarser ones (72 x 36 x 1, 8 x 4 x 4):
the requests are the same, the records they fall on are not.  No time is a gate.

    python tools/gpu_exp_shell_map.py [--out FILE] [N]          (default: 1e6)

``--moments``: k_shell against k_shell_moments (ShellMap(moments=True)) instead, alternated in the
same way over the same rows, on 72 x 36 x 32 and on 720 x 360 x 32: per grid and kernel median
[min, max], the requests (k_shell_moments: six more per sample with w != 0), requests/s and the
share of the atomic floor in the kernel's time.

    python tools/gpu_exp_shell_map.py --moments [--out FILE] [N]

``--ages``: k_shell against k_shell_ages (ShellMap(ages=...), 32 age bins over the run) in the same
way, 1 warm-up round and 10 timed ones, on 72 x 36 x 32 and on 720 x 360 x 1: per grid and kernel
median [min, max], the requests (k_shell_ages: two more per sample with w != 0, five in all),
requests/s, the atomic floor and its share of the kernel's time, and the bytes of the block.

    python tools/gpu_exp_shell_map.py --ages [--out FILE] [N]
"""
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools')]
import numpy as np                                            # noqa: E402
from gpu_exp_image_moments import ATOMIC_RPS, CHUNK, ROUNDS, WARMUP, spread   # noqa: E402
from nexoclom_amd import Input, ModelImage, ShellMap, hip_api   # noqa: E402
from nexoclom_amd.catalogue import sample_spans                    # noqa: E402


SWEEP = (('720,360', '0,4,32'), ('72,36', '0,4,1'), ('8,4', '0,4,4'))


def lit_counts(launches, image):
    """Samples with w != 0: of the shell map (sunlit, away from the centre) and binned by the image"""
    M = image.image_rotation().astype(np.float32)
    count = {'shell': 0, 'image': 0}
    for store, first, total in launches:
        for at in range(first, first + total, CHUNK):
            rows, _ = store.download(at, min(CHUNK, first + total - at), index=False)
            x, y, z = rows[1], rows[2], rows[3]
            sunlit = (x*x + z*z > 1) | (y < 0)
            count['shell'] += int(np.count_nonzero(sunlit & (x*x + y*y + z*z > 0)))
            xo, yo, zo = (M[r, 0]*x + M[r, 1]*y + M[r, 2]*z for r in range(3))
            inside = (xo >= image.xedges[0]) & (xo <= image.xedges[-1]) \
                & (zo >= image.zedges[0]) & (zo <= image.zedges[-1])
            count['image'] += int(np.count_nonzero(inside & sunlit & ((xo*xo + zo*zo > 1) | (yo < 0))))
    return count


MOMENT_GRIDS = (('72,36', '0,4,32'), ('720,360', '0,4,32'))


def main_moments(n, out_path):
    """``--moments``: k_shell against k_shell_moments over the same resident rows, alternated, on
    the two grids of the table above.  k_shell makes one request per binned sample and two more
    for one with w != 0; k_shell_moments makes six more for those (the samples exactly on the polar
    axis, which make none of the six, are not told apart: none is expected among float32 rows)."""
    ctx = hip_api.Context(0)
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    lit = 0
    for store, first, total in launches:
        for at in range(first, first + total, CHUNK):
            got, _ = store.download(at, min(CHUNK, first + total - at), index=False)
            x, y, z = got[1], got[2], got[3]
            lit += int(np.count_nonzero(((x*x + z*z > 1) | (y < 0)) & (x*x + y*y + z*z > 0)))
    kernels = {'k_shell': lambda span: ctx.shell_accumulate(rows=span),
               'k_shell_moments': lambda span: ctx.shell_moments_accumulate(rows=span)}
    grids = {}
    for dims, altitude in MOMENT_GRIDS:
        params = dict(quantity='radiance', dims=dims, altitude=altitude)
        with contextlib.redirect_stdout(io.StringIO()):
            # the class checks the whole path once and leaves its description set and enabled
            ShellMap(inputs, params, context=ctx, moments=True)
        times = {name: [] for name in kernels}
        binned = {}
        for rnd in range(WARMUP + ROUNDS):
            for name, accumulate in kernels.items():
                ms, hit = 0.0, 0
                for span in launches:
                    accumulate(span)
                    ms += ctx.last_kernel_ms()
                    hit += ctx.counters()['samples_binned']
                binned[name] = hit
                if rnd >= WARMUP:
                    times[name].append(ms)
        med = {name: float(np.median(t)) for name, t in times.items()}
        requests = {'k_shell': binned['k_shell'] + 2*lit,
                    'k_shell_moments': binned['k_shell_moments'] + 8*lit}
        grids[f'{dims} x {altitude.split(",")[2]}'] = {
            'binned': binned, 'requests': requests,
            **{name + '_ms': spread(t) for name, t in times.items()},
            'moments_over_shell': round(med['k_shell_moments']/med['k_shell'], 3),
            'requests_per_s': {name: round(requests[name]/med[name]*1e3, 0) for name in kernels},
            'atomic_floor_ms': {name: round(requests[name]/ATOMIC_RPS*1e3, 3) for name in kernels},
            'floor_share_of_kernel_time': {name: round(requests[name]/ATOMIC_RPS*1e3/med[name], 3)
                                           for name in kernels}}
    line = json.dumps({'npackets': n, 'rows': rows, 'launches': len(launches),
                       'binned_nonzero': lit, 'warmup': WARMUP, 'rounds': ROUNDS, 'grids': grids})
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')
    ctx.close()


AGE_GRIDS = (('72,36', '0,4,32'), ('720,360', '0,4,1'))
AGE_BINS = 32


def main_ages(n, out_path, warmup=1, rounds=10):
    """``--ages``: k_shell against k_shell_ages over the same resident rows, alternated, on the two
    grids above.  k_shell makes one request per binned sample and two more for one with w != 0;
    k_shell_ages makes two more again for those, to (nbins + 2) times as many records."""
    ctx = hip_api.Context(0)
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    lit = 0
    for store, first, total in launches:
        for at in range(first, first + total, CHUNK):
            got, _ = store.download(at, min(CHUNK, first + total - at), index=False)
            x, y, z = got[1], got[2], got[3]
            lit += int(np.count_nonzero(((x*x + z*z > 1) | (y < 0)) & (x*x + y*y + z*z > 0)))
    kernels = {'k_shell': lambda span: ctx.shell_accumulate(rows=span),
               'k_shell_ages': lambda span: ctx.shell_ages_accumulate(rows=span)}
    endtime = float(inputs.options.endtime.value)
    grids = {}
    for dims, altitude in AGE_GRIDS:
        params = dict(quantity='radiance', dims=dims, altitude=altitude)
        with contextlib.redirect_stdout(io.StringIO()):
            # the class checks the whole path once and leaves its description set and enabled
            sm = ShellMap(inputs, params, context=ctx, ages=(0., endtime, AGE_BINS))
        times = {name: [] for name in kernels}
        binned = {}
        for rnd in range(warmup + rounds):
            for name, accumulate in kernels.items():
                ms, hit = 0.0, 0
                for span in launches:
                    accumulate(span)
                    ms += ctx.last_kernel_ms()
                    hit += ctx.counters()['samples_binned']
                binned[name] = hit
                if rnd >= warmup:
                    times[name].append(ms)
        med = {name: float(np.median(t)) for name, t in times.items()}
        requests = {'k_shell': binned['k_shell'] + 2*lit,
                    'k_shell_ages': binned['k_shell_ages'] + 4*lit}
        grids[f'{dims} x {altitude.split(",")[2]}'] = {
            'age_bins': AGE_BINS, 'block_bytes': int(sm.shell_age_sums.size*8),
            'binned': binned, 'requests': requests,
            **{name + '_ms': spread(t) for name, t in times.items()},
            'ages_over_shell': round(med['k_shell_ages']/med['k_shell'], 3),
            'requests_per_s': {name: round(requests[name]/med[name]*1e3, 0) for name in kernels},
            'atomic_floor_ms': {name: round(requests[name]/ATOMIC_RPS*1e3, 3) for name in kernels},
            'floor_share_of_kernel_time': {name: round(requests[name]/ATOMIC_RPS*1e3/med[name], 3)
                                           for name in kernels}}
    line = json.dumps({'npackets': n, 'rows': rows, 'launches': len(launches),
                       'binned_nonzero': lit, 'warmup': warmup, 'rounds': rounds, 'grids': grids})
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')
    ctx.close()


def main():
    args = sys.argv[1:]
    out_path = None
    if '--out' in args:
        out_path = args[args.index('--out') + 1]
        del args[args.index('--out'):args.index('--out') + 2]
    moments = '--moments' in args
    if moments:
        args.remove('--moments')
    ages = '--ages' in args
    if ages:
        args.remove('--ages')
    n = float(args[0]) if args else 1e6
    if moments:
        return main_moments(n, out_path)
    if ages:
        return main_ages(n, out_path)
    ctx = hip_api.Context(0)
    copy_bps = ctx.stream_copy_gbs()*1e9
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.bench.input'))
    image_params = dict(quantity='radiance', dims='512,512', width='8,8')
    shell_params = dict(quantity='radiance', dims='72,36', altitude='0,4,32')
    with contextlib.redirect_stdout(io.StringIO()):
        inputs.run(n, seed=7, context=ctx)
        # the classes check the whole path once and leave their descriptions set
        shell = ShellMap(inputs, shell_params, context=ctx)
        image = ModelImage(inputs, image_params, context=ctx, moments=True)
    launches = [span for _, span in sample_spans(inputs._catalogue, ctx)]
    rows = sum(s[2] for s in launches)
    lit = lit_counts(launches, image)
    kernels = {'k_image_moments': lambda span: ctx.image_moments_accumulate(rows=span),
               'k_shell': lambda span: ctx.shell_accumulate(rows=span)}
    times = {name: [] for name in kernels}
    binned = {}
    for rnd in range(WARMUP + ROUNDS):
        for name, accumulate in kernels.items():
            ms, hit = 0.0, 0
            for span in launches:
                accumulate(span)
                ms += ctx.last_kernel_ms()
                hit += ctx.counters()['samples_binned']
            binned[name] = hit
            if rnd >= WARMUP:
                times[name].append(ms)
    med = {name: float(np.median(t)) for name, t in times.items()}
    requests = {'k_image_moments': binned['k_image_moments'] + 2*lit['image'],
                'k_shell': binned['k_shell'] + 2*lit['shell']}
    floors = dict(bytes_ms=round(20*rows/copy_bps*1e3, 3),
                  atomics_ms=round(requests['k_shell']/ATOMIC_RPS*1e3, 3))
    binds = max(floors, key=floors.get)
    weights = shell.shell_sums[0, ..., 0]
    # the same rows on other grids: the requests stay, the records they fall on change
    sweep = {}
    for dims, altitude in SWEEP:
        with contextlib.redirect_stdout(io.StringIO()):
            ShellMap(inputs, dict(shell_params, dims=dims, altitude=altitude), context=ctx)
        ms = []
        for rnd in range(WARMUP + ROUNDS):
            ms.append(0.0)
            for span in launches:
                ctx.shell_accumulate(rows=span)
                ms[-1] += ctx.last_kernel_ms()
        sweep[f'{dims} x {altitude.split(",")[2]}'] = spread(ms[WARMUP:])
    line = json.dumps({
        'npackets': n, 'rows': rows, 'launches': len(launches), 'shell': [72, 36, 32],
        'image_dims': [512, 512], 'binned': binned, 'binned_nonzero': lit, 'requests': requests,
        **{name + '_ms': spread(t) for name, t in times.items()},
        'shell_over_image_moments': round(med['k_shell']/med['k_image_moments'], 3),
        'requests_per_s': {name: round(requests[name]/med[name]*1e3, 0) for name in kernels},
        'k_shell_on_other_grids_ms': sweep,
        'busiest_cell_share_of_packets': round(float(shell.packets.max()/shell.packets.sum()), 5),
        'busiest_record_share_of_weight': round(float(weights.max()/weights.sum()), 5),
        'stream_copy_gbs': round(copy_bps/1e9, 1), 'floors': floors, 'binding_floor': binds,
        'floor_share_of_kernel_time': round(floors[binds]/med['k_shell'], 3)})
    print(line, flush=True)
    if out_path:
        with open(out_path, 'a') as f:
            f.write(line + '\n')
    ctx.close()


if __name__ == '__main__':
    main()
