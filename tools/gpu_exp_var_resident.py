"""What leaving an adaptive-step run's final rows in HBM saves, end to end: Input.run(N) at
options.step_size = 0 + produce_image(512^2) + simulate_data_from_inputs over 512 lines of sight,
for a checkout of the parent commit (--parent DIR: its package and library) and for this tree, each
in a process of its own, 3 warm-up rounds and 7 timed ones; and the HIP-event time of
nxc_var_rows_build's two passes against the bytes they move at the box's k_stream_copy rate.
Appends one record to profiles/var_resident.jsonl.

usage: python tools/gpu_exp_var_resident.py [--parent DIR] [--n 1e7] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TIMED = 3, 7


def child(n):
    """Runs in the tree named by sys.path[0]: the rounds' wall times as one JSON line."""
    import contextlib
    import io
    import numpy as np
    import nexoclom_amd
    from nexoclom_amd import Input, LOSResult, SpacecraftData, hip_api
    infile = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                          'Na.mercury.bench.input')
    ctx = hip_api.Context(0)
    rng = np.random.default_rng(3)
    th = np.linspace(0, 2*np.pi, 512, endpoint=False)
    r = 1.6 + 1.2*rng.random(512)
    pos = np.stack([0.3*r*np.cos(th), r*np.sin(th)*0.6 - 0.4, r*np.sin(th)*0.8], 1)
    look = -pos + 0.6*rng.normal(size=pos.shape)
    look /= np.linalg.norm(look, axis=1)[:, None]
    sc = SpacecraftData(*pos.T, *look.T)
    rounds = []
    for k in range(WARM + TIMED):
        inputs = Input(infile)
        inputs.options.step_size = 0.
        inputs.options.resolution = 1e-4
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            inputs.run(n, seed=7, context=ctx)
            inputs.wait()
            t1 = time.perf_counter()
            image = inputs.produce_image({'quantity': 'radiance', 'dims': '512,512'}, context=ctx)
            t2 = time.perf_counter()
            los = LOSResult(sc, inputs, dphi=np.radians(1.0), context=ctx)
            los.simulate_data_from_inputs(sc)
            t3 = time.perf_counter()
        rounds.append({'run_s': t1 - t0, 'image_s': t2 - t1, 'los_s': t3 - t2, 'all_s': t3 - t0,
                       'resident': all(o.resident_rows(ctx) is not None
                                       for o in inputs._catalogue),
                       'counts': float(image.packet_image.sum()),
                       'radiance_sum': float(np.sum(los.radiance.values))})
        del inputs, image, los
    out = {'rounds': rounds[WARM:], 'device': ctx.device_name()}
    if hasattr(ctx, 'var_rows_build'):
        out['kernels'] = kernels(ctx, n)
    ctx.close()
    print('RESULT ' + json.dumps(out), flush=True)


def kernels(ctx, n):
    """HIP-event span of the two passes of nxc_var_rows_build over n packets (count: 8 B read per
    packet; write: 64 B read, 1 B kept flag and 40 B per kept packet written when narrow)."""
    import contextlib
    import io
    import nexoclom_amd
    from nexoclom_amd import Input, Output
    inputs = Input(os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                                'Na.mercury.bench.input'))
    inputs.options.step_size = 0.
    inputs.options.resolution = 1e-4
    with contextlib.redirect_stdout(io.StringIO()):
        out = Output(inputs, n, seed=5, integrate=False, save=False, context=ctx)
    ctx.set_forces(**out.forces_kwargs())
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_soa(out.x0_soa())
    ctx.integrate_var(1e-4, inputs.options.outeredge, resident=True)
    k_var_ms = ctx.last_kernel_ms()
    gbs = ctx.stream_copy_gbs()
    res = {'k_var_ms': k_var_ms, 'stream_copy_gbs': gbs}
    for narrow in (True, False):
        times = []
        for k in range(WARM + TIMED):
            store, kept = ctx.var_rows_build(narrow=narrow, compress=True)
            times.append(ctx.last_kernel_ms())
            total = store.total
            store.free()
        times = sorted(times[WARM:])
        moved = n*(8 + 64 + 1) + total*(40 if narrow else 80)
        res['narrow' if narrow else 'wide'] = {
            'span_ms_median': times[len(times)//2], 'span_ms_min': times[0], 'span_ms_max': times[-1],
            'kept': total, 'bytes_moved': moved, 'floor_ms': moved/(gbs*1e9)*1e3,
            'issue_floor_ms_104B': n*104/(gbs*1e9)*1e3}
    return res


def median(values):
    values = sorted(values)
    return values[len(values)//2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the parent commit, built')
    ap.add_argument('--n', type=float, default=1e7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'var_resident.jsonl'))
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, args.child)
        return child(int(args.n))
    record = {'what': 'Input.run + produce_image(512^2) + LOS(512) at step_size = 0',
              'n': int(args.n), 'warmup': WARM, 'timed': TIMED}
    for name, tree in (('parent', args.parent), ('tree', ROOT)):
        if tree is None:
            continue
        tree = os.path.abspath(tree)
        env = dict(os.environ, PYTHONPATH=tree)
        env.pop('NEXOCLOM_HIP_LIB', None)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, '--n',
                              str(args.n)], env=env, cwd=tree, capture_output=True, text=True,
                             timeout=1100)
        line = [ln for ln in res.stdout.splitlines() if ln.startswith('RESULT ')]
        if res.returncode != 0 or not line:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f'{name}: the measurement process failed ({res.returncode})')
        out = json.loads(line[-1][7:])
        rounds = out.pop('rounds')
        out['median_s'] = {k: median([r[k] for r in rounds]) for k in ('run_s', 'image_s', 'los_s', 'all_s')}
        out['spread_s'] = {k: [min(r[k] for r in rounds), max(r[k] for r in rounds)]
                           for k in ('run_s', 'image_s', 'los_s', 'all_s')}
        out['resident'] = all(r['resident'] for r in rounds)
        out['counts'], out['radiance_sum'] = rounds[-1]['counts'], rounds[-1]['radiance_sum']
        record[name] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as handle:
        handle.write(json.dumps(record) + '\n')
    print(json.dumps(record, indent=1))


if __name__ == '__main__':
    main()
