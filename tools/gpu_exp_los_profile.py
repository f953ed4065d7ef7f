"""The line-of-sight pass with and without its profile, on the shape of bench.py's line-of-sight
side measurement: the resident float32 rows of the bench input (1e6 packets), 512 synthetic
spectra, dphi 1 degree; the profile has 64 bins over +-10 km/s.

The plain pass must not have changed, so it is measured against another build of the library
(``--parent-lib``: the parent commit's, built with tools/build_variant.py from a checkout of it).
One process loads one library, so every measurement is a child process of its own, run one after
the other and alternated: parent, this, parent, this (``--repeats`` each).  The parent's own
process-to-process spread is what this tree's plain pass is compared with.  A child makes the row
store, then runs 2 warm-up and 9 timed plain passes back to back -- the same calls in the same
order whichever library is loaded -- and, where the library has the entries, 2 + 9 rounds of one
plain and one profile pass for the ratio of the two.  A pass's figure is the HIP-event time of its
launches (nxc_last_kernel_ms: k_los_blocks + k_los + k_los_pairs).  No time is a gate.

    python tools/gpu_exp_los_profile.py [--parent-lib FILE] [--repeats 3] [--out FILE] [N]
    python tools/gpu_exp_los_profile.py --child [--passes K] [N]     one process, this library (or
                                        NEXOCLOM_HIP_LIB's); what a kernel trace is taken of

Each child prints one JSON line; the parent process prints them and a summary line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np                                            # noqa: E402

PROFILE_KMS, NV, S = (-10.0, 10.0), 64, 512
WARMUP, ROUNDS = 2, 9


def spread(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4),
            'max': round(float(np.max(ms)), 4)}


def child(n, passes):
    import bench
    from nexoclom_amd import Input, LOSResult, Output, SpacecraftData, hip_api
    from nexoclom_amd.LOSResult import arccos_threshold, los_geometry
    from nexoclom_amd.Output import n_output_steps
    ctx = hip_api.Context(0)
    inputs = Input(bench.INFILE)
    opt = inputs.options
    _, n_iter = n_output_steps(opt.endtime.value, opt.step_size)
    with bench.quiet():
        out = Output(inputs, n, seed=bench.SEED, integrate=False, save=False, context=ctx)
    ctx.set_forces(**out.forces_kwargs())
    ctx.upload_soa(out.x0_soa())
    store = ctx.integrate_const_rows(opt.step_size, n_iter, opt.outeredge, narrow=True,
                                     resident=True)['store']
    pos, look = bench.synthetic_orbit(S)
    sc = SpacecraftData(*pos.T, *look.T)
    with bench.quiet():
        los = LOSResult(sc, inputs, dphi=np.radians(1.0), context=ctx)
    dist, lengths, ladder = los_geometry(sc.data, opt.outeredge, los.dphi)
    scarr = np.vstack([pos.T, look.T, dist, lengths.astype(float)])
    args = (los.dphi, np.sin(los.dphi), np.sin(2*los.dphi), arccos_threshold(los.dphi),
            float(out.vrplanet_Rs()), out.unit_km*1e5, los.g_tables(float(out.aplanet)), ladder, scarr)
    rows = dict(rows=(store, 0, store.total, 0), n_index=out.npackets)
    has_profile = hasattr(ctx.lib, 'nxc_los_profile_enable')
    if has_profile:
        ctx.los_profile_enable(S, NV, PROFILE_KMS[0]/out.unit_km, PROFILE_KMS[1]/out.unit_km)
    times = {'plain': [], 'plain_beside_profile': [], 'profile': []}
    results = {}
    for rnd in range(0 if passes and has_profile else WARMUP + ROUNDS):
        results['plain'] = ctx.los_accumulate(*args, **rows)
        if rnd >= WARMUP:
            times['plain'].append(ctx.last_kernel_ms())
    for rnd in range((passes or WARMUP + ROUNDS) if has_profile else 0):
        for name in ('plain_beside_profile', 'profile'):
            results['profile' if name == 'profile' else 'plain'] = ctx.los_accumulate(
                *args, **rows, profile=name == 'profile')
            if passes or rnd >= WARMUP:
                times[name].append(ctx.last_kernel_ms())
    times['plain'] = times['plain'] or times['plain_beside_profile']
    line = {'lib': os.environ.get('NEXOCLOM_HIP_LIB', 'this tree'), 'npackets': n,
            'rows': int(store.total), 'spectra': S, 'dphi_deg': 1.0,
            'plain_ms': spread(times['plain']),
            'pairs_inside_cones': int(results['plain']['npackets'].sum()),
            'pairs_of_the_hottest_spectrum': int(results['plain']['npackets'].max())}
    if has_profile:
        plain, prof = results['plain'], results['profile']
        sums, moments = ctx.los_profile_download()
        done = len(times['profile']) + (0 if passes else WARMUP)
        assert np.array_equal(plain['npackets'], prof['npackets'])
        lit = plain['radiance'] > 0
        line.update(
            profile_ms=spread(times['profile']), profile_kms=list(PROFILE_KMS) + [NV],
            plain_beside_profile_ms=spread(times['plain_beside_profile']),
            profile_over_plain=round(float(np.median(times['profile']) /
                                           np.median(times['plain_beside_profile'])), 3),
            radiance_max_rel_diff=float(np.max(np.abs(prof['radiance'][lit]/plain['radiance'][lit] - 1))),
            records_over_radiance_max_rel_diff=float(np.max(np.abs(
                sums[lit, :, 0].sum(1)/(done*plain['radiance'][lit]) - 1))),
            weight_inside_the_range=round(float(sums[:, 1:-1, 0].sum()/sums[..., 0].sum()), 4))
        ctx.los_profile_enable(S, 0)
    store.free()
    ctx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--passes', type=int, default=0, help='child: this many rounds, all of them timed (a short run for a kernel trace)')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('n', nargs='?', type=float, default=1e6)
    args = ap.parse_args()
    n = int(args.n)
    if args.child:
        return child(n, args.passes)
    libs = ([args.parent_lib] if args.parent_lib else []) + [None]
    lines = []
    for _ in range(args.repeats):
        for lib in libs:
            env = dict(os.environ)
            env.pop('NEXOCLOM_HIP_LIB', None)
            if lib:
                env['NEXOCLOM_HIP_LIB'] = os.path.abspath(lib)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n)],
                                  env=env, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:       # a child that failed ends the experiment: nothing more is started
                sys.stderr.write(done.stdout + done.stderr)
                raise SystemExit(f'a child process failed with status {done.returncode}')
            lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(json.dumps(lines[-1]), flush=True)
    medians = {}
    for line in lines:
        medians.setdefault('parent' if line['lib'] != 'this tree' else 'this', []).append(
            line['plain_ms']['median'])
    summary = {'plain_ms_medians_per_process': medians}
    if 'parent' in medians:
        lo, hi = min(medians['parent']), max(medians['parent'])
        summary['parent_spread_ms'] = [lo, hi]
        summary['this_within_parent_spread'] = all(lo <= m <= hi for m in medians['this'])
        summary['this_over_parent'] = round(float(np.median(medians['this'])/np.median(medians['parent'])), 4)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(json.dumps(x) for x in lines + [summary]) + '\n')


if __name__ == '__main__':
    main()
