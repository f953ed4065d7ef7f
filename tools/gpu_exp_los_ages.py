"""The line-of-sight pass plain, with its profile and with its ages, on the scene of
tools/gpu_exp_los_profile.py: the resident float32 rows of the bench input (1e6 packets), 512
synthetic spectra, dphi 1 degree; the profile has 64 bins over +-10 km/s, the ages 64 bins over
[0, endtime).

The plain and the profile pass must not have changed, so they are measured against another build of
the library (``--parent-lib``: the parent commit's, built with tools/build_variant.py from a checkout
of it).  One process loads one library, so every measurement is a child process of its own, run one
after the other and alternated: parent, this, parent, this (``--repeats`` each).  The parent's own
process-to-process spread is what this tree's passes are compared with.  A child makes the row
store, then runs 2 warm-up and 9 timed plain passes back to back -- the same calls in the same
order whichever library is loaded --, then 2 + 9 rounds of one plain and one profile pass, again
the same for both libraries, and last (where the library has the entries) 2 + 9 rounds of one plain
and one ages pass.  A pass's figure is the HIP-event time of its launches
(nxc_last_kernel_ms: k_los_blocks + k_los + k_los_pairs).  No time is a gate.

The whole experiment runs under ``--time-limit`` seconds: a child gets what is left of them, and
one that outlasts them is killed and ends the experiment.

    python tools/gpu_exp_los_ages.py [--parent-lib FILE] [--repeats 3] [--out FILE] [N]
    python tools/gpu_exp_los_ages.py --child [N]        one process, this library (or
                                                        NEXOCLOM_HIP_LIB's)

Each child prints one JSON line; the parent process prints them and a summary line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np                                            # noqa: E402

PROFILE_KMS, NV, NA, S = (-10.0, 10.0), 64, 64, 512
WARMUP, ROUNDS = 2, 9


def spread(ms):
    return {'median': round(float(np.median(ms)), 4), 'min': round(float(np.min(ms)), 4),
            'max': round(float(np.max(ms)), 4)}


def child(n):
    import bench
    from nexoclom_amd import Input, LOSResult, Output, SpacecraftData, hip_api
    from nexoclom_amd.LOSResult import arccos_threshold, los_geometry
    from nexoclom_amd.Output import n_output_steps
    ctx = hip_api.Context(0)
    inputs = Input(bench.INFILE)
    opt = inputs.options
    endtime = float(opt.endtime.value)
    _, n_iter = n_output_steps(endtime, opt.step_size)
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
    has_ages = hasattr(ctx.lib, 'nxc_los_ages_enable')
    ctx.los_profile_enable(S, NV, PROFILE_KMS[0]/out.unit_km, PROFILE_KMS[1]/out.unit_km)
    if has_ages:
        ctx.los_ages_enable(S, NA, endtime, 0.0, endtime)
    modes = ('profile',) + (('ages',) if has_ages else ())
    times = {'plain': []}
    times.update({name: [] for mode in modes for name in ('plain_beside_' + mode, mode)})
    results = {}
    for rnd in range(WARMUP + ROUNDS):
        results['plain'] = ctx.los_accumulate(*args, **rows)
        if rnd >= WARMUP:
            times['plain'].append(ctx.last_kernel_ms())
    for mode in modes:
        for rnd in range(WARMUP + ROUNDS):
            for name, how in (('plain_beside_' + mode, {}), (mode, {mode: True})):
                results[name] = ctx.los_accumulate(*args, **rows, **how)
                if rnd >= WARMUP:
                    times[name].append(ctx.last_kernel_ms())
    plain = results['plain']
    lit = plain['radiance'] > 0
    done = WARMUP + ROUNDS
    line = {'lib': os.environ.get('NEXOCLOM_HIP_LIB', 'this tree'), 'npackets': n,
            'rows': int(store.total), 'spectra': S, 'dphi_deg': 1.0,
            'plain_ms': spread(times['plain']),
            'plain_beside_profile_ms': spread(times['plain_beside_profile']),
            'profile_ms': spread(times['profile']), 'profile_kms': list(PROFILE_KMS) + [NV],
            'pairs_inside_cones': int(plain['npackets'].sum()),
            'pairs_of_the_hottest_spectrum': int(plain['npackets'].max())}
    sums, _ = ctx.los_profile_download()
    assert np.array_equal(plain['npackets'], results['profile']['npackets'])
    line['profile_records_over_radiance_max_rel_diff'] = float(np.max(np.abs(
        sums[lit, :, 0].sum(1)/(done*plain['radiance'][lit]) - 1)))
    ctx.los_profile_enable(S, 0)
    if has_ages:
        aged = results['ages']
        sums = ctx.los_ages_download()
        assert np.array_equal(plain['npackets'], aged['npackets'])
        line.update(
            ages_ms=spread(times['ages']), ages_s=[0.0, endtime, NA],
            plain_beside_ages_ms=spread(times['plain_beside_ages']),
            ages_over_plain=round(float(np.median(times['ages']) /
                                        np.median(times['plain_beside_ages'])), 3),
            ages_over_profile=round(float(np.median(times['ages'])/np.median(times['profile'])), 3),
            ages_radiance_max_rel_diff=float(np.max(np.abs(aged['radiance'][lit]/plain['radiance'][lit] - 1))),
            ages_records_over_radiance_max_rel_diff=float(np.max(np.abs(
                sums[lit, :, 0].sum(1)/(done*plain['radiance'][lit]) - 1))),
            ages_weight_inside_the_range=round(float(sums[:, 1:-1, 0].sum()/sums[..., 0].sum()), 4),
            ages_bins_filled=int(np.count_nonzero(sums[:, 1:-1, 0].sum(0))))
        ctx.los_ages_enable(S, 0)
    store.free()
    ctx.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--time-limit', type=float, default=900.0, help='seconds for the whole experiment')
    ap.add_argument('--out', default=None)
    ap.add_argument('n', nargs='?', type=float, default=1e6)
    args = ap.parse_args()
    n = int(args.n)
    if args.child:
        return child(n)
    deadline = time.monotonic() + args.time_limit
    libs = ([args.parent_lib] if args.parent_lib else []) + [None]
    lines = []
    for _ in range(args.repeats):
        for lib in libs:
            env = dict(os.environ)
            env.pop('NEXOCLOM_HIP_LIB', None)
            if lib:
                env['NEXOCLOM_HIP_LIB'] = os.path.abspath(lib)
            left = deadline - time.monotonic()
            if left <= 0:
                raise SystemExit('the time limit ran out: nothing more is started')
            try:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n)],
                                      env=env, capture_output=True, text=True, timeout=left)
            except subprocess.TimeoutExpired:
                raise SystemExit('a child process outlasted the time limit and was killed') from None
            if done.returncode != 0:       # a child that failed ends the experiment: nothing more is started
                sys.stderr.write(done.stdout + done.stderr)
                raise SystemExit(f'a child process failed with status {done.returncode}')
            lines.append(json.loads(done.stdout.strip().splitlines()[-1]))
            print(json.dumps(lines[-1]), flush=True)
    summary = {}
    for what in ('plain_ms', 'profile_ms'):
        medians = {}
        for line in lines:
            medians.setdefault('parent' if line['lib'] != 'this tree' else 'this', []).append(
                line[what]['median'])
        entry = {'medians_per_process': medians}
        if 'parent' in medians:
            lo, hi = min(medians['parent']), max(medians['parent'])
            entry['parent_spread_ms'] = [lo, hi]
            entry['this_within_parent_spread'] = all(lo <= m <= hi for m in medians['this'])
            entry['this_over_parent'] = round(float(np.median(medians['this'])/np.median(medians['parent'])), 4)
        summary[what] = entry
    summary['ages_ms_medians_per_process'] = [line['ages_ms']['median'] for line in lines if 'ages_ms' in line]
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(json.dumps(x) for x in lines + [summary]) + '\n')


if __name__ == '__main__':
    main()
