#!/usr/bin/env python3
"""k_sample at 1e7 packets for thermal launch speeds against the two speed laws it sits beside.

Three sources, alternated in one process so that they see the same clocks: uniform surface with
(a) flat speeds, (b) a constant-temperature Maxwellian (the 5000-point inverse-CDF table) and (c)
thermal speeds (speed_type 3: the surface temperature and the bicubic v(T, p) spline per packet).
Per source: 3 warm-up calls, then the HIP-event time of the k_sample launch (nxc_last_kernel_ms)
of 15 calls; median, minimum and maximum as one JSON line each.

    python tools/gpu_exp_thermal_sampler.py [--existing-only] [--tag NAME]

``--existing-only`` times (a) and (b) alone: with NEXOCLOM_HIP_LIB naming the parent commit's
library it gives the no-regression baseline of the two existing sources.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nexoclom_amd import Input, hip_api                                   # noqa: E402
from nexoclom_amd.source_distribution import density_cdf, tabulated_speed_density   # noqa: E402
from nexoclom_amd.surface import (NIGHT_SIDE_K, day_side_t1, spline_tables,          # noqa: E402
                                  thermal_launch_spline)

N, WARM, REPS = 10_000_000, 3, 15


def main():
    tag = sys.argv[sys.argv.index('--tag') + 1] if '--tag' in sys.argv else 'this build'
    base = dict(endtime=50000., exobase=1.0, unit_km=2440.53, random_time=0, angular_type=1,
                is_planet=1, sinlat0=-1.0, sinlat1=1.0, lon0=0.0, lon1=2*np.pi, vprob=2.5,
                vwidth=2.0, sinalt0=0.0, sinalt1=1.0, az0=0.0, az1=2*np.pi, spatial_type=0)
    inputs = Input(os.path.join(ROOT, 'nexoclom_amd', 'inputfiles', 'Na.mercury.thermal.input'))
    vd = inputs.speeddist
    vd.temperature = type(vd.temperature)(1500., 'K')
    maxwell = density_cdf(*tabulated_speed_density(vd, 'Na'))
    sources = {'uniform+flat': dict(base, speed_type=0),
               'uniform+maxwellian_1500K': dict(base, speed_type=2, speed_table=maxwell)}
    if '--existing-only' not in sys.argv:
        sources['uniform+thermal'] = dict(
            base, speed_type=3, t0=NIGHT_SIDE_K, t1=float(day_side_t1(inputs.geometry)),
            thermal_spline=spline_tables(thermal_launch_spline(inputs)))
    ctx = hip_api.Context(0)
    times = {name: [] for name in sources}
    for rep in range(WARM + REPS):
        for name, src in sources.items():
            ctx.sample_packets(N, 1234, 0, **src)
            if rep >= WARM:
                times[name].append(ctx.last_kernel_ms())
    for name, ms in times.items():
        print(json.dumps({'kernel': 'k_sample', 'build': tag, 'source': name, 'packets': N,
                          'reps': REPS, 'median_ms': float(np.median(ms)), 'min_ms': min(ms),
                          'max_ms': max(ms), 'all_ms': [round(float(t), 5) for t in ms]}))
    ctx.close()


if __name__ == '__main__':
    main()
