#!/usr/bin/env python3
"""k_sample at 1e7 packets for the surface-map source against the uniform one.

Three sources, alternated in one process so that they see the same clocks: (a) uniform, (b) a
181 x 91 map with one sharp peak and 99 % of its cells empty, (c) a flat map of the same size.
Per source: 3 warm-up calls, then the HIP-event time of the k_sample launch (nxc_last_kernel_ms)
of 15 calls; median, minimum and maximum as one JSON line each.  The work per packet of the map
source does not depend on the map (one bisection of the cell cdf, two linear inversions), so (b)
and (c) should agree; if (b) were several times (c), the bisection's memory pattern would be the
thing to look at.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nexoclom_amd import hip_api                                          # noqa: E402
from nexoclom_amd.source_distribution import surface_map_cells            # noqa: E402

N, WARM, REPS = 10_000_000, 3, 15


def peaked(longitude, latitude):
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    a = np.exp(-0.5*(((lon - 2.0)/0.05)**2 + ((lat - 0.4)/0.05)**2))
    a[np.abs(lon - 2.0) > 0.17] = 0.0
    a[np.abs(lat - 0.4) > 0.17] = 0.0
    return a


def main():
    base = dict(endtime=50000., exobase=1.0, unit_km=2440.53, random_time=0, angular_type=1,
                is_planet=1, sinlat0=-1.0, sinlat1=1.0, lon0=0.0, lon1=2*np.pi, vprob=2.5,
                vwidth=2.0, sinalt0=0.0, sinalt1=1.0, az0=0.0, az1=2*np.pi, speed_type=0)
    longitude = np.linspace(0, 2*np.pi, 181)
    latitude = np.linspace(-np.pi/2, np.pi/2, 91)
    sources = {'uniform': dict(base, spatial_type=0)}
    for name, nodes in (('map_peaked', peaked(longitude, latitude)),
                        ('map_flat', np.ones((181, 91)))):
        cdf, (lon0, lon1, s0, s1) = surface_map_cells(longitude, latitude, nodes)
        sources[name] = dict(base, spatial_type=2, map_nodes=nodes, map_cdf=cdf, map_lon0=lon0,
                             map_lon1=lon1, map_s0=s0, map_s1=s1)
    ctx = hip_api.Context(0)
    times = {name: [] for name in sources}
    for rep in range(WARM + REPS):
        for name, src in sources.items():
            ctx.sample_packets(N, 1234, 0, **src)
            if rep >= WARM:
                times[name].append(ctx.last_kernel_ms())
    for name, ms in times.items():
        print(json.dumps({'kernel': 'k_sample', 'source': name, 'packets': N, 'reps': REPS,
                          'median_ms': float(np.median(ms)), 'min_ms': min(ms), 'max_ms': max(ms)}))
    ctx.close()


if __name__ == '__main__':
    main()
