#!/usr/bin/env python3
"""k_sample at 1e7 packets for a source map's per-point laws against the map source without them.

Three sources on one smooth 181 x 91 map with make_source_map's default law sizes (100 speed, 23
altitude, 45 azimuth bins), alternated in one process so that they see the same clocks: launch
points from the map with (a) 'user defined' speeds and isotropic directions (the code every map
source ran before), (b) per-point speeds only and (c) per-point speeds and directions.  Per source:
3 warm-up calls, then the HIP-event time of the k_sample launch (nxc_last_kernel_ms) of 15 calls;
median, minimum and maximum as one JSON line each.

    python tools/gpu_exp_distmap_sampler.py [--tag NAME]
"""
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nexoclom_amd import SourceMap, hip_api                                 # noqa: E402
from nexoclom_amd.source_distribution import (density_cdf, node_law_tables,  # noqa: E402
                                              surface_map_cells, surface_map_density)

N, WARM, REPS = 10_000_000, 3, 15
NV, NA, NZ = 100, 23, 45


def centres(top, n):
    edges = np.linspace(0, top, n + 1)
    return edges[:-1] + (edges[1] - edges[0])/2


def smooth_map():
    longitude = np.linspace(0, 2*np.pi, 181)
    latitude = np.linspace(-np.pi/2, np.pi/2, 91)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    speed = np.linspace(0.025, 4.975, NV)
    vth2 = (1.0 + 0.9*np.cos(lon)*np.cos(lat))[:, :, None] + 0.3
    alt, az = centres(np.pi/2, NA), centres(2*np.pi, NZ)
    return dict(longitude=longitude, latitude=latitude,
                abundance=1.0 + 0.8*np.cos(lon)*np.cos(lat), speed=speed,
                speed_dist=speed**3*np.exp(-speed**2/1.3),
                speed_dist_map=speed**3*np.exp(-speed**2/vth2),
                altitude_dist_map=np.cos(alt)*np.sin(alt)**(1.0 + 2.0*np.abs(np.sin(lat)))[:, :, None],
                azimuth_dist_map=1.0 + 0.6*np.cos(az - lon[:, :, None]))


def main():
    tag = sys.argv[sys.argv.index('--tag') + 1] if '--tag' in sys.argv else 'this build'
    content = smooth_map()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'map.npz')
        SourceMap(content).save(path)
        sd = SimpleNamespace(mapfile=path, subsolarlon=None)
        longitude, latitude, abundance, _ = surface_map_density(sd)
        tables = {law: node_law_tables(sd, law) for law in ('speed', 'altitude', 'azimuth')}
    cdf, (lon0, lon1, s0, s1) = surface_map_cells(longitude, latitude, abundance)
    base = dict(endtime=50000., exobase=1.0, unit_km=2440.53, random_time=0, angular_type=1,
                is_planet=1, sinlat0=-1.0, sinlat1=1.0, lon0=0.0, lon1=2*np.pi, vprob=0.0,
                vwidth=0.0, sinalt0=0.0, sinalt1=1.0, az0=0.0, az1=2*np.pi, spatial_type=2,
                map_nodes=abundance, map_cdf=cdf, map_lon0=lon0, map_lon1=lon1, map_s0=s0,
                map_s1=s1)
    sources = {
        'map+user_defined+isotropic': dict(base, speed_type=2, speed_table=density_cdf(
            content['speed'], content['speed_dist'])),
        'map+node_speeds+isotropic': dict(base, speed_type=4, node_speed_table=tables['speed']),
        'map+node_speeds+node_angles': dict(base, speed_type=4, angular_type=2,
                                            node_speed_table=tables['speed'],
                                            node_altitude_table=tables['altitude'],
                                            node_azimuth_table=tables['azimuth'])}
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
