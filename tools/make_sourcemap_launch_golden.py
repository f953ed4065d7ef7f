"""Generate tests/golden/g10_map_deviates.npz FROM THE REFERENCE'S OWN DEVIATE FUNCTIONS.

Build machine only (like oracle/make_golden.py): it needs the reference checkout, which
$NEXOCLOM_REFERENCE names (default /root/reference).

    python tools/make_sourcemap_launch_golden.py

math/randomdeviates.py is loaded by path.  It imports astropy.units only to recognise a
``1*u.cm`` in a type check, so a stand-in module with a ``cm`` that plain floats can be multiplied
with is enough.  Only inputs, seeds and the deviates the reference draws are stored.

What the file holds (the launch-from-a-map tests read it):
  longitude [24], latitude [13], abundance [24, 13]
        a hand-made map: a peak on a low floor, a band of zeros in longitude, unevenly spaced
        latitudes
  abundance_1d [24]         a 1-D map on the same longitudes
  speed [50], speed_dist [50]   a speed table, km/s
  seed, n                   np.random.seed(seed) before each of the two sequences below
  lon_2d, s_2d, speed_2d    random_deviates_2d(abundance, longitude, sin(latitude), n), then --
                            without re-seeding, as a model run draws them --
                            random_deviates_1d(speed, speed_dist, n)
  lon_1d, speed_1d          random_deviates_1d(longitude, abundance_1d, n), then the speeds
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ROOT = os.environ.get('NEXOCLOM_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'g10_map_deviates.npz')
SEED, N = 20260, 2000


class _Unit:
    def __rmul__(self, other):
        return self


def reference_deviates():
    if 'astropy' not in sys.modules:
        units = types.ModuleType('astropy.units')
        units.cm = _Unit()
        package = types.ModuleType('astropy')
        package.units = units
        sys.modules['astropy'], sys.modules['astropy.units'] = package, units
    path = os.path.join(REF_ROOT, 'nexoclom', 'math', 'randomdeviates.py')
    spec = importlib.util.spec_from_file_location('reference_randomdeviates', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def inputs():
    longitude = np.linspace(0, 2*np.pi, 24)
    # uneven latitudes: denser towards the equator
    latitude = np.pi/2*np.sign(np.linspace(-1, 1, 13))*np.abs(np.linspace(-1, 1, 13))**1.5
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    distance2 = ((lon - 4.0)/0.5)**2 + ((lat - 0.3)/0.35)**2
    abundance = 0.02 + np.exp(-0.5*distance2)
    abundance[5:9, :] = 0.0                                  # a band nobody looked at
    abundance_1d = 1.0 + np.cos(longitude - 1.0)**2
    abundance_1d[14:17] = 0.0
    speed = np.linspace(0.05, 9.95, 50)
    speed_dist = speed**3*np.exp(-(speed/2.2)**2)
    return dict(longitude=longitude, latitude=latitude, abundance=abundance,
                abundance_1d=abundance_1d, speed=speed, speed_dist=speed_dist)


def main():
    ref = reference_deviates()
    d = inputs()
    np.random.seed(SEED)
    lon_2d, s_2d = ref.random_deviates_2d(d['abundance'], d['longitude'], np.sin(d['latitude']), N)
    speed_2d = ref.random_deviates_1d(d['speed'], d['speed_dist'], N)
    np.random.seed(SEED)
    lon_1d = ref.random_deviates_1d(d['longitude'], d['abundance_1d'], N)
    speed_1d = ref.random_deviates_1d(d['speed'], d['speed_dist'], N)
    np.savez_compressed(OUT, seed=SEED, n=N, lon_2d=lon_2d, s_2d=s_2d, speed_2d=speed_2d,
                        lon_1d=lon_1d, speed_1d=speed_1d, **d)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
