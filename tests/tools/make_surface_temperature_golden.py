"""Generate tests/golden/g11_surface_temperature.npz FROM THE REFERENCE'S OWN SURFACE TEMPERATURE.

Build machine only: it needs a checkout of the reference, named by the first argument or by
$NEXOCLOM_REFERENCE.

    python tests/tools/make_surface_temperature_golden.py REFERENCE_CHECKOUT

initial_state/surface_temperature.py is loaded by path; it imports only numpy.  The reference
reads ``geometry.taa`` as an astropy quantity (``np.cos(geometry.taa)`` followed by ``.value``);
astropy is not needed for that: a one-element ndarray subclass with a ``value`` property is what
np.cos hands back.

What the file holds (tests/test_thermal_source_cpu.py compares surface.surface_temperature with
it bit for bit):
  taa [2]                  true anomalies, rad
  longitude, latitude [n]  a 5-degree grid (73 x 37, flattened lon-major), the terminator
                           longitudes pi/2 and 3 pi/2 with their neighbouring doubles, 0 and
                           2 pi, the poles, and random points
  temperature [2, n]       surface_temperature(geometry(taa[k]), longitude, latitude), K
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g11_surface_temperature.npz')
TAA = (1.3, 3.5)
SEED = 11


class Angle(np.ndarray):
    """What the reference's ``geometry.taa`` has to do: np.cos of it keeps the class, and
    ``.value`` is the plain number array."""

    @property
    def value(self):
        return np.asarray(self)


class Geometry:
    def __init__(self, taa):
        self.startpoint = 'Mercury'
        self.taa = np.array([taa], dtype=np.float64).view(Angle)


def points():
    grid_lon, grid_lat = np.meshgrid(np.arange(0, 361, 5)*np.pi/180.,
                                     np.arange(0, 181, 5)*np.pi/180. - np.pi/2., indexing='ij')
    special_lon = []
    for lon in (0.0, np.pi/2, 3*np.pi/2, 2*np.pi):
        special_lon += [np.nextafter(lon, -np.inf), lon, np.nextafter(lon, np.inf)]
    special_lon = np.array([x for x in special_lon if 0.0 <= x <= 2*np.pi])
    special_lat = np.array([-np.pi/2, np.nextafter(-np.pi/2, 0), 0.0, np.nextafter(np.pi/2, 0),
                            np.pi/2, 0.3, -1.1])
    sl, sb = np.meshgrid(special_lon, special_lat, indexing='ij')
    rng = np.random.default_rng(SEED)
    rand_lon = rng.random(2000)*2*np.pi
    rand_lat = np.arcsin(2*rng.random(2000) - 1)
    lon = np.concatenate([grid_lon.ravel(), sl.ravel(), rand_lon])
    lat = np.concatenate([grid_lat.ravel(), sb.ravel(), rand_lat])
    return lon, lat


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NEXOCLOM_REFERENCE')
    if not ref_root:
        sys.exit(__doc__)
    path = os.path.join(ref_root, 'nexoclom', 'initial_state', 'surface_temperature.py')
    spec = importlib.util.spec_from_file_location('reference_surface_temperature', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    lon, lat = points()
    temperature = np.array([module.surface_temperature(Geometry(taa), lon, lat) for taa in TAA])
    assert temperature.shape == (len(TAA), len(lon)) and np.all(np.isfinite(temperature))
    np.savez_compressed(OUT, taa=np.array(TAA), longitude=lon, latitude=lat,
                        temperature=temperature)
    print(f'{OUT}: {len(lon)} points at taa = {TAA}, T in [{temperature.min():.3f}, '
          f'{temperature.max():.3f}] K')


if __name__ == '__main__':
    main()
