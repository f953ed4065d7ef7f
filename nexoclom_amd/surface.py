"""Surface interaction set-up for re-emitted packets (host side).

What the kernels need when a packet that hits the surface is not simply absorbed
(particle_tracking/bouncepackets.py:39-100): the Mercury surface-temperature model
(initial_state/surface_temperature.py:4-19), the temperature-dependent sticking coefficient and
the table of thermally accommodated emission speeds v(T, probability) with its interpolating
bicubic spline (particle_tracking/SurfaceInteraction.py:10-61: scipy RectBivariateSpline =
FITPACK).  ``bounce_tables()`` exports the spline's knots and coefficients so that the HIP kernel
evaluates the very same spline (de Boor) at every impact.  The same table gives thermal launch
speeds ('maxwellian' at temperature 0): ``thermal_launch_spline`` builds it once per Input, whatever
the surface interaction.

Sticking from a surface map (``sticktype = surface map``; docs/nexoclom/inputfiles.rst, "Sticking
Coefficient from a Surface Map"; the reference stops at ``assert 0``, SurfaceInteraction.py:23-24 and
bouncepackets.py:90-91): ``stick_mapfile`` names a SourceMap .npz whose ``abundance`` holds the
coefficient on the nodes ``longitude`` (x ``latitude``), solar-fixed.  ``load_sticking_map`` reads
and checks it, ``sticking_map_callable`` is the interpolation rule the kernel follows operation
for operation (nxc_device.hpp, stick_map_at).
"""
import threading

import numpy as np
from scipy import interpolate

from . import constants as const
from .source_distribution import MaxwellianDist, density_cdf

NIGHT_SIDE_K = 100.


def day_side_t1(geometry):
    """Sub-solar excess temperature [K] at the planet's true anomaly."""
    return 600. + 125*(np.cos(float(geometry.taa)) - 1)/2.


def surface_temperature(geometry, longitude, latitude, t0=NIGHT_SIDE_K, t1=None, n=.25):
    """Mercury only (surface_temperature.py:4-19): t0 on the night side; on the day side (within
    90 degrees of the sub-solar longitude) t0 + t1 |cos(lon) cos(lat)|^n."""
    if geometry.startpoint != 'Mercury':
        raise NotImplementedError('surface temperature is only defined for Mercury')
    excess = day_side_t1(geometry) if t1 is None else t1
    lon = np.asarray(longitude, dtype=float)
    lat = np.asarray(latitude, dtype=float)
    day = (lon <= np.pi/2) | (lon >= 3*np.pi/2)
    temperature = np.full_like(lon, t0)
    temperature[day] = t0 + excess*np.abs(np.cos(lon[day]) * np.cos(lat[day]))**n
    return temperature


def tabulate_thermal_speeds(geometry, species, nt=201, nv=101, nprob=101):
    """(temperature, probability, probgrid, spline) of SurfaceInteraction.py:28-61: on ``nt``
    temperatures spanning the surface temperatures of the 1-degree (lon, lat) grid and ``nprob``
    probabilities, the speed [km/s] below which a fraction p of a Maxwellian flux at temperature T
    is emitted (inverse CDF on ``nv`` speeds up to 3 v_th), and its interpolating bicubic spline
    (scipy RectBivariateSpline = FITPACK).  Used for accommodated re-emission and for the thermal
    launch source ('maxwellian' at temperature 0)."""
    lon, lat = np.meshgrid(np.arange(361)*np.pi/180., np.arange(181)*np.pi/180. - np.pi/2.)
    everywhere = surface_temperature(geometry, lon.flatten(), lat.flatten())
    temperature = np.linspace(min(everywhere), max(everywhere), nt)
    probability = np.linspace(0, 1, nprob)
    mass = const.ATOMIC_MASS[species]*const.AMU
    thermal = np.sqrt(2*temperature*const.K_B/mass)/1e3                     # km/s
    probgrid = np.ndarray((nt, nprob))
    for row, (kelvin, v_th) in enumerate(zip(temperature, thermal)):
        speeds = np.linspace(0, v_th*3, nv)
        cdf, grid = density_cdf(speeds, MaxwellianDist(speeds, kelvin, species))
        probgrid[row, :] = np.interp(probability, cdf, grid)
    spline = interpolate.RectBivariateSpline(temperature, probability, probgrid)
    return temperature, probability, probgrid, spline


def spline_tables(spline):
    """(tx, ty, coef[nx-4, ny-4]) of a bicubic RectBivariateSpline, contiguous: what the kernels
    evaluate it from (nxc_device.hpp, bispev3)."""
    tx, ty, c = spline.tck
    return (np.ascontiguousarray(tx), np.ascontiguousarray(ty),
            np.ascontiguousarray(c.reshape(len(tx)-4, len(ty)-4)))


_THERMAL_LOCK = threading.Lock()


def thermal_launch_spline(inputs):
    """The v(T, p) spline of ``tabulate_thermal_speeds`` at the reference's default resolution for
    these inputs, built once per Input (Input.run makes many Outputs) and kept on it.  Raises
    NotImplementedError unless the packets start from Mercury (the only temperature model)."""
    geometry = inputs.geometry
    if geometry.startpoint != 'Mercury':
        raise NotImplementedError('thermal launch speeds need a surface temperature, which is '
                                  'only defined for Mercury')
    key = (inputs.options.species, float(geometry.taa))
    with _THERMAL_LOCK:
        kept = getattr(inputs, '_thermal_spline', None)
        if kept is not None and kept[0] == key:
            return kept[1]
        spline = tabulate_thermal_speeds(geometry, inputs.options.species)[3]
        try:
            inputs._thermal_spline = (key, spline)
        except AttributeError:
            pass
        return spline


TWO_PI = 6.283185307179586
DEFAULT_A = (1.57014, -0.006262, 0.1614157)      # the inputfiles' default coefficients of the law


def _first_not_a_coefficient(values):
    """Index (as a tuple) and value of the first entry that is not a finite number in [0, 1]."""
    bad = np.argwhere(~(np.isfinite(values) & (values >= 0) & (values <= 1)))
    return (None, None) if len(bad) == 0 else (tuple(int(k) for k in bad[0]), values[tuple(bad[0])])


def check_sticking_map(longitude, latitude, coef, name='sticking map'):
    """(longitude, latitude or None, coef) as contiguous float64, or the ValueError that says why
    the map cannot be interpolated: what nxc_set_stick_map checks, with names."""
    if coef is None or longitude is None:
        raise ValueError(f'{name} holds no abundance map (the sticking coefficient)')
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    longitude = np.ascontiguousarray(longitude, dtype=np.float64)
    latitude = None if latitude is None else np.ascontiguousarray(latitude, dtype=np.float64)
    if longitude.ndim != 1 or (latitude is not None and latitude.ndim != 1):
        raise ValueError(f'{name}: longitude and latitude must be 1-D')
    shape = (len(longitude),) if latitude is None else (len(longitude), len(latitude))
    if coef.shape != shape or min(shape) < 2:
        raise ValueError(f'{name}: abundance{coef.shape} does not fit its axes {shape} (at least '
                         'two nodes each)')
    if not (np.all(np.diff(longitude) > 0) and longitude[0] >= 0 and longitude[-1] < TWO_PI):
        raise ValueError(f'{name}: longitude nodes must increase strictly within [0, 2 pi)')
    if latitude is not None and not (np.all(np.diff(latitude) > 0) and latitude[0] >= -np.pi/2
                                     and latitude[-1] <= np.pi/2):
        raise ValueError(f'{name}: latitude nodes must increase strictly within [-pi/2, pi/2]')
    where, value = _first_not_a_coefficient(coef)
    if where is not None:
        raise ValueError(f'{name}: abundance{list(where)} = {value}; a sticking coefficient must be '
                         'finite and in [0, 1]')
    return longitude, latitude, coef


def load_sticking_map(spec):
    """(longitude, latitude or None, coef) of ``surfaceinteraction.stick_mapfile``, or the reason
    it cannot be used.  Planet-fixed maps are refused as the reference refuses them for sources
    ('Need to verify this works', source_distribution.py:85-93)."""
    from .source_distribution import source_file
    smap = source_file('stick_mapfile', spec.stick_mapfile)
    checked = check_sticking_map(smap.longitude, smap.latitude, smap.abundance, spec.stick_mapfile)
    if 'planet' in smap.coordinate_system:
        if spec.subsolarlon is None:
            raise ValueError('inputs.surfaceinteraction.subsolarlon is None')
        raise NotImplementedError('planet-fixed sticking maps: the reference stops here for source '
                                  "maps as well ('Need to verify this works')")
    return checked


def sticking_map_callable(longitude, latitude, coef):
    """stickcoef(lon, lat) of a checked map.  Bilinear on the map's own nodes.  Longitude is
    periodic: the interval from the last node to the first + 2 pi serves lon >= L[n-1] and
    lon < L[0], the latter shifted by 2 pi.  Latitude is clamped to the end nodes.  i is the
    largest index with L[i] <= lon, j likewise, capped at m - 2; wl = (lon - L[i])/(L[i+1] - L[i]),
    wt likewise, and
        S = (S[i,j] (1 - wl) + S[i+1,j] wl) (1 - wt) + (S[i,j+1] (1 - wl) + S[i+1,j+1] wl) wt,
    every operation rounded once, in that order (the kernel's stick_map_at), then clipped to
    [0, 1].  A 1-D map (``latitude`` None) uses the longitude part only."""
    L, T, S = longitude, latitude, coef
    n = len(L)

    def stickcoef(lon, lat):
        lon = np.array(lon, dtype=np.float64, ndmin=1)
        low = lon < L[0]
        lon[low] = lon[low] + TWO_PI
        i = np.clip(np.searchsorted(L, lon, side='right') - 1, 0, n - 1)
        i[low] = n - 1
        last = i == n - 1
        i1 = np.where(last, 0, i + 1)
        l1 = np.where(last, L[0] + TWO_PI, L[i1])
        wl = (lon - L[i])/(l1 - L[i])
        if T is None:
            return np.clip(S[i]*(1 - wl) + S[i1]*wl, 0., 1.)
        lat = np.array(lat, dtype=np.float64, ndmin=1)
        lat = np.where(lat < T[0], T[0], np.where(lat > T[-1], T[-1], lat))
        j = np.clip(np.searchsorted(T, lat, side='right') - 1, 0, len(T) - 2)
        wt = (lat - T[j])/(T[j + 1] - T[j])
        return np.clip((S[i, j]*(1 - wl) + S[i1, j]*wl)*(1 - wt) +
                       (S[i, j + 1]*(1 - wl) + S[i1, j + 1]*wl)*wt, 0., 1.)
    return stickcoef


def sticking_map_from_law(inputs, longitude, latitude):
    """The Yakshinskiy-Madey law clip(A0 exp(A1 T) + A2, 0, 1) of these inputs
    (``surfaceinteraction.A``, or the inputfiles' default coefficients when the inputs name no
    ``A``) on the nodes ``longitude`` x ``latitude`` [rad], as a SourceMap ready for ``.save()``:
    the file a ``sticktype = surface map`` run reads back."""
    from .sourcemap import SourceMap
    longitude = np.asarray(longitude, dtype=np.float64)
    latitude = np.asarray(latitude, dtype=np.float64)
    A = getattr(inputs.surfaceinteraction, 'A', None) or DEFAULT_A
    law = SurfaceInteraction._sticking_law(inputs.geometry, A)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    coef = law(lon.ravel(), lat.ravel()).reshape(lon.shape)
    smap = SourceMap(dict(abundance=coef, longitude=longitude, latitude=latitude,
                          coordinate_system='solar-fixed'))
    smap.units = {'longitude': 'rad', 'latitude': 'rad', 'abundance': ''}
    return smap



class SurfaceInteraction:
    """SurfaceInteraction.py:10-61: ``stickcoef(lon, lat)`` for temperature-dependent sticking
    and for sticking from a surface map (``stick_map``: its nodes and coefficients), and ``v_interp(T, p)`` [km/s] for accommodation (when accomfactor != 0): the speed below which
    a fraction p of a Maxwellian flux at temperature T is emitted, tabulated on ``nt``
    temperatures spanning the planet's surface and ``nprob`` probabilities."""

    def __init__(self, inputs, nt=201, nv=101, nprob=101):
        spec = inputs.surfaceinteraction
        self.inputs = inputs
        self.stick_map = None
        if spec.sticktype == 'temperature dependent':
            self.stickcoef = self._sticking_law(inputs.geometry, spec.A)
        elif spec.sticktype == 'surface map':
            self.stick_map = load_sticking_map(spec)
            self.stickcoef = sticking_map_callable(*self.stick_map)
        self.spline = None
        if spec.accomfactor != 0:
            self._tabulate(inputs, nt, nv, nprob)

    @staticmethod
    def _sticking_law(geometry, A):
        def stickcoef(lon, lat):
            warm = surface_temperature(geometry, lon, lat)
            return np.clip(A[0] * np.exp(A[1]*warm) + A[2], 0., 1.)
        return stickcoef

    def _tabulate(self, inputs, nt, nv, nprob):
        self.temperature, self.probability, self.probgrid, self.spline = \
            tabulate_thermal_speeds(inputs.geometry, inputs.options.species, nt, nv, nprob)
        self.v_interp = self.spline.ev

    def bounce_tables(self):
        """(tx, ty, coef[nx-4, ny-4]) of the bicubic spline, or zero-filled dummies when there is
        no accommodation."""
        if self.spline is None:
            return np.zeros(8), np.zeros(8), np.zeros((4, 4))
        return spline_tables(self.spline)


def bounce_config(inputs, GM, unit_km, seed):
    """Keyword arguments of hip_api.Context.set_bounce for these inputs; None when packets simply
    stick (stickcoef == 1).  ``temp_dependent`` is the sticking law: 0 constant, 1 temperature,
    2 the surface map ``stick_map`` = (longitude, latitude or None, coef)."""
    spec = inputs.surfaceinteraction
    if spec.sticktype == 'constant' and spec.stickcoef == 1.:
        return None
    surf = SurfaceInteraction(inputs)
    tx, ty, coef = surf.bounce_tables()
    by_temperature = spec.sticktype == 'temperature dependent'
    by_map = spec.sticktype == 'surface map'
    return dict(GM=float(GM), unit_km=float(unit_km),
                accomfactor=float(spec.accomfactor or 0.0),
                temp_dependent=2 if by_map else int(by_temperature), stick_map=surf.stick_map,
                stickcoef=0.0 if by_temperature or by_map else float(spec.stickcoef),
                A=tuple(spec.A) if by_temperature else (0., 0., 0.),
                t0=NIGHT_SIDE_K, t1=float(day_side_t1(inputs.geometry)), tpow=0.25,
                tx=tx, ty=ty, coef=coef, seed=0 if seed is None else int(seed),
                surf=surf)
