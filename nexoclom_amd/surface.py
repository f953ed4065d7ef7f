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


class SurfaceInteraction:
    """SurfaceInteraction.py:10-61: ``stickcoef(lon, lat)`` for temperature-dependent sticking
    and ``v_interp(T, p)`` [km/s] for accommodation (when accomfactor != 0): the speed below which
    a fraction p of a Maxwellian flux at temperature T is emitted, tabulated on ``nt``
    temperatures spanning the planet's surface and ``nprob`` probabilities."""

    def __init__(self, inputs, nt=201, nv=101, nprob=101):
        spec = inputs.surfaceinteraction
        self.inputs = inputs
        assert spec.sticktype != 'surface map', 'sticking maps are out of scope'
        if spec.sticktype == 'temperature dependent':
            self.stickcoef = self._sticking_law(inputs.geometry, spec.A)
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
    stick (stickcoef == 1)."""
    spec = inputs.surfaceinteraction
    if spec.sticktype == 'constant' and spec.stickcoef == 1.:
        return None
    surf = SurfaceInteraction(inputs)
    tx, ty, coef = surf.bounce_tables()
    by_temperature = spec.sticktype == 'temperature dependent'
    return dict(GM=float(GM), unit_km=float(unit_km),
                accomfactor=float(spec.accomfactor or 0.0),
                temp_dependent=int(by_temperature),
                stickcoef=0.0 if by_temperature else float(spec.stickcoef),
                A=tuple(spec.A) if by_temperature else (0., 0., 0.),
                t0=NIGHT_SIDE_K, t1=float(day_side_t1(inputs.geometry)), tpow=0.25,
                tx=tx, ty=ty, coef=coef, seed=0 if seed is None else int(seed),
                surf=surf)
