"""NumPy restatement of the device's thermal launch speeds (k_sample, speed_type 3), and the
table they come from built the way the reference builds it.

TEST INFRASTRUCTURE.  The uniforms are the kernel's own counter-based ones
(oracle.np_oracle.philox_uniform_pairs: block 0 -> (time, sin latitude), block 1 -> (longitude,
speed), block 2 -> (sin altitude, azimuth); a 2-D surface map takes its launch point from blocks 16
and 17 as tests/sourcemap_launch_restatement.py states).  The temperature is formed as the device
forms it -- t0 + t1 sqrt(sqrt(|cos lon cos lat|)), both square roots correctly rounded -- and the
spline is summed as bispev3 sums it (de Boor's basis of FITPACK's fpbspl, then coef * hx[i] * hy[j]
added i-major), so the two agree to the last bits of libm's sin / cos / asin.
"""
import numpy as np
from scipy import interpolate

from nexoclom_amd import constants as const
from oracle.np_oracle import philox_uniform_pairs

from . import sourcemap_launch_restatement as M

STREAM_SOURCE = 0x5a0
NIGHT_K = 100.


# ---- the table, as the reference builds it --------------------------------------------------------
def reference_temperature(taa, lon, lat, t0=NIGHT_K):
    """initial_state/surface_temperature.py:4-19 (Mercury): x**0.25 as the reference takes it."""
    t1 = 600. + 125*(np.cos(taa) - 1)/2.
    lon, lat = np.asarray(lon, dtype=float), np.asarray(lat, dtype=float)
    temperature = np.zeros_like(lon) + t0
    day = (lon <= np.pi/2) | (lon >= 3*np.pi/2)
    temperature[day] = t0 + t1*np.abs(np.cos(lon[day])*np.cos(lat[day]))**.25
    return temperature


def reference_spline(taa, species, nt=201, nv=101, nprob=101):
    """particle_tracking/SurfaceInteraction.py:28-61 step for step (the construction the package
    used for accommodation before the thermal source shared it): temperatures spanning the
    1-degree grid's, for each the inverse CDF of a Maxwellian flux on nv speeds up to 3 v_th
    (math/distributions.py:16-21, randomdeviates.py:29-32), and the RectBivariateSpline over
    (temperature, probability)."""
    lon, lat = np.meshgrid(np.arange(361)*np.pi/180., np.arange(181)*np.pi/180. - np.pi/2.)
    everywhere = reference_temperature(taa, lon.flatten(), lat.flatten())
    temperature = np.linspace(min(everywhere), max(everywhere), nt)
    probability = np.linspace(0, 1, nprob)
    mass = const.ATOMIC_MASS[species]*const.AMU
    thermal = np.sqrt(2*temperature*const.K_B/mass)/1e3
    probgrid = np.ndarray((nt, nprob))
    for row, (kelvin, v_th) in enumerate(zip(temperature, thermal)):
        speeds = np.linspace(0, v_th*3, nv)
        vth2 = 2*kelvin*const.K_B/mass/1e6
        density = speeds**3*np.exp(-speeds**2/vth2)
        density = density/np.max(density)
        cdf = density.cumsum()
        cdf -= cdf.min()
        cdf /= cdf.max()
        grid = np.linspace(speeds.min(), speeds.max(), density.shape[0])
        probgrid[row, :] = np.interp(probability, cdf, grid)
    return interpolate.RectBivariateSpline(temperature, probability, probgrid)


def tables(spline):
    tx, ty, c = spline.tck
    return tx, ty, c.reshape(len(tx) - 4, len(ty) - 4)


# ---- the device's arithmetic -------------------------------------------------------------------------
def device_temperature(lon, lat, t0, t1, cos_lon=None, cos_lat=None):
    """bounce_packet's / k_sample's surface temperature.  ``cos_lon`` / ``cos_lat`` replace
    np.cos(lon) / np.cos(lat) (the tolerance derivation perturbs them)."""
    cl = np.cos(lon) if cos_lon is None else cos_lon
    cb = np.cos(lat) if cos_lat is None else cos_lat
    day = (lon <= 1.5707963267948966) | (lon >= 4.71238898038469)
    return np.where(day, t0 + t1*np.sqrt(np.sqrt(np.abs(cl*cb))), t0)


def _basis3(t, l, x):
    """The four cubic B-spline values at x in knot interval l (nxc_device.hpp bspline_basis3)."""
    h = [np.ones_like(x), np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)]
    for j in range(1, 4):
        hh = list(h[:3])
        h[0] = np.zeros_like(x)
        for i in range(j):
            li = l + i + 1
            lj = li - j
            f = hh[i]/(t[li] - t[lj])
            h[i] = h[i] + f*(t[li] - x)
            h[i + 1] = f*(x - t[lj])
    return h


def _interval(t, x):
    """knot_interval: the last l in [3, n-5] with t[l] <= x (x already clamped)."""
    return np.clip(np.searchsorted(t, x, side='right') - 1, 3, len(t) - 5)


def bispev3(tx, ty, coef, x, y):
    """scipy's .ev(x, y) as the device evaluates it."""
    tx, ty, coef = (np.asarray(a, dtype=float) for a in (tx, ty, coef))
    x = np.fmin(np.fmax(np.asarray(x, dtype=float), tx[3]), tx[len(tx) - 4])
    y = np.fmin(np.fmax(np.asarray(y, dtype=float), ty[3]), ty[len(ty) - 4])
    l, m = _interval(tx, x), _interval(ty, y)
    hx, hy = _basis3(tx, l, x), _basis3(ty, m, y)
    s = np.zeros_like(x)
    for i in range(4):
        for j in range(4):
            s = s + coef[l - 3 + i, m - 3 + j]*hx[i]*hy[j]
    return s


def thermal_speed(lon, lat, u, t0, t1, thermal_spline, **perturb):
    """max(S(T, u), 0) in km/s, T the device's temperature at (lon, lat)."""
    s = bispev3(*thermal_spline, device_temperature(lon, lat, t0, t1, **perturb), u)
    return np.where(s > 0.0, s, 0.0)


# ---- the whole launch ----------------------------------------------------------------------------------
def launch(n, seed, first_index=0, *, spatial_type, sinlat0=-1.0, sinlat1=1.0, lon0=0.0,
           lon1=2*np.pi, **src):
    """(lon, lat, uspd) of packets first_index .. first_index + n - 1 (Philox)."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    _, ulat = philox_uniform_pairs(idx, 0, STREAM_SOURCE, seed)
    ulon, uspd = philox_uniform_pairs(idx, 1, STREAM_SOURCE, seed)
    if spatial_type == 0:
        lat = np.arcsin(sinlat0 + (sinlat1 - sinlat0)*ulat)
        lon = np.fmod(lon0 + (lon1 - lon0)*ulon, 2*np.pi)
    else:
        lon, lat = M.launch_points(n, seed, first_index, spatial_type=spatial_type, **src)
    return lon, lat, uspd


def sample_x0(n, seed, first_index=0, *, endtime, exobase, unit_km, random_time, angular_type,
              is_planet, speed_type, t0, t1, thermal_spline, sinalt0=0.0, sinalt1=1.0, az0=0.0,
              az1=2*np.pi, **source):
    """X0 (n, 8) of a thermal source, k_sample's operations."""
    assert speed_type == 3
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    ut, _ = philox_uniform_pairs(idx, 0, STREAM_SOURCE, seed)
    ualt, uaz = philox_uniform_pairs(idx, 2, STREAM_SOURCE, seed)
    source = {k: v for k, v in source.items() if k not in ('vprob', 'vwidth')}
    lon, lat, uspd = launch(n, seed, first_index, **source)
    time = ut*endtime if random_time else np.zeros(n) + endtime
    sign = 1.0 if is_planet else -1.0
    x0 = sign*exobase*np.sin(lon)*np.cos(lat)
    y0 = -exobase*np.cos(lon)*np.cos(lat)
    z0 = exobase*np.sin(lat)
    v = thermal_speed(lon, lat, uspd, t0, t1, thermal_spline)/unit_km
    if angular_type == 0:
        alt, az = np.zeros(n) + np.pi/2, np.zeros(n)
    else:
        alt = np.arcsin(ualt*(sinalt1 - sinalt0) + sinalt0)
        az = az0 + (az1 - az0)*uaz
    v_rad, v_t0, v_t1 = np.sin(alt), np.cos(alt)*np.cos(az), np.cos(alt)*np.sin(az)
    rn = np.sqrt((x0*x0 + y0*y0) + z0*z0)
    en = np.sqrt(y0*y0 + x0*x0)
    n0, n1, n2 = -z0*x0, -z0*y0, x0*x0 + y0*y0
    nn = np.sqrt((n0*n0 + n1*n1) + n2*n2)
    X = np.zeros((n, 8))
    X[:, 0] = time
    X[:, 1], X[:, 2], X[:, 3] = x0, y0, z0
    X[:, 4] = ((v_t0*(n0/nn) + v_t1*(y0/en)) + v_rad*(x0/rn))*v
    X[:, 5] = ((v_t0*(n1/nn) + v_t1*(-x0/en)) + v_rad*(y0/rn))*v
    X[:, 6] = ((v_t0*(n2/nn) + v_t1*0.0) + v_rad*(z0/rn))*v
    X[:, 7] = 1.0
    return X


# ---- how far libm's last bits can move a speed ------------------------------------------------------
def speed_ulp_sensitivity(lon, lat, u, t0, t1, thermal_spline):
    """Largest relative change of the thermal speed when cos(lon), cos(lat) or the latitude move by
    one ulp either way (np.nextafter): the device's cos / asin may differ from NumPy's by that
    much, and the speed inherits it through T.  Speeds of 0 (u = 0) are left out."""
    base = thermal_speed(lon, lat, u, t0, t1, thermal_spline)
    keep = base > 0
    worst = 0.0
    cl, cb = np.cos(lon), np.cos(lat)
    for direction in (-np.inf, np.inf):
        for perturbed in (dict(cos_lon=np.nextafter(cl, direction), cos_lat=cb),
                          dict(cos_lon=cl, cos_lat=np.nextafter(cb, direction)),
                          dict(cos_lon=np.cos(lon), cos_lat=np.cos(np.nextafter(lat, direction)))):
            v = thermal_speed(lon, lat, u, t0, t1, thermal_spline, **perturbed)
            worst = max(worst, float(np.max(np.abs(v[keep] - base[keep])/base[keep])))
    return worst


# ---- the law, for the statistical tests --------------------------------------------------------------
def invert_in_p(spline, temperature, speed, iterations=60):
    """û with max(S(T, û), 0) = speed, by bisection in p on [0, 1] (S non-decreasing in p):
    the uniform that the speed came from, to within 2^-60."""
    lo, hi = np.zeros_like(speed), np.ones_like(speed)
    for _ in range(iterations):
        mid = 0.5*(lo + hi)
        below = np.maximum(spline.ev(temperature, mid), 0.0) < speed
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    return 0.5*(lo + hi)


def nondecreasing_in_p(spline, points=20001):
    """Whether S(T, .) is non-decreasing on a fine p grid for every temperature of the table."""
    temperature = spline.get_knots()[0]
    rows = np.unique(np.concatenate([temperature, np.linspace(temperature[0], temperature[-1],
                                                              201)]))
    p = np.linspace(0, 1, points)
    for kelvin in rows:
        if np.any(np.diff(spline.ev(np.full_like(p, kelvin), p)) < 0):
            return False
    return True


def law_pvalues(spline, t0, temperature, speed):
    """KS p-values of the recovered uniforms û (``invert_in_p``) against U(0, 1): all packets,
    night-side packets (T == t0), and the day side split into temperature terciles."""
    from scipy import stats
    u_hat = invert_in_p(spline, temperature, speed)
    night = temperature == t0
    day_t = temperature[~night]
    cuts = np.quantile(day_t, [1/3, 2/3])
    groups = {'all': np.ones_like(night), 'night': night,
              'day low': ~night & (temperature <= cuts[0]),
              'day mid': ~night & (temperature > cuts[0]) & (temperature <= cuts[1]),
              'day high': ~night & (temperature > cuts[1])}
    return {name: float(stats.kstest(u_hat[mask], 'uniform').pvalue)
            for name, mask in groups.items()}, groups
