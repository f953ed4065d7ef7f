"""Restatement of an impact with sticking from a surface map, and the maps the tests use.

The reference never wrote this law (SurfaceInteraction.py:23-24, bouncepackets.py:90-91:
``assert 0``), so the restatement is np_oracle.bounce_packets with constant sticking 0 -- which
leaves frac alone and does everything else: the move back to the surface, the draws, the direction,
the accommodated speed -- followed by what the inputfile format documents: the coefficient at the
impact point (lonhit, lathit), formed from the re-emitted position as bouncepackets.py:84-85 forms
them, and frac *= 1 - stickcoef(lonhit, lathit).  atan2 and asin are called through np_oracle's
``np``, so that the one-ulp harness of tests/test_gpu_bounce.py (libm_rows, which swaps that name)
moves them here as it does inside bounce_packets.
"""
import numpy as np

from nexoclom_amd import surface
from oracle import np_oracle as O
from tests import bounce_cases as B

_plain_restate = B.restate


def map_config(taa, accomfactor, stick_map, GM, unit_km, seed):
    """bounce_cases.config for sticking law 2 with ``stick_map`` = (lon, lat or None, coef)."""
    cfg = B.config(taa, accomfactor, 2, 0.0, (0., 0., 0.), GM, unit_km, seed)
    lon, lat, coef = surface.check_sticking_map(*stick_map)
    cfg['stick_map'] = (lon, lat, coef)
    cfg['surf'].stickcoef = surface.sticking_map_callable(lon, lat, coef)
    return cfg


def impact_point(X):
    """(lonhit, lathit) of rows already moved back to the surface (bouncepackets.py:84-85)."""
    lonhit = (O.np.arctan2(X[:, 1], -X[:, 2]) + 2*np.pi) % (2*np.pi)
    lathit = O.np.arcsin(X[:, 3])
    return lonhit, lathit


def restate(X, cfg, ids, nbounce, hit=None):
    """bounce_cases.restate for every law: rows after the impact.  Law 2: the constant law with
    coefficient 0, then the map at the impact point."""
    if cfg['temp_dependent'] != 2:
        return _plain_restate(X, cfg, ids, nbounce, hit)
    X = np.array(X, dtype=np.float64)
    r0 = np.sqrt((X[:, 1]*X[:, 1] + X[:, 2]*X[:, 2]) + X[:, 3]*X[:, 3])
    hit = (r0 - 1.) < 0 if hit is None else np.asarray(hit, dtype=bool)
    out = _plain_restate(X, dict(cfg, temp_dependent=0, stickcoef=0.0), ids, nbounce, hit)
    if hit.any():
        lonhit, lathit = impact_point(out[hit])
        out[hit, 7] *= (1 - cfg['surf'].stickcoef(lonhit, lathit))
    return out


# ---- the maps ---------------------------------------------------------------------------------------
def smooth_map(nlon=36, nlat=18):
    """Smooth in both directions, periodic in longitude, within [0.13, 0.87]; nodes at bin centres,
    so that neither longitude 0 nor the poles are nodes: the seam interval and the clamp are used."""
    lon = (np.arange(nlon) + 0.5)*(2*np.pi/nlon)
    lat = -np.pi/2 + (np.arange(nlat) + 0.5)*(np.pi/nlat)
    coef = 0.5 + 0.25*np.cos(lon)[:, None]*np.cos(lat)[None, :] + 0.12*np.sin(2*lon)[:, None]*np.sin(lat)[None, :]
    return lon, lat, coef


def steep_map(nlon=36, nlat=18):
    """0.05 on one side, 0.95 on the other of a step one cell wide: across longitude on the day
    side, and across latitude in the north."""
    lon = np.arange(nlon)*(2*np.pi/nlon)
    lat = np.linspace(-np.pi/2, np.pi/2, nlat)
    coef = np.full((nlon, nlat), 0.05)
    coef[3:20, :] = 0.95
    coef[:, 13:] = 0.95
    return lon, lat, coef


def longitude_map(nlon=24):
    """1-D: a function of longitude only, on uneven nodes."""
    rng = np.random.default_rng(11)
    lon = np.sort(rng.uniform(0.02, 2*np.pi - 0.02, nlon))
    return lon, None, 0.5 + 0.4*np.sin(lon + 0.3)


MAPS = {'smooth': smooth_map, 'steep': steep_map, 'longitude': longitude_map}


def padded(lon, lat, coef):
    """The map as a plain rectangular table for an independent interpolator: one more longitude
    node on either side (the last - 2 pi, the first + 2 pi) and latitude nodes at +-(pi/2 + 1)
    carrying the end rows' values (so that clamping is interpolation between equal values)."""
    lon2 = np.concatenate([[lon[-1] - 2*np.pi], lon, [lon[0] + 2*np.pi]])
    coef2 = np.concatenate([coef[-1:], coef, coef[:1]], axis=0)
    if lat is None:
        return lon2, None, coef2
    lat2 = np.concatenate([[-np.pi/2 - 1.], lat, [np.pi/2 + 1.]])
    coef2 = np.concatenate([coef2[:, :1], coef2, coef2[:, -1:]], axis=1)
    return lon2, lat2, coef2
