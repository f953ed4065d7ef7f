"""NumPy restatement of the "ShellMap moments" definition in include/nexoclom_hip.h, written from that
text, operation by operation, one IEEE rounding per operation (np.sqrt and / are correctly rounded).
It stands on tests/shell_map_restatement.py: the pair, planes A and B, the counters and the three
guards are ``shell_map``'s, and the record and weight of every filed sample are formed by the same
steps 1-8 (``filed_samples``; plane A rebuilt from them must equal ``shell_map``'s bit for bit, which
is asserted).  It does not call the library.

``shell_moments(...)`` returns a ``ShellMomentsResult``: ``base`` (the ``ShellResult``), ``moments``
(6, nlon, nlat, nalt + 2, 2): the twelve sums, ``abs_moments``, the same shape: the sum of |term| per
entry, and ``base``'s fields (counts, column, sums, abs_sums, samples, binned, nonfinite, edge_guard,
margin_guard, bin_guard) by name."""
from collections import namedtuple

import numpy as np

from tests.camera_restatement import _bins
from tests.shell_map_restatement import TWO_PI, ShellResult, edges, shell_map

_Fields = namedtuple('ShellMomentsResult', ('base', 'moments', 'abs_moments') + ShellResult._fields)
SHELL_MOMENT_COLUMNS = ('ur', 'ue', 'un', 'urr', 'uee', 'unn', 'ure', 'urn', 'uen', 'up', 'upup',
                        'dndn')


class ShellMomentsResult(_Fields):
    __slots__ = ()


def filed_samples(x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt):
    """(index of every filed sample, its record cell * (nalt + 2) + k, its weight w): steps 1-8 of
    "ShellMap" as tests/shell_map_restatement.py takes them."""
    lon_edges, mu_edges = edges(nlon, nlat)
    inv_dr = np.float64(nalt)/(np.float64(r_hi) - np.float64(r_lo))
    with np.errstate(all='ignore'):
        radvel = vy + vrplanet
        r2 = (x*x + y*y) + z*z
        r = np.sqrt(r2)
        mu = z/r
        lon = np.arctan2(x, -y)
        lon = np.where(lon < 0, lon + TWO_PI, lon)
        ix, iz = _bins(lon, lon_edges), _bins(mu, mu_edges)
        located = (ix >= 0) & (iz >= 0)
        f = frac
        if quantity == 'radiance':
            sunlit = (x*x + z*z > 1.0 + 2.0**-52) | (y < 0)
            f = np.where(sunlit, f, f*0.0)
            gg = np.zeros(len(f))
            for k, (v_tab, g_tab) in enumerate(g_tables):
                g = np.interp(radvel, v_tab, g_tab)
                gg = g if k == 0 else gg + g
            w = (f*gg)/1e6
        elif quantity == 'column':
            w = f
        else:
            raise ValueError(f'{quantity} is invalid.')
        keep = located & np.isfinite(w) & ~np.isnan(radvel) & np.isfinite(w/r2)
        filed = np.flatnonzero(keep & (w != 0))
        t = (r[filed] - r_lo)*inv_dr
        inside = (t >= 0) & (t < nalt)
        k = np.full(t.shape, nalt + 1, dtype=np.int64)
        k[t < 0] = 0
        k[inside] = 1 + t[inside].astype(np.int64)
        rec = (ix*nlat + iz)[filed]*(nalt + 2) + k
    return filed, rec, w[filed]


def local_velocity(x, y, z, vx, vy, vz):
    """(v_r, v_e, v_n, p2) of steps 1-4 of "ShellMap moments" """
    with np.errstate(all='ignore'):
        p2 = x*x + y*y
        r2 = p2 + z*z
        r, p = np.sqrt(r2), np.sqrt(p2)
        h = x*vx + y*vy
        v_r = (h + z*vz)/r
        v_e = (x*vy - y*vx)/p
        v_n = (p2*vz - z*h)/(r*p)
    return v_r, v_e, v_n, p2


def shell_moments(x, y, z, vx, vy, vz, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi,
                  nalt):
    x, y, z, vx, vy, vz, frac = (np.asarray(c).astype(np.float64) for c in (x, y, z, vx, vy, vz, frac))
    nalt = int(nalt)
    grid = (vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt)
    base = shell_map(x, y, z, vy, frac, *grid)
    filed, rec, w = filed_samples(x, y, z, vy, frac, *grid)
    n = nlon*nlat*(nalt + 2)
    shape = (nlon, nlat, nalt + 2)
    # the same samples under the same records as shell_map's plane A
    assert np.array_equal(np.bincount(rec, weights=w, minlength=n).reshape(shape), base.sums[0, ..., 0])
    v_r, v_e, v_n, p2 = local_velocity(*(c[filed] for c in (x, y, z, vx, vy, vz)))
    off_axis = p2 != 0.0                                                   # step 5
    rec, w, v_r, v_e, v_n = (a[off_axis] for a in (rec, w, v_r, v_e, v_n))
    with np.errstate(all='ignore'):
        u_r, u_e, u_n = w*v_r, w*v_e, w*v_n                                # step 6
        up = np.where(v_r > 0, u_r, 0.0)
        dn = np.where(v_r < 0, -u_r, 0.0)
        terms = [[u_r, u_e], [u_n, u_r*v_r], [u_e*v_e, u_n*v_n], [u_r*v_e, u_r*v_n],
                 [u_e*v_n, up], [up*up, dn*dn]]                            # step 7
        sums = np.array([[np.bincount(rec, weights=term, minlength=n) for term in plane]
                         for plane in terms])
        mags = np.array([[np.bincount(rec, weights=np.abs(term), minlength=n) for term in plane]
                         for plane in terms])
    full = (6, nlon, nlat, nalt + 2, 2)
    sums = np.moveaxis(sums, 1, 2).reshape(full)
    mags = np.moveaxis(mags, 1, 2).reshape(full)
    return ShellMomentsResult(base, sums, mags, *base)
