"""NumPy restatement of the ShellMap definition in include/nexoclom_hip.h ("ShellMap"), written from
that text, operation by operation, one IEEE rounding per operation (np.sqrt and / are correctly
rounded; np.arctan2 decides a bin only).  It does not call the library.

``shell_map(...)`` returns a ``ShellResult``:

* ``counts``, ``column`` (nlon, nlat); ``sums`` (2, nlon, nlat, nalt + 2, 2): plane A {w, w*w} and
  plane B {c, c*c}, c = w / r2, per cell and altitude record; ``abs_sums``, the same shape: the sum
  of |term| per entry; ``samples``, ``binned``, ``nonfinite``;
* ``edge_guard``: the smallest distance of the lon (mu) of a located sample to an edge of its axis,
  in units of the axis' length 2 pi (2) -- the seam 0 / 2 pi and the poles are edges;
* ``margin_guard``: the smallest relative margin of the sunlit test of a located sample,
  min(|s - 1| / max(s, 1), |y| / r) with s = x*x + z*z (inf for quantity 'column', which does not
  take the decision);
* ``bin_guard``: the smallest distance of any t in [0, nalt] of a filed sample to an integer (inf
  when there is none): how far the nearest sample is from changing its altitude record.

``shell_samples(...)`` takes the same arguments and returns the per-sample intermediates of the same
arithmetic as a dict of arrays: lon, mu, r, r2, ix, iz (-1: outside), located, cell, s = x*x + z*z,
sunlit (all true for quantity 'column'), w, c, keep (step 7 reached), filed (keep and w != 0), t and
k, the altitude record of step 8 (NaN and -1 where nothing is filed), and the count ``nonfinite``.
tests/threshold_cases.py places samples on the thresholds with them.
"""
from collections import namedtuple

import numpy as np

from tests.camera_restatement import _bins

ShellResult = namedtuple('ShellResult', 'counts column sums abs_sums samples binned nonfinite '
                                        'edge_guard margin_guard bin_guard')
TWO_PI = 2*np.pi


def edges(nlon, nlat):
    return np.linspace(0, TWO_PI, nlon + 1), np.linspace(-1, 1, nlat + 1)


def _edge_distance(value, edge, length):
    if len(value) == 0:
        return np.inf
    k = np.clip(np.searchsorted(edge, value), 1, len(edge) - 1)
    near = np.minimum(np.abs(value - edge[k - 1]), np.abs(value - edge[k]))
    return float(np.min(near))/length


def shell_samples(x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt):
    return shell_map(x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt,
                     samples=True)


def shell_map(x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt,
              samples=False):
    x, y, z, vy, frac = (np.asarray(c).astype(np.float64) for c in (x, y, z, vy, frac))
    lon_edges, mu_edges = edges(nlon, nlat)
    nalt = int(nalt)
    inv_dr = np.float64(nalt)/(np.float64(r_hi) - np.float64(r_lo))
    with np.errstate(all='ignore'):
        # 1
        radvel = vy + vrplanet
        r2 = (x*x + y*y) + z*z
        r = np.sqrt(r2)
        mu = z/r
        # 2
        lon = np.arctan2(x, -y)
        lon = np.where(lon < 0, lon + TWO_PI, lon)
        # 3
        ix, iz = _bins(lon, lon_edges), _bins(mu, mu_edges)
        located = (ix >= 0) & (iz >= 0)
        outside_bad = ~located & (~np.isfinite(frac) | np.isnan(radvel))
        # 4
        f = frac
        s = x*x + z*z
        sunlit = np.ones(len(f), dtype=bool)
        if quantity == 'radiance':
            sunlit = (s > 1.0 + 2.0**-52) | (y < 0)
            f = np.where(sunlit, f, f*0.0)
            # 5
            gg = np.zeros(len(f))
            for k, (v_tab, g_tab) in enumerate(g_tables):
                g = np.interp(radvel, v_tab, g_tab)
                gg = g if k == 0 else gg + g
            w = (f*gg)/1e6
        elif quantity == 'column':
            w = f
        else:
            raise ValueError(f'{quantity} is invalid.')
        weighed = located & np.isfinite(w) & ~np.isnan(radvel)
        # 6
        c = w/r2
        keep = weighed & np.isfinite(c)
        nonfinite = int(outside_bad.sum() + (located & ~keep).sum())
        # 7
        cell = (ix*nlat + iz)[keep]
        ncell = nlon*nlat
        column = np.bincount(cell, weights=c[keep], minlength=ncell).reshape(nlon, nlat)
        counts = np.bincount(cell, minlength=ncell).reshape(nlon, nlat)
        # 8
        filed = keep & (w != 0)
        t = (r[filed] - r_lo)*inv_dr
        inside = (t >= 0) & (t < nalt)
        k = np.full(t.shape, nalt + 1, dtype=np.int64)
        k[t < 0] = 0
        k[inside] = 1 + t[inside].astype(np.int64)
        rec = (ix*nlat + iz)[filed]*(nalt + 2) + k
        if samples:
            t_all, k_all = np.full(len(x), np.nan), np.full(len(x), -1, dtype=np.int64)
            t_all[filed], k_all[filed] = t, k
            return dict(lon=lon, mu=mu, r=r, r2=r2, t=t_all, ix=ix, iz=iz, located=located,
                        cell=ix*nlat + iz, sunlit=sunlit, s=s, w=w, c=c, keep=keep, filed=filed, k=k_all,
                        nonfinite=nonfinite)
        n = ncell*(nalt + 2)
        wf, cf = w[filed], c[filed]
        terms = [[wf, wf*wf], [cf, cf*cf]]
        sums = np.array([[np.bincount(rec, weights=term, minlength=n) for term in plane]
                         for plane in terms])
        mags = np.array([[np.bincount(rec, weights=np.abs(term), minlength=n) for term in plane]
                         for plane in terms])
        shape = (2, nlon, nlat, nalt + 2, 2)
        sums = np.moveaxis(sums, 1, 2).reshape(shape)
        mags = np.moveaxis(mags, 1, 2).reshape(shape)

        edge_guard = min(_edge_distance(lon[located], lon_edges, TWO_PI),
                         _edge_distance(mu[located], mu_edges, 2.0))
        margin_guard = np.inf
        if quantity == 'radiance' and located.any():
            sl, yl, rl = s[located], y[located], r[located]
            margin_guard = float(np.min(np.minimum(np.abs(sl - 1.0)/np.maximum(sl, 1.0),
                                                   np.abs(yl)/rl)))
        near = t[(t >= 0) & (t <= nalt)]
        bin_guard = float(np.min(np.abs(near - np.rint(near)))) if near.size else np.inf
    return ShellResult(counts, column, sums, mags, len(x), int(keep.sum()), nonfinite, edge_guard,
                       margin_guard, bin_guard)
