"""NumPy restatement of the CameraImage definition in include/nexoclom_hip.h (nxc_camera_desc),
written from that text, operation by operation, one IEEE rounding per operation.  It does not call
the library.

``camera_image(...)`` returns a ``CameraResult``: image, counts (nx, nz), the number of samples
offered and binned, ``nonfinite`` as steps 3, 6 and 8 count it, and two guards that say how far
the inputs are from any decision the device
could take differently by a rounding:

* ``edge_guard``: the smallest distance of any tangent-plane coordinate (u, v of a sample in front
  of the camera) to a bin edge or frame border, relative to max(|coordinate|, half width);
* ``margin_guard``: the smallest relative margin of ``dc > 0`` (all samples) and of the three
  occultation inequalities (binned samples): |dc| / r, |b| / (|o| r), |b - r2| / max(|b|, r2),
  |c2 - r2| / max(c2, r2).

``camera_samples(...)`` takes the same arguments and returns the per-sample intermediates of the
same arithmetic as a dict of arrays: dc, front, u, v, ix, iz (-1: not located), located, pix, b, r2,
c2, b_r2 = b - r2 and c2_r2 = c2 - r2 (0 iff the two are equal), hidden, s = x*x + z*z, sunlit (all
true for quantity 'column', which does not take the decision), w (the final weight of step 7) and
keep (step 8 reached with a finite weight), and the count ``nonfinite``.
tests/threshold_cases.py places samples on the thresholds with them.
"""
from collections import namedtuple

import numpy as np

CameraResult = namedtuple('CameraResult', 'image counts samples binned edge_guard margin_guard '
                                          'nonfinite')


def _bins(value, edges):
    """np.histogram2d's bin along one axis: searchsorted(edges, v, 'right') - 1, the last edge
    folded into the last bin, everything else (NaN included) outside = -1."""
    n = len(edges) - 1
    k = np.searchsorted(edges, value, side='right') - 1
    k = np.where(value == edges[-1], n - 1, k)
    inside = (value >= edges[0]) & (value <= edges[-1])
    return np.where(inside, k, -1)


def _edge_distance(value, edges):
    """Smallest |value - edge| over the edges, relative to max(|value|, half width)."""
    if len(value) == 0:
        return np.inf
    k = np.clip(np.searchsorted(edges, value), 1, len(edges) - 1)
    near = np.minimum(np.abs(value - edges[k - 1]), np.abs(value - edges[k]))
    return float(np.min(near / np.maximum(np.abs(value), edges[-1])))


def _camera(x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity, g_tables):
    x, y, z, vy, frac = (np.asarray(c).astype(np.float64) for c in (x, y, z, vy, frac))
    o = np.asarray(o, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64).reshape(9)
    uedges, vedges = np.asarray(uedges, dtype=np.float64), np.asarray(vedges, dtype=np.float64)
    nx, nz = len(uedges) - 1, len(vedges) - 1
    with np.errstate(all='ignore'):
        # 1
        dx, dy, dz = x - o[0], y - o[1], z - o[2]
        radvel = vy + vrplanet
        xc = (C[0]*dx + C[1]*dy) + C[2]*dz
        dc = (C[3]*dx + C[4]*dy) + C[5]*dz
        zc = (C[6]*dx + C[7]*dy) + C[8]*dz
        # 2, 3
        front = dc > 0
        u, v = xc/dc, zc/dc
        ix = np.where(front, _bins(u, uedges), -1)
        iz = np.where(front, _bins(v, vedges), -1)
        located = (ix >= 0) & (iz >= 0)
        # 4
        r2 = (dx*dx + dy*dy) + dz*dz
        b = -((o[0]*dx + o[1]*dy) + o[2]*dz)
        cx, cy, cz = o[1]*z - o[2]*y, o[2]*x - o[0]*z, o[0]*y - o[1]*x
        c2 = (cx*cx + cy*cy) + cz*cz
        hidden = (b > 0) & (b < r2) & (c2 < r2)
        f = np.where(hidden, frac*0.0, frac)
        # 5
        sunlit = np.ones(len(f), dtype=bool)
        if quantity == 'radiance':
            sunlit = (x*x + z*z > 1.0 + 2.0**-52) | (y < 0)
            f = np.where(sunlit, f, f*0.0)
            # 6
            gg = np.zeros(len(f))
            for k, (v_tab, g_tab) in enumerate(g_tables):
                g = np.interp(radvel, v_tab, g_tab)
                gg = g if k == 0 else gg + g
            w = (f*gg)/1e6
        elif quantity == 'column':
            w = f
        else:
            raise ValueError(f'{quantity} is invalid.')
        keep = located & np.isfinite(w) & ~np.isnan(radvel)
        # 7
        r = np.sqrt(r2)
        foot = ((dc*dc)*dc)/r
        w = w/(foot*pix_area_cm2)
        # 8
        outside_bad = ~located & (~np.isfinite(frac) | np.isnan(radvel))
        keep &= np.isfinite(w)
    return dict(dc=dc, u=u, v=v, ix=ix, iz=iz, located=located, b=b, r2=r2, c2=c2, hidden=hidden,
                b_r2=b - r2, c2_r2=c2 - r2,
                sunlit=sunlit, s=x*x + z*z, w=w, keep=keep, pix=ix*nz + iz, front=front,
                nonfinite=int(outside_bad.sum() + (located & ~keep).sum()))


def camera_samples(x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity,
                   g_tables=()):
    return _camera(x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity, g_tables)


def camera_image(x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity,
                 g_tables=()):
    d = _camera(x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity, g_tables)
    o = np.asarray(o, dtype=np.float64)
    uedges, vedges = np.asarray(uedges, dtype=np.float64), np.asarray(vedges, dtype=np.float64)
    nx, nz = len(uedges) - 1, len(vedges) - 1
    dc, u, v, ix, iz, located, b, r2, c2, w, keep, front = (d[k] for k in (
        'dc', 'u', 'v', 'ix', 'iz', 'located', 'b', 'r2', 'c2', 'w', 'keep', 'front'))
    pix = (ix*nz + iz)[keep]
    image = np.bincount(pix, weights=w[keep], minlength=nx*nz).reshape(nx, nz)
    counts = np.bincount(pix, minlength=nx*nz).reshape(nx, nz)

    with np.errstate(all='ignore'):
        edge_guard = min(_edge_distance(u[front], uedges), _edge_distance(v[front], vedges))
        rr = np.sqrt(r2)
        margins = [np.abs(dc)/rr]
        if located.any():
            bl, r2l, c2l = b[located], r2[located], c2[located]
            margins += [np.abs(bl)/(np.linalg.norm(o)*np.sqrt(r2l)),
                        np.abs(bl - r2l)/np.maximum(np.abs(bl), r2l),
                        np.abs(c2l - r2l)/np.maximum(c2l, r2l)]
        margin_guard = min((float(np.min(m)) for m in margins if len(m)), default=np.inf)
    return CameraResult(image, counts, len(dc), int(keep.sum()), edge_guard, margin_guard,
                        d['nonfinite'])
