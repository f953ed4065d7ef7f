"""NumPy restatement of the velocity cube of include/nexoclom_hip.h ("Velocity cube"), written from
that text.  It does not call the library.

The per-sample (pixel, w, sample) come from the recorders of tests/pixel_moments_restatement.py
(the oracle's ``create_image`` for the image, tests/camera_restatement.py for the camera) and the
line-of-sight velocity from its ``image_vlos`` / ``camera_vlos``.  Only the bin rule is written
out here, with the header's operations:

    inv_dv = nv / (v_hi - v_lo)                                   formed once, fp64
    t = (vlos - v_lo) * inv_dv
    k = 0 if t < 0;   1 + (int)t if 0 <= t < nv;   nv + 1 otherwise (also vlos not a number)
    {w, w*w} added to record pix*(nv + 2) + k                     (w != 0 only)

``image_cube`` / ``camera_cube`` return a ``CubeResult``: counts, image, sums (nx, nz, nv + 2, 2),
abs_sums (the same shape: sum |w| and sum w*w), the samples offered and binned, the two guards of
the camera restatement (``edge_guard``, ``margin_guard``) and ``bin_guard``, the smallest distance
of any t in [0, nv] to an integer (inf when there is none): how far the nearest sample is from
changing its plane."""
from collections import namedtuple
from unittest import mock

import numpy as np

from tests import camera_restatement as CR
from tests import pixel_moments_restatement as PM

CubeResult = namedtuple('CubeResult', 'counts image sums abs_sums samples binned edge_guard '
                                      'margin_guard bin_guard')


class _Kept(PM._Recorder):
    """A recorder that also keeps what every call returned."""

    def __init__(self, fn):
        super().__init__(fn)
        self.results = []

    def __call__(self, *args, **kwargs):
        self.results.append(super().__call__(*args, **kwargs))
        return self.results[-1]


def planes(vlos, nv, v_lo, v_hi):
    """The plane of every vlos and the bin guard of them all."""
    nv = int(nv)
    inv_dv = np.float64(nv)/(np.float64(v_hi) - np.float64(v_lo))
    with np.errstate(all='ignore'):
        t = (np.asarray(vlos, dtype=np.float64) - np.float64(v_lo))*inv_dv
        inside = (t >= 0) & (t < nv)
        k = np.full(t.shape, nv + 1, dtype=np.int64)
        k[t < 0] = 0
        k[inside] = 1 + t[inside].astype(np.int64)
    near = t[(t >= 0) & (t <= nv)]
    guard = float(np.min(np.abs(near - np.rint(near)))) if near.size else np.inf
    return k, guard


def _cube(pix, w, vlos, nx, nz, nv, v_lo, v_hi):
    use = w != 0
    pix, w, vlos = pix[use], w[use], vlos[use]
    k, guard = planes(vlos, nv, v_lo, v_hi)
    rec = pix*(nv + 2) + k
    n = nx*nz*(nv + 2)
    terms = [w, w*w]
    sums = np.stack([np.bincount(rec, weights=t, minlength=n) for t in terms], axis=1)
    mags = np.stack([np.bincount(rec, weights=np.abs(t), minlength=n) for t in terms], axis=1)
    return sums.reshape(nx, nz, nv + 2, 2), mags.reshape(nx, nz, nv + 2, 2), guard


def image_cube(x, y, z, vx, vy, vz, frac, vrplanet, M, quantity, g_tables, dims, xrange_, zrange_,
               apix_cm2, nv, v_lo, v_hi):
    cols = tuple(np.asarray(c).astype(np.float64) for c in (x, y, z, vx, vy, vz, frac))
    x, y, z, vx, vy, vz, frac = cols
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    nx, nz = dims
    # the moments' restatement runs create_image once, with its recorder and its checks of it; a
    # second recorder around the same call keeps the arguments and the edges for this one
    recorder = _Kept(np.histogram2d)
    with mock.patch.object(np, 'histogram2d', recorder):
        base = PM.image_moments(*cols, vrplanet, M, quantity, g_tables, dims, xrange_, zrange_, apix_cm2)
    ((xo, zo), kwargs), (_, ex, ez) = recorder.calls[0], recorder.results[0]
    w = kwargs['weights']
    ix, iz = CR._bins(xo, ex), CR._bins(zo, ez)
    located = (ix >= 0) & (iz >= 0)
    pix = (ix*nz + iz)[located]
    assert np.array_equal(np.bincount(pix, minlength=nx*nz).reshape(nx, nz), base.counts)
    vlos = PM.image_vlos(M, vx, vy, vz)
    sums, mags, guard = _cube(pix, w[located], vlos[located], nx, nz, nv, v_lo, v_hi)
    return CubeResult(base.counts, base.image, sums, mags, base.samples, base.binned,
                      base.edge_guard, base.margin_guard, guard)


def camera_cube(x, y, z, vx, vy, vz, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity,
                g_tables, nv, v_lo, v_hi):
    cols = tuple(np.asarray(c).astype(np.float64) for c in (x, y, z, vx, vy, vz, frac))
    x, y, z, vx, vy, vz, frac = cols
    o = np.asarray(o, dtype=np.float64)
    nx, nz = len(uedges) - 1, len(vedges) - 1
    args = (o, C, uedges, vedges, vrplanet, pix_area_cm2)
    # the sample of every binned weight, found as camera_moments finds it
    res, pix, w = PM._camera_kept((x, y, z, vy, frac), args, quantity, g_tables)
    tag = np.arange(1.0, len(x) + 1.0)
    _, pix_one, w_one = PM._camera_kept((x, y, z, vy, np.ones(len(x))), args, 'column', ())
    _, pix_tag, w_tag = PM._camera_kept((x, y, z, vy, tag), args, 'column', ())
    assert np.array_equal(pix, pix_one) and np.array_equal(pix, pix_tag)
    assert np.all(w[w_one == 0] == 0)
    seen = w_one != 0
    index = np.rint(w_tag[seen]/w_one[seen]).astype(np.int64) - 1
    assert np.all(np.abs(w_tag[seen]/w_one[seen] - (index + 1)) < 1e-6) and np.all(np.diff(index) > 0)
    pix, w = pix[seen], w[seen]
    vlos = PM.camera_vlos(o, *(c[index] for c in (x, y, z, vx, vy, vz)))
    sums, mags, guard = _cube(pix, w, vlos, nx, nz, nv, v_lo, v_hi)
    return CubeResult(res.counts, res.image, sums, mags, res.samples, res.binned, res.edge_guard,
                      res.margin_guard, guard)
