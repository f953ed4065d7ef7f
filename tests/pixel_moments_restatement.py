"""NumPy restatement of the pixel moments of include/nexoclom_hip.h ("Pixel moments"), written from
that text.  It does not call the library.

The image steps are not restated here: the per-sample pixel and final weight w are taken from the
two existing restatements while they run -- the oracle's ``create_image`` (ModelImage) hands them
to ``np.histogram2d`` and ``tests/camera_restatement.camera_image`` (CameraImage) to
``np.bincount``, and a recorder around those two NumPy calls keeps what they were given.  Every
result is checked against what the restatement itself returned (same counts, same image), so a
recorder that picked up the wrong call fails loudly.  Only the line-of-sight velocity and the four
terms are written out here:

    image    vlos = (M[3]*vx + M[4]*vy) + M[5]*vz
    camera   vlos = ((dx*vx + dy*vy) + dz*vz) / r,   dx = x - o[0] ...,  r = sqrt((dx*dx + dy*dy) + dz*dz)
    a = w*vlos;  m1 = a;  m2 = a*vlos;  m3 = (a*vlos)*vlos;  ww = w*w        (w != 0 only)

``image_moments`` / ``camera_moments`` return a ``MomentResult``: counts, image, sums (nx, nz, 4) in
the order m1 m2 m3 ww, abs_sums (nx, nz, 4) = sum |term|, the samples offered and binned, and the two
guards of the camera restatement: ``edge_guard`` (distance of any binned coordinate to a bin edge)
and ``margin_guard`` (distance of any decision to its threshold)."""
from collections import namedtuple
from unittest import mock

import numpy as np

from oracle import np_oracle as O
from tests import camera_restatement as CR

MomentResult = namedtuple('MomentResult',
                          'counts image sums abs_sums samples binned edge_guard margin_guard')


class _Recorder:
    """Calls ``fn`` and keeps the arguments of every call."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.fn(*args, **kwargs)


def image_vlos(M, vx, vy, vz):
    """Row 1 of the image rotation applied to the velocity: positive = receding."""
    m = np.asarray(M, dtype=np.float64).reshape(9)
    return (m[3]*vx + m[4]*vy) + m[5]*vz


def camera_vlos(o, x, y, z, vx, vy, vz):
    """The velocity along the sample's own ray, away from the camera at o."""
    dx, dy, dz = x - o[0], y - o[1], z - o[2]
    r = np.sqrt((dx*dx + dy*dy) + dz*dz)
    return ((dx*vx + dy*vy) + dz*vz)/r


def _sums(pix, w, vlos, nx, nz):
    """The four sums and the sums of the terms' magnitudes over the samples with w != 0."""
    use = w != 0
    pix, w, vlos = pix[use], w[use], vlos[use]
    with np.errstate(all='ignore'):
        a = w*vlos
        m2 = a*vlos
        terms = [a, m2, m2*vlos, w*w]
    sums = np.stack([np.bincount(pix, weights=t, minlength=nx*nz) for t in terms], axis=1)
    mags = np.stack([np.bincount(pix, weights=np.abs(t), minlength=nx*nz) for t in terms], axis=1)
    return sums.reshape(nx, nz, 4), mags.reshape(nx, nz, 4)


def image_moments(x, y, z, vx, vy, vz, frac, vrplanet, M, quantity, g_tables, dims, xrange_, zrange_,
                  apix_cm2):
    x, y, z, vx, vy, vz, frac = (np.asarray(c).astype(np.float64) for c in (x, y, z, vx, vy, vz, frac))
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    nx, nz = dims
    recorder = _Recorder(np.histogram2d)
    with mock.patch.object(np, 'histogram2d', recorder):
        image, counts, ex, ez = O.create_image(x, y, z, vy, frac, vrplanet, M, quantity, g_tables,
                                               list(dims), xrange_, zrange_, apix_cm2, matmul=False)
    (xo, zo), kwargs = recorder.calls[0]
    w = kwargs['weights']
    ix, iz = CR._bins(xo, ex), CR._bins(zo, ez)
    located = (ix >= 0) & (iz >= 0)
    pix = (ix*nz + iz)[located]
    assert np.array_equal(np.bincount(pix, minlength=nx*nz).reshape(nx, nz), counts)
    assert np.array_equal(np.bincount(pix, weights=w[located], minlength=nx*nz).reshape(nx, nz), image)
    m = M.reshape(9)
    vlos = image_vlos(M, vx, vy, vz)
    sums, mags = _sums(pix, w[located], vlos[located], nx, nz)

    # guards: the binned coordinates against the edges; of the located samples, the occultation
    # test (rho_obs > 1 or y_obs < 0) and the shadow test (rho_sun > 1 or y < 0) against their
    # thresholds (both inequalities of each, whichever decides)
    edge_guard = min(CR._edge_distance(xo, ex), CR._edge_distance(zo, ez))
    margin_guard = np.inf
    if located.any():
        yo = ((m[3]*x + m[4]*y) + m[5]*z)[located]
        s_obs = (xo*xo + zo*zo)[located]
        margins = [np.abs(s_obs - 1.0), np.abs(yo)]
        if quantity in ('radiance', 'difrad'):
            margins += [np.abs(x*x + z*z - 1.0)[located], np.abs(y)[located]]
        margin_guard = min(float(np.min(v)) for v in margins)
    return MomentResult(counts, image, sums, mags, len(x), int(located.sum()), edge_guard,
                        margin_guard)


def _camera_kept(cols, args, quantity, g_tables):
    """camera_image's result with the (pixel, weight) pairs it handed to np.bincount."""
    recorder = _Recorder(np.bincount)
    with mock.patch.object(np, 'bincount', recorder):
        res = CR.camera_image(*cols, *args, quantity, g_tables)
    (pix,), kwargs = recorder.calls[0]
    return res, pix, kwargs['weights']


def camera_moments(x, y, z, vx, vy, vz, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity,
                   g_tables=()):
    x, y, z, vx, vy, vz, frac = (np.asarray(c).astype(np.float64) for c in (x, y, z, vx, vy, vz, frac))
    o = np.asarray(o, dtype=np.float64)
    nx, nz = len(uedges) - 1, len(vedges) - 1
    args = (o, C, uedges, vedges, vrplanet, pix_area_cm2)
    res, pix, w = _camera_kept((x, y, z, vy, frac), args, quantity, g_tables)
    # which sample each binned weight belongs to: the same pass over weights 1 and over weights
    # 1 + sample number (column: w = frac / footprint) bins the same samples in the same order; the
    # quotient of the two is the sample's number to a few ulp, and sample numbers are far below 2^52.
    # A hidden sample has weight 0 in all three passes and needs no number: it adds no moment.
    tag = np.arange(1.0, len(x) + 1.0)
    _, pix_one, w_one = _camera_kept((x, y, z, vy, np.ones(len(x))), args, 'column', ())
    _, pix_tag, w_tag = _camera_kept((x, y, z, vy, tag), args, 'column', ())
    assert np.array_equal(pix, pix_one) and np.array_equal(pix, pix_tag)
    assert np.all(w[w_one == 0] == 0)
    seen = w_one != 0
    index = np.rint(w_tag[seen]/w_one[seen]).astype(np.int64) - 1
    assert np.all(np.abs(w_tag[seen]/w_one[seen] - (index + 1)) < 1e-6) and np.all(np.diff(index) > 0)
    pix, w = pix[seen], w[seen]

    vlos = camera_vlos(o, *(c[index] for c in (x, y, z, vx, vy, vz)))
    sums, mags = _sums(pix, w, vlos, nx, nz)
    return MomentResult(res.counts, res.image, sums, mags, res.samples, res.binned, res.edge_guard,
                        res.margin_guard)
