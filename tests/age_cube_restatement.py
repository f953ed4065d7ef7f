"""NumPy restatement of the age cube of include/nexoclom_hip.h ("Age cube"), written from that
text.  It does not call the library.

The per-sample (pixel, w, sample) come as in tests/pixel_cube_restatement.py: from the recorders of
tests/pixel_moments_restatement.py (the oracle's ``create_image`` for the image,
tests/camera_restatement.py for the camera).  Written out here, with the header's operations:

    inv_da = na / (a_hi - a_lo)                                   formed once, fp64
    age = t0 - (double)time
    u = (age - a_lo) * inv_da
    k = 0 if u < 0;   1 + (int)u if 0 <= u < na;   na + 1 otherwise (also time not a number)
    {w, w*w} added to record pix*(na + 2) + k                     (w != 0 only)

and the contraction of nxc_*_ages_apply, ``apply_ordered``: per (pixel, epoch) the sums over
k = 0 .. na + 1 in that order from 0.0, one rounding per operation.

``image_ages`` / ``camera_ages`` return an ``AgesResult``: counts, image, sums (nx, nz, na + 2, 2),
abs_sums (the same shape: sum |w| and sum w*w), packets (nx, nz, na + 2: samples filed per plane),
the samples offered and binned, the two guards of the camera restatement and ``bin_guard``, the
smallest distance of any u in [0, na] to an integer (inf when there is none)."""
from collections import namedtuple
from unittest import mock

import numpy as np

from tests import camera_restatement as CR
from tests import pixel_moments_restatement as PM
from tests.pixel_cube_restatement import _Kept

AgesResult = namedtuple('AgesResult', 'counts image sums abs_sums packets samples binned '
                                      'edge_guard margin_guard bin_guard')


def planes(time, na, t0, a_lo, a_hi):
    """The plane of every row time (float32 times are widened) and the bin guard of them all."""
    na = int(na)
    inv_da = np.float64(na)/(np.float64(a_hi) - np.float64(a_lo))
    with np.errstate(all='ignore'):
        age = np.float64(t0) - np.asarray(time).astype(np.float64)
        u = (age - np.float64(a_lo))*inv_da
        inside = (u >= 0) & (u < na)
        k = np.full(u.shape, na + 1, dtype=np.int64)
        k[u < 0] = 0
        k[inside] = 1 + u[inside].astype(np.int64)
    near = u[(u >= 0) & (u <= na)]
    guard = float(np.min(np.abs(near - np.rint(near)))) if near.size else np.inf
    return k, guard


def _file(pix, w, time, nx, nz, na, t0, a_lo, a_hi):
    use = w != 0
    pix, w, time = pix[use], w[use], time[use]
    k, guard = planes(time, na, t0, a_lo, a_hi)
    rec = pix*(na + 2) + k
    n = nx*nz*(na + 2)
    terms = [w, w*w]
    sums = np.stack([np.bincount(rec, weights=t, minlength=n) for t in terms], axis=1)
    mags = np.stack([np.bincount(rec, weights=np.abs(t), minlength=n) for t in terms], axis=1)
    packets = np.bincount(rec, minlength=n).reshape(nx, nz, na + 2)
    return sums.reshape(nx, nz, na + 2, 2), mags.reshape(nx, nz, na + 2, 2), packets, guard


def image_ages(time, x, y, z, vy, frac, vrplanet, M, quantity, g_tables, dims, xrange_, zrange_,
               apix_cm2, na, t0, a_lo, a_hi):
    time, x, y, z, vy, frac = (np.asarray(c).astype(np.float64) for c in (time, x, y, z, vy, frac))
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    nx, nz = dims
    zero = np.zeros(len(x))
    recorder = _Kept(np.histogram2d)
    with mock.patch.object(np, 'histogram2d', recorder):
        base = PM.image_moments(x, y, z, zero, vy, zero, frac, vrplanet, M, quantity, g_tables, dims,
                                xrange_, zrange_, apix_cm2)
    ((xo, zo), kwargs), (_, ex, ez) = recorder.calls[0], recorder.results[0]
    w = kwargs['weights']
    ix, iz = CR._bins(xo, ex), CR._bins(zo, ez)
    located = (ix >= 0) & (iz >= 0)
    pix = (ix*nz + iz)[located]
    assert np.array_equal(np.bincount(pix, minlength=nx*nz).reshape(nx, nz), base.counts)
    sums, mags, packets, guard = _file(pix, w[located], time[located], nx, nz, na, t0, a_lo, a_hi)
    return AgesResult(base.counts, base.image, sums, mags, packets, base.samples, base.binned,
                      base.edge_guard, base.margin_guard, guard)


def camera_ages(time, x, y, z, vy, frac, o, C, uedges, vedges, vrplanet, pix_area_cm2, quantity,
                g_tables, na, t0, a_lo, a_hi):
    time, x, y, z, vy, frac = (np.asarray(c).astype(np.float64) for c in (time, x, y, z, vy, frac))
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
    sums, mags, packets, guard = _file(pix[seen], w[seen], time[index], nx, nz, na, t0, a_lo, a_hi)
    return AgesResult(res.counts, res.image, sums, mags, packets, res.samples, res.binned,
                      res.edge_guard, res.margin_guard, guard)


def apply_ordered(sums, K):
    """out (ne,) + pixels + (2,): {sum_k S K, sum_k WW (K K)} added plane after plane from 0.0,
    every product and every sum rounded once -- what k_ages_apply computes, bit for bit."""
    sums = np.asarray(sums, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    planes_, ne = K.shape
    assert sums.shape[-2:] == (planes_, 2)
    pixels = sums.shape[:-2]
    out = np.zeros((ne,) + pixels + (2,))
    for e in range(ne):
        s, ww = np.zeros(pixels), np.zeros(pixels)
        for k in range(planes_):
            c = K[k, e]
            s = s + sums[..., k, 0]*c
            ww = ww + sums[..., k, 1]*(c*c)
        out[e, ..., 0], out[e, ..., 1] = s, ww
    return out


def apply_plan(planes_, ne, lds_bytes):
    """(stride, run, chunk) of ages_apply_plan (nxc_ages_check.hpp), restated: the pixel run and
    the epoch chunk of a workgroup of k_ages_apply; None when nothing fits."""
    stride = planes_ | 1
    least = stride*16 + planes_*8
    if planes_ < 3 or ne < 1 or least > lds_bytes:
        return None
    budget = min(lds_bytes, max(32*1024, least))
    chunk = max(1, min(ne, 64, ((budget - stride*16)//2)//(planes_*8)))
    run = max(1, min(256, (budget - planes_*chunk*8)//(stride*16)))
    return stride, run, chunk
