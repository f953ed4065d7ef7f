"""NumPy restatement of the line-of-sight profile of include/nexoclom_hip.h ("Line-of-sight
profile"), written from that text.  It does not call the library.

Which (sample, spectrum) pairs contribute comes from ``oracle.np_oracle.los_iteration``: its
``used`` pairs, the decided pairs with weight > 0.  The header's contributing pairs are those with
wtemp != 0, so every case asserts that no decided pair can have a negative weight (all ``frac`` and
all g-values are >= 0, and the oracle's radiance of every spectrum is the sum of its used pairs'
wtemp: a decided pair with a negative weight would be missing from that sum).  For every used pair
the weight is formed as the oracle forms it (compute_iteration.py:177-196, ModelResult.py:150-161)
and the profile's own terms with the header's operations:

    vlos = (vx*bx + vy*by) + vz*bz
    record spectrum*(nv + 2) + k gets {wtemp, wtemp*wtemp}, k by the cube's rule
        (tests/pixel_cube_restatement.py, ``planes``)
    a = wtemp*vlos;   m1 = a,  m2 = a*vlos,  m3 = (a*vlos)*vlos,  ww = wtemp*wtemp

``los_profile`` returns a ``ProfileResult``: the oracle's radiance, npackets, included and used
pairs {(spectrum, row)}, sums (S, nv + 2, 2), moments (S, 4), moment_mags (S, 4) = the sums of the
terms' magnitudes (what a tolerance on a sum of signed terms is measured by), planes: the record of
every used pair as {(spectrum, row): k}, and bin_guard as ``planes`` gives it."""
from collections import namedtuple

import numpy as np

from oracle import np_oracle as O
from tests.pixel_cube_restatement import planes

ProfileResult = namedtuple('ProfileResult', 'radiance npackets included pairs sums moments '
                                            'moment_mags planes bin_guard')


def pair_terms(samples, sc, i, rows, dphi, vrplanet, g_tables, unit_cm):
    """(wtemp, vlos) of spectrum i's pairs with the sample rows ``rows``."""
    pts = np.stack([samples['x'], samples['y'], samples['z']], axis=1).astype(float)[rows]
    x_sc = np.array([sc['x'][i], sc['y'][i], sc['z'][i]], dtype=float)
    bore = np.array([sc['xbore'][i], sc['ybore'][i], sc['zbore'][i]], dtype=float)
    vx, vy, vz = (np.asarray(samples[c], dtype=float)[rows] for c in ('vx', 'vy', 'vz'))
    frac = np.asarray(samples['frac'], dtype=float)[rows]
    dist = np.linalg.norm(pts - x_sc[np.newaxis, :], axis=1)
    weight = O.packet_weights(frac, vy + vrplanet, 1., 'radiance', g_tables)
    wtemp = weight/(np.pi*(dist*np.sin(dphi))**2*unit_cm**2)
    with np.errstate(all='ignore'):
        vlos = (vx*bore[0] + vy*bore[1]) + vz*bore[2]
    return wtemp, vlos


def los_profile(samples, sc, dphi, outeredge, vrplanet, g_tables, unit_cm, nv, v_lo, v_hi,
                n_index=None):
    """samples: dict x, y, z, vx, vy, vz, frac [, Index]; sc: dict x, y, z, xbore, ybore, zbore; the
    other arguments are los_iteration's and the profile's bins [R/s]."""
    assert np.all(np.asarray(samples['frac']) >= 0) and all(np.all(g >= 0) for _, g in g_tables)
    rad, npack, included, used = O.los_iteration(samples, sc, dphi, outeredge, vrplanet, g_tables,
                                                 unit_cm, n_index=n_index)
    S = len(rad)
    sums = np.zeros((S, nv + 2, 2))
    moments, mags = np.zeros((S, 4)), np.zeros((S, 4))
    pairs, plane_of, guard = set(), {}, np.inf
    for i in range(S):
        rows = np.asarray(used[i], dtype=np.int64)
        if not len(rows):
            assert rad[i] == 0
            continue
        w, vlos = pair_terms(samples, sc, i, rows, dphi, vrplanet, g_tables, unit_cm)
        # the used pairs are the contributing ones: nothing negative was left out of the radiance
        assert np.all(w > 0)
        np.testing.assert_allclose(w.sum(), rad[i], rtol=1e-12, atol=0)
        k, g = planes(vlos, nv, v_lo, v_hi)
        guard = min(guard, g)
        with np.errstate(all='ignore'):
            a = w*vlos
            terms = [a, a*vlos, (a*vlos)*vlos, w*w]
            sums[i, :, 0] = np.bincount(k, weights=w, minlength=nv + 2)
            sums[i, :, 1] = np.bincount(k, weights=w*w, minlength=nv + 2)
            moments[i] = [t.sum() for t in terms]
            mags[i] = [np.abs(t).sum() for t in terms]
        pairs.update((i, int(r)) for r in rows)
        plane_of.update(((i, int(r)), int(kk)) for r, kk in zip(rows, k))
    return ProfileResult(rad, npack, included, pairs, sums, moments, mags, plane_of, guard)
