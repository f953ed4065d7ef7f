"""NumPy restatement of the line-of-sight ages of include/nexoclom_hip.h ("Line-of-sight ages"),
written from that text.  It does not call the library.

Which (sample, spectrum) pairs contribute, and with which wtemp, is what the profile's restatement
works out (tests/los_profile_restatement.py: ``O.los_iteration``'s used pairs, ``pair_terms``, and
the assertion that no decided pair has a negative weight).  The plane of a pair is the header's
rule, evaluated per pair in Python floats, one rounding per operation:

    age = t0 - time;   u = (age - a_lo)*inv_da,   inv_da = na/(a_hi - a_lo)
    k = 0 if u < 0,   1 + int(u) if 0 <= u < na,   na + 1 otherwise (a_hi and above; time a NaN)

and the pair adds {wtemp, wtemp*wtemp} to record spectrum*(na + 2) + k.

``los_ages`` returns an ``AgesResult``: the oracle's radiance, npackets, included and used pairs
{(spectrum, row)}, sums (S, na + 2, 2) and planes: the record of every used pair as
{(spectrum, row): k}."""
from collections import namedtuple

import numpy as np

from oracle import np_oracle as O
from tests.los_profile_restatement import pair_terms

AgesResult = namedtuple('AgesResult', 'radiance npackets included pairs sums planes')


def age_plane(time, na, t0, a_lo, a_hi):
    """The plane of one row's time (a Python float) by the header's rule."""
    inv_da = float(na)/(a_hi - a_lo)
    age = t0 - time
    u = (age - a_lo)*inv_da
    if u < 0.0:
        return 0
    if u < float(na):
        return 1 + int(u)
    return na + 1


def los_ages(samples, sc, dphi, outeredge, vrplanet, g_tables, unit_cm, na, t0, a_lo, a_hi,
             n_index=None):
    """samples: dict time, x, y, z, vy, frac [, Index]; sc: dict x, y, z, xbore, ybore, zbore; the
    other arguments are los_iteration's and the age bins [s]."""
    assert np.all(np.asarray(samples['frac']) >= 0) and all(np.all(g >= 0) for _, g in g_tables)
    rad, npack, included, used = O.los_iteration(samples, sc, dphi, outeredge, vrplanet, g_tables,
                                                 unit_cm, n_index=n_index)
    # pair_terms also forms vlos: the velocities it reads are of no account here
    zeros = np.zeros(len(samples['x']))
    with_v = dict(samples, vx=zeros, vz=zeros)
    time = np.asarray(samples['time'], dtype=np.float64)
    S = len(rad)
    sums = np.zeros((S, na + 2, 2))
    pairs, plane_of = set(), {}
    for i in range(S):
        rows = np.asarray(used[i], dtype=np.int64)
        if not len(rows):
            assert rad[i] == 0
            continue
        w, _ = pair_terms(with_v, sc, i, rows, dphi, vrplanet, g_tables, unit_cm)
        assert np.all(w > 0)
        np.testing.assert_allclose(w.sum(), rad[i], rtol=1e-12, atol=0)
        k = np.array([age_plane(float(t), na, t0, a_lo, a_hi) for t in time[rows]], dtype=np.int64)
        sums[i, :, 0] = np.bincount(k, weights=w, minlength=na + 2)
        sums[i, :, 1] = np.bincount(k, weights=w*w, minlength=na + 2)
        pairs.update((i, int(r)) for r in rows)
        plane_of.update(((i, int(r)), int(kk)) for r, kk in zip(rows, k))
    return AgesResult(rad, npack, included, pairs, sums, plane_of)
