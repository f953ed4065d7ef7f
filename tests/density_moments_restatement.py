"""ModelDensity's velocity moments restated with NumPy and scipy (no test lives here).

Per query point the rows within ``dr`` are scipy's (``KDTree.query_ball_point``, the reference's
own call).  Each such row contributes, in fp64 and with one rounding per operation,

    m1_a = f * v_a,  m2_ab = (f * v_a) * v_b,  ff = f * f          (f = frac)

in the order of ``MOMENT_COLUMNS`` -- the very products k_density_moments forms, so device and
restatement add bit-identical terms and differ only in the order of addition.

Tolerance (``Restated.bound`` / ``bound_s0``), derived and not tuned: any order of adding n terms
t_i in fp64 leaves an error of at most (n - 1) 2^-53 sum|t_i| (to first order in 2^-53).  That
holds for the device's order and for NumPy's here, so the two sums differ by at most
(n - 1) 2^-52 sum|t_i|, evaluated per point and per sum from the restatement's own terms.  One
hit or none: the sums must be equal."""
from collections import namedtuple

import numpy as np
from scipy.spatial import KDTree

MOMENT_COLUMNS = ('m1x', 'm1y', 'm1z', 'm2xx', 'm2yy', 'm2zz', 'm2xy', 'm2xz', 'm2yz', 'ff')
Restated = namedtuple('Restated', 'sums s0 counts bound bound_s0')


def products(vx, vy, vz, frac):
    """(P, 10) fp64: the ten terms of every row, each operation rounded once."""
    f, vx, vy, vz = (np.asarray(c).astype(np.float64) for c in (frac, vx, vy, vz))
    fx, fy, fz = f*vx, f*vy, f*vz
    return np.stack([fx, fy, fz, fx*vx, fy*vy, fz*vz, fx*vy, fx*vz, fy*vz, f*f], axis=1)


def sums_over(found, terms, frac):
    """``Restated`` from the rows found per point (lists of row numbers)."""
    Q = len(found)
    frac = np.asarray(frac).astype(np.float64)
    sums, bound = np.zeros((Q, 10)), np.zeros((Q, 10))
    s0, bound_s0, counts = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    for j, rows in enumerate(found):
        n = len(rows)
        counts[j] = n
        if n == 0:
            continue
        rows = np.asarray(rows, dtype=np.int64)
        t = terms[rows]
        sums[j] = t.sum(axis=0)
        bound[j] = (n - 1) * 2.0**-52 * np.abs(t).sum(axis=0)
        s0[j] = frac[rows].sum()
        bound_s0[j] = (n - 1) * 2.0**-52 * np.abs(frac[rows]).sum()
    return Restated(sums, s0, counts, bound, bound_s0)


def restate(points, dr, x, y, z, vx, vy, vz, frac):
    """The ten sums, S0 and the counts per point over the given rows (any float width; widened to
    fp64 first, as the device does)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    data = np.stack([np.asarray(c).astype(np.float64) for c in (x, y, z)], axis=1)
    if len(data) == 0:
        found = [[] for _ in points]
    else:
        found = KDTree(data).query_ball_point(points, dr)
    return sums_over(found, products(vx, vy, vz, frac), frac)


def brute_force(points, dr, x, y, z, vx, vy, vz, frac):
    """The same by a double loop over points and rows, every product formed from Python floats:
    d = q - p, (dx*dx + dy*dy) + dz*dz <= dr*dr."""
    cols = [[float(v) for v in np.asarray(c).astype(np.float64)] for c in (x, y, z, vx, vy, vz, frac)]
    found, terms = [], np.zeros((len(cols[0]), 10))
    for i, (_, _, _, a, b, c, f) in enumerate(zip(*cols)):
        fa, fb, fc = f*a, f*b, f*c
        terms[i] = [fa, fb, fc, fa*a, fb*b, fc*c, fa*b, fa*c, fb*c, f*f]
    for qx, qy, qz in np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist():
        hits = []
        for i, (px, py, pz) in enumerate(zip(*cols[:3])):
            dx, dy, dz = qx - px, qy - py, qz - pz
            if (dx*dx + dy*dy) + dz*dz <= dr*dr:
                hits.append(i)
        found.append(hits)
    return sums_over(found, terms, cols[6]), terms


def check(got_sums, got_s0, got_counts, want, label=''):
    """Counts equal; S0 and every one of the ten sums within the summation bound."""
    assert np.array_equal(got_counts, want.counts), label
    err_s0 = np.abs(np.asarray(got_s0) - want.s0)
    err = np.abs(np.asarray(got_sums) - want.sums)
    with np.errstate(divide='ignore', invalid='ignore'):
        worst = np.nanmax(np.where(want.bound > 0, err / want.bound, 0.), initial=0.)
    print(f'{label} hits {int(want.counts.sum())} worst error / bound {worst:.3f} '
          f'max |S0 error| {err_s0.max(initial=0.):.3e}')
    assert np.all(err_s0 <= want.bound_s0), label
    assert np.all(err <= want.bound), label
