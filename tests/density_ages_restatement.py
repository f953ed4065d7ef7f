"""ModelDensity's ages restated with NumPy (no test lives here), from include/nexoclom_hip.h,
"Density ages".  It does not call the library.

Per query point the rows within ``dr`` are scipy's (``KDTree.query_ball_point``, the reference's
own call) when scipy is there; without it ``members`` runs the file's own double loop of
query_ball_point's test, ``(dx dx + dy dy) + dz dz <= dr dr`` in fp64, for every caller.  The
plane of a member row is tests/age_cube_restatement.planes' (the header's operations, one per
line), and the row adds {f, f f} to record (point, plane) and {f, 1} to the point -- the very
terms k_density_ages adds, so device and restatement differ only in the order of addition.  The
restatement adds every sum in row order, one addition after the other (``in_order``), which makes
it equal to ``brute_force`` bit for bit.

Tolerance (``Restated.bound`` / ``bound_s0``), derived and not tuned, the one of
tests/density_spectrum_restatement.py: two orders of adding n terms t_i in fp64 differ by at most
(n - 1) 2^-52 sum|t_i|, evaluated per record and per sum from the restatement's own terms.  One
term or none: the sums must be equal."""
from collections import namedtuple

import numpy as np

from tests.age_cube_restatement import planes
from tests.density_spectrum_restatement import in_order

try:
    from scipy.spatial import KDTree
except ImportError:                          # the double loop below serves every test then
    KDTree = None

# sums, bound: (Q, na + 2, 2); rows: (Q, na + 2) rows per record; s0, counts, bound_s0: (Q,)
Restated = namedtuple('Restated', 'sums s0 counts rows bound bound_s0 bin_guard')


def members(points, dr, data):
    """Per point the row numbers of ``data`` (p, 3) within ``dr``: scipy's, else a double loop."""
    if len(data) == 0:
        return [[] for _ in points]
    if KDTree is not None:
        return KDTree(data).query_ball_point(points, dr)
    found = []
    for q in points:
        d = q - data
        found.append(np.flatnonzero((d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2] <= dr*dr))
    return found


def restate(points, dr, na, t0, a_lo, a_hi, time, x, y, z, frac):
    """The block, S0, the counts and the rows per record over the given rows (any float width;
    widened to fp64 first, as the device does)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    data = np.stack([np.asarray(c).astype(np.float64) for c in (x, y, z)], axis=1)
    frac = np.asarray(frac).astype(np.float64)
    k, guard = planes(time, na, t0, a_lo, a_hi)
    Q = len(points)
    sums, bound, rows_n = np.zeros((Q, na + 2, 2)), np.zeros((Q, na + 2, 2)), np.zeros((Q, na + 2))
    s0, bound_s0, counts = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    for j, rows in enumerate(members(points, dr, data)):
        n = len(rows)
        counts[j] = n
        if n == 0:
            continue
        rows = np.sort(np.asarray(rows, dtype=np.int64))
        f = frac[rows]
        with np.errstate(invalid='ignore', over='ignore'):
            ff = f * f
            s0[j] = in_order(f)
            bound_s0[j] = (n - 1) * 2.0**-52 * np.abs(f).sum()
            for plane in np.unique(k[rows]):
                pick = k[rows] == plane
                m = int(pick.sum())
                rows_n[j, plane] = m
                for col, term in ((0, f), (1, ff)):
                    sums[j, plane, col] = in_order(term[pick])
                    bound[j, plane, col] = (m - 1) * 2.0**-52 * np.abs(term[pick]).sum()
    return Restated(sums, s0, counts, rows_n, bound, bound_s0, guard)


def brute_force(points, dr, na, t0, a_lo, a_hi, time, x, y, z, frac):
    """The same by a double loop over points and rows, every operation on Python floats, adding in
    row order: (sums, s0, counts, rows per record)."""
    cols = [[float(v) for v in np.asarray(c).astype(np.float64)] for c in (time, x, y, z, frac)]
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()
    t0, a_lo, a_hi = float(t0), float(a_lo), float(a_hi)
    inv_da = float(na) / (a_hi - a_lo)
    Q = len(pts)
    sums, rows_n = np.zeros((Q, na + 2, 2)), np.zeros((Q, na + 2))
    s0, counts = np.zeros(Q), np.zeros(Q)
    for j, (qx, qy, qz) in enumerate(pts):
        for t, px, py, pz, f in zip(*cols):
            dx, dy, dz = qx - px, qy - py, qz - pz
            if not (dx*dx + dy*dy) + dz*dz <= dr*dr:
                continue
            s0[j] += f
            counts[j] += 1
            age = t0 - t
            u = (age - a_lo) * inv_da
            k = 0 if u < 0 else 1 + int(u) if u < na else na + 1
            rows_n[j, k] += 1
            sums[j, k, 0] += f
            sums[j, k, 1] += f*f
    return sums, s0, counts, rows_n


def rows_per_record(sums):
    """Rows per record from device sums of a pass with frac = 1: every record then holds {n, n}."""
    sums = np.asarray(sums)
    assert np.array_equal(sums[..., 0], sums[..., 1])
    return sums[..., 0]


def check(got, want, label=''):
    """``got`` = (sums, S0, counts) or (sums, S0, counts, rows per record | None) of the device.
    Counts equal (and the rows per record, where a frac = 1 pass gave them); S0 and every sum
    of the block within the summation bound; an empty record holds exact zeros."""
    got_sums, got_s0, got_counts, got_rows = (*got, None)[:4]
    assert np.array_equal(got_counts, want.counts), label
    got_sums = np.asarray(got_sums)
    assert got_sums.shape == want.sums.shape, label
    if got_rows is not None:
        assert np.array_equal(got_rows, want.rows), label
    both_nan = np.isnan(got_sums) & np.isnan(want.sums)
    assert np.array_equal(np.isnan(got_sums), np.isnan(want.sums)), label
    err_s0 = np.abs(np.asarray(got_s0) - want.s0)
    with np.errstate(divide='ignore', invalid='ignore'):
        err = np.where(both_nan, 0., np.abs(got_sums - want.sums))
        worst = np.nanmax(np.where(want.bound > 0, err / want.bound, 0.), initial=0.)
    print(f'{label} hits {int(want.counts.sum())} worst error / bound {worst:.3f} '
          f'max |S0 error| {err_s0.max(initial=0.):.3e}')
    assert np.all(err_s0 <= want.bound_s0), label
    assert np.all(both_nan | (err <= want.bound)), label
    assert not got_sums[want.rows == 0].any(), label


def check_exact(got, want, label=''):
    """``got`` as for ``check``.  A dyadic scene: every sum is exact in fp64 whatever the order,
    so all is ``array_equal``."""
    got_sums, got_s0, got_counts, got_rows = (*got, None)[:4]
    assert np.array_equal(got_counts, want.counts), label
    if got_rows is not None:
        assert np.array_equal(got_rows, want.rows), label
    assert np.array_equal(got_s0, want.s0), label
    assert np.array_equal(got_sums, want.sums, equal_nan=True), label
