"""ModelDensity's spectrum restated with NumPy and scipy (no test lives here).

Per query point the rows within ``dr`` are scipy's (``KDTree.query_ball_point``, the reference's
own call).  Each such row is taken through steps 1-7 of include/nexoclom_hip.h, "Density
spectrum", in fp64 with one operation per line -- the very operations k_density_spectrum makes,
so device and restatement add bit-identical terms to the same records and differ only in the
order of addition.  The restatement itself adds every sum in row order, one addition after the
other (``in_order``), which makes it equal to ``brute_force`` bit for bit.

Tolerance (``Restated.bound`` / ``bound_s0``), derived and not tuned, the one of
tests/density_moments_restatement.py: any order of adding n terms t_i in fp64 leaves an error of
at most (n - 1) 2^-53 sum|t_i| (to first order in 2^-53).  That holds for the device's order and
for the row order here, so the two sums differ by at most (n - 1) 2^-52 sum|t_i|, evaluated per
record and per sum from the restatement's own terms.  One term or none: the sums must be equal."""
from collections import namedtuple

import numpy as np
from scipy.spatial import KDTree

# sums, bound: (2, Q, nv + 2, 2); seen: (Q, nv + 2) rows per record; s0, counts, bound_s0: (Q,)
Restated = namedtuple('Restated', 'sums s0 counts seen bound bound_s0')


def in_order(terms):
    """The sum of ``terms`` added one after the other from the first (``np.sum`` adds in pairs from
    eight terms on); 0 for none."""
    return np.add.accumulate(terms)[-1] if len(terms) else 0.0


def frames_of(u, b, Q):
    """(Q, 8) frame records ux uy uz 0 bx by bz 0 from (3,) or (Q, 3) velocities and boresights."""
    frames = np.zeros((Q, 8))
    frames[:, 0:3] = u
    frames[:, 4:7] = b
    return frames


def row_terms(frame, nv, s_lo, inv_ds, cos_half, all_sky, vx, vy, vz, f):
    """Steps 1-5 and the terms of step 7 for rows (fp64 arrays) against one frame record:
    (seen, k, f, f f, g, g g)."""
    with np.errstate(invalid='ignore', over='ignore'):
        cx = vx - frame[0]
        cy = vy - frame[1]
        cz = vz - frame[2]
        xx = cx * cx
        yy = cy * cy
        zz = cz * cz
        s2 = xx + yy
        s2 = s2 + zz
        s = np.sqrt(s2)
        ax = cx * frame[4]
        ay = cy * frame[5]
        az = cz * frame[6]
        a = ax + ay
        a = a + az
        a = -a
        lim = cos_half * s
        seen = (a >= lim) | bool(all_sky)
        t = s - s_lo
        t = t * inv_ds
        k = np.full(len(t), nv + 1, dtype=np.int64)
        inside = (t >= 0) & (t < nv)
        k[inside] = 1 + t[inside].astype(np.int64)
        k[t < 0] = 0
        ff = f * f
        g = f * s
        gg = g * g
    return seen, k, f, ff, g, gg


def sums_over(found, frames, nv, s_lo, inv_ds, cos_half, all_sky, vx, vy, vz, frac):
    """``Restated`` from the rows found per point (lists of row numbers)."""
    Q = len(found)
    vx, vy, vz, frac = (np.asarray(c).astype(np.float64) for c in (vx, vy, vz, frac))
    sums, bound = np.zeros((2, Q, nv + 2, 2)), np.zeros((2, Q, nv + 2, 2))
    seen_n = np.zeros((Q, nv + 2))
    s0, bound_s0, counts = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    for j, rows in enumerate(found):
        n = len(rows)
        counts[j] = n
        if n == 0:
            continue
        rows = np.sort(np.asarray(rows, dtype=np.int64))
        s0[j] = in_order(frac[rows])
        bound_s0[j] = (n - 1) * 2.0**-52 * np.abs(frac[rows]).sum()
        seen, k, f, ff, g, gg = row_terms(frames[j], nv, s_lo, inv_ds, cos_half, all_sky,
                                          vx[rows], vy[rows], vz[rows], frac[rows])
        for plane in np.unique(k[seen]):
            pick = seen & (k == plane)
            m = int(pick.sum())
            seen_n[j, plane] = m
            for where, term in (((0, j, plane, 0), f), ((0, j, plane, 1), ff),
                                ((1, j, plane, 0), g), ((1, j, plane, 1), gg)):
                sums[where] = in_order(term[pick])
                bound[where] = (m - 1) * 2.0**-52 * np.abs(term[pick]).sum()
    return Restated(sums, s0, counts, seen_n, bound, bound_s0)


def restate(points, dr, frames, nv, s_lo, s_hi, cos_half, all_sky, x, y, z, vx, vy, vz, frac):
    """The two planes, S0, the counts and the seen rows per record over the given rows (any float
    width; widened to fp64 first, as the device does).  ``frames``: (Q, 8) in the points' order."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    data = np.stack([np.asarray(c).astype(np.float64) for c in (x, y, z)], axis=1)
    if len(data) == 0:
        found = [[] for _ in points]
    else:
        found = KDTree(data).query_ball_point(points, dr)
    inv_ds = nv / (s_hi - s_lo)
    return sums_over(found, np.asarray(frames, dtype=np.float64), nv, s_lo, inv_ds, cos_half,
                     all_sky, vx, vy, vz, frac)


def brute_force(points, dr, frames, nv, s_lo, s_hi, cos_half, all_sky, x, y, z, vx, vy, vz, frac):
    """The same by a double loop over points and rows, every operation on Python floats, adding in
    row order: (sums, s0, counts, seen rows per record)."""
    import math
    cols = [[float(v) for v in np.asarray(c).astype(np.float64)] for c in (x, y, z, vx, vy, vz, frac)]
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()
    frames = np.asarray(frames, dtype=np.float64).tolist()
    inv_ds = nv / (s_hi - s_lo)
    Q = len(pts)
    sums, seen_n = np.zeros((2, Q, nv + 2, 2)), np.zeros((Q, nv + 2))
    s0, counts = np.zeros(Q), np.zeros(Q)
    for j, ((qx, qy, qz), fr) in enumerate(zip(pts, frames)):
        for px, py, pz, a_, b_, c_, f in zip(*cols):
            dx, dy, dz = qx - px, qy - py, qz - pz
            if not (dx*dx + dy*dy) + dz*dz <= dr*dr:
                continue
            s0[j] += f
            counts[j] += 1
            cx, cy, cz = a_ - fr[0], b_ - fr[1], c_ - fr[2]
            s2 = (cx*cx + cy*cy) + cz*cz
            s = math.sqrt(s2) if s2 == s2 else s2
            a = -((cx*fr[4] + cy*fr[5]) + cz*fr[6])
            if not (all_sky or a >= cos_half*s):
                continue
            t = (s - s_lo)*inv_ds
            k = 0 if t < 0 else 1 + int(t) if t < nv else nv + 1
            g = f*s
            seen_n[j, k] += 1
            sums[0, j, k, 0] += f
            sums[0, j, k, 1] += f*f
            sums[1, j, k, 0] += g
            sums[1, j, k, 1] += g*g
    return sums, s0, counts, seen_n


def seen_counts(sums):
    """Rows per record from device sums of a case with frac = 1: plane 0 then holds {n, n}."""
    return np.asarray(sums)[0, :, :, 0]


def check(got_sums, got_s0, got_counts, want, label=''):
    """Counts equal; S0 and every sum of the two planes within the summation bound."""
    assert np.array_equal(got_counts, want.counts), label
    got_sums = np.asarray(got_sums)
    assert got_sums.shape == want.sums.shape, label
    # a sum that a NaN has reached (a planted non-finite velocity) must be NaN on both sides
    both_nan = np.isnan(got_sums) & np.isnan(want.sums)
    assert np.array_equal(np.isnan(got_sums), np.isnan(want.sums)), label
    err_s0 = np.abs(np.asarray(got_s0) - want.s0)
    with np.errstate(divide='ignore', invalid='ignore'):
        err = np.where(both_nan, 0., np.abs(got_sums - want.sums))
        worst = np.nanmax(np.where(want.bound > 0, err / want.bound, 0.), initial=0.)
    print(f'{label} hits {int(want.counts.sum())} seen {int(want.seen.sum())} worst error / bound '
          f'{worst:.3f} max |S0 error| {err_s0.max(initial=0.):.3e}')
    assert np.all(err_s0 <= want.bound_s0), label
    assert np.all(both_nan | (err <= want.bound)), label
    # an empty record stays empty: its sums are exact zeros on both sides
    assert not got_sums[:, want.seen == 0].any(), label
