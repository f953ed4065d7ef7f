"""NumPy restatement of "ShellMap ages" (include/nexoclom_hip.h), on top of the per-sample steps of
tests/shell_map_restatement.py ("ShellMap", steps 1 to 8) and the plane rule of
tests/age_cube_restatement.py ("Age cube").  It does not call the library.

``shell_ages(time, x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt,
na, t0, a_lo, a_hi)`` returns a ``ShellAges``:

* ``base``: the ``ShellResult`` of the same samples -- counts, column, planes A and B, the counters
  and the three guards (edge, sunlit margin, altitude bin), which the ages pass must reproduce;
* ``block`` (2, nlon, nlat, nalt + 2, na + 2, 2): age plane A {w, w*w} and age plane B {c, c*c} per
  record and age plane, every sum added in row order (np.bincount adds its weights one after the
  other), so that a plain double loop gives the same bits; ``abs_block``: the sum of |term|;
* ``rows`` (nlon, nlat, nalt + 2, na + 2): the filed rows per record of the block;
* ``edge_guard``, ``margin_guard``, ``bin_guard``: the base's.  The age plane needs no guard: it is a
  fixed sequence of fp64 operations, which NumPy repeats exactly (``age_guard``, the distance of the
  nearest u to an integer, is given for information only).

``bound(want, n)``: the tolerance of a sum added in another order than this one, derived in
tests/density_spectrum_restatement.py and not measured: two orders of adding n terms t_i in fp64
differ by at most (n - 1) 2^-52 sum |t_i|, per record and sum."""
from collections import namedtuple

import numpy as np

from tests.age_cube_restatement import planes
from tests.shell_map_restatement import shell_map, shell_samples

ShellAges = namedtuple('ShellAges', 'base block abs_block rows edge_guard margin_guard bin_guard '
                                    'age_guard')
GUARD = 1e-9


def shell_ages(time, x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt,
               na, t0, a_lo, a_hi):
    args = (x, y, z, vy, frac, vrplanet, quantity, g_tables, nlon, nlat, r_lo, r_hi, nalt)
    base = shell_map(*args)
    s = shell_samples(*args)
    filed = s['filed']
    time = np.asarray(time).astype(np.float64)[filed]           # only a filed row's time is read
    ka, age_guard = planes(time, na, t0, a_lo, a_hi)
    rec = s['cell'][filed]*(nalt + 2) + s['k'][filed]
    arec = rec*(na + 2) + ka
    n = nlon*nlat*(nalt + 2)*(na + 2)
    w, c = s['w'][filed], s['c'][filed]
    with np.errstate(all='ignore'):
        terms = [[w, w*w], [c, c*c]]
    shape = (2, nlon, nlat, nalt + 2, na + 2, 2)
    block = np.array([[np.bincount(arec, weights=t, minlength=n) for t in plane] for plane in terms])
    mags = np.array([[np.bincount(arec, weights=np.abs(t), minlength=n) for t in plane]
                     for plane in terms])
    block = np.moveaxis(block, 1, 2).reshape(shape)
    mags = np.moveaxis(mags, 1, 2).reshape(shape)
    rows = np.bincount(arec, minlength=n).reshape(shape[1:-1])
    return ShellAges(base, block, mags, rows, base.edge_guard, base.margin_guard, base.bin_guard,
                     age_guard)


def guards_hold(want):
    return min(want.edge_guard, want.margin_guard, want.bin_guard) >= GUARD


def bound(want, n=None):
    """(n - 1) 2^-52 sum |term| per entry of the block; ``n`` (rows per record, the block's shape
    without its first and last axis) defaults to the restatement's own rows."""
    n = want.rows if n is None else np.asarray(n)
    return (np.maximum(n - 1, 0)*2.0**-52)[None, ..., None]*want.abs_block
