"""Inputs of the line-of-sight profile tests and the restatement's answer to them, made once and
shared read-only (tests/test_los_profile_cpu.py, tests/test_gpu_los_profile.py).  NumPy only.

The samples and spectra are those of tests/los_edge_cases.py -- a small ball beside the planet,
"hot" lines of sight that look at it, "cold" ones that look away -- with vx and vz drawn N(0, 2e-3)
as its vy is.  The bins (NV over [V_LO, V_HI) R/s, about one sigma either side and off centre) are
chosen so that a hot spectrum fills `below`, `above` and every bin; build() asserts it on the
restatement."""
import functools

import numpy as np
import pandas as pd

from tests import los_edge_cases as LC
from tests.los_profile_restatement import los_profile

D_LINES = (5891, 5897)
NV, V_LO, V_HI = 7, -1.5e-3, 2.5e-3
COLUMNS = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac')


def velocities(P, seed=0):
    """vx, vz of P rows."""
    rng = np.random.default_rng(3000 + seed)
    return rng.normal(0, 2e-3, P), rng.normal(0, 2e-3, P)


def build(smp, ids, pos, look, lines=D_LINES, bins=(NV, V_LO, V_HI), f32=False, filled=True):
    """The case of samples ``smp`` (dict of the seven COLUMNS, float64), index column ``ids`` (or
    None: one packet, `included` by row) and spectra at ``pos`` looking along ``look``.  f32: the
    device gets float32 columns, the restatement their widened values.  filled: assert that some
    spectrum fills every record."""
    from nexoclom_amd.LOSResult import POSITION, BORESIGHT, arccos_threshold, los_geometry
    P, S = len(smp['x']), len(pos)
    dtype = np.float32 if f32 else np.float64
    cols = {c: np.ascontiguousarray(np.asarray(smp[c]).astype(dtype)) for c in COLUMNS}
    spectra = pd.DataFrame(dict(zip(POSITION + BORESIGHT, list(pos.T) + list(look.T))))
    f, gt, dphi = LC.forces(), LC.g_tables(lines), LC.DPHI
    cut, lengths, ladder = los_geometry(spectra, LC.OUTEREDGE, dphi)
    sc = np.vstack([pos.T, look.T, cut, lengths.astype(float)])
    setup = (dphi, np.sin(dphi), np.sin(2*dphi), arccos_threshold(dphi), f.vrplanet, f.R_km*1e5, gt,
             ladder, sc)
    n_index = int(ids.max()) + 1 if ids is not None else P
    wide = {c: cols[c].astype(np.float64) for c in COLUMNS}
    wide['Index'] = ids if ids is not None else np.arange(P)
    scd = {c: spectra[c].values for c in spectra.columns}
    want = los_profile(wide, scd, dphi, LC.OUTEREDGE, f.vrplanet, gt, f.R_km*1e5, *bins,
                       n_index=n_index)
    if filled:
        assert np.any(np.all(want.sums[..., 0] > 0, axis=1)), 'no spectrum fills every record'
    for a in list(cols.values()) + [sc] + [v for v in want if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return dict(P=P, S=S, setup=setup, cols=cols, index=ids, n_index=n_index, want=want, bins=bins,
                lines=lines, n_ladder=len(ladder), m=len(want.pairs))


@functools.lru_cache(maxsize=None)
def case(layout, rows=None, S=6, hot=(0, 2, 3, 5), lines=D_LINES, use_index=True, f32=False, seed=0):
    """A layout of tests/los_edge_cases.py under its lines of sight."""
    ids = LC.layout_ids(layout, rows)
    smp = dict(LC.cloud(ids, seed))
    smp['vx'], smp['vz'] = velocities(len(ids), seed)
    pos, look = LC.lines_of_sight(S, hot, seed)
    c = build(smp, ids if use_index else None, pos, look, lines, f32=f32)
    cold = np.setdiff1d(np.arange(S), hot)
    assert (c['want'].npackets[cold] == 0).all() and (c['want'].npackets[list(hot)] > 0).all()
    return c


ALONG_Y = (np.array([[0.0, -8.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
EDGE_BINS = (8, -2.0**-8, 2.0**-8)            # edges v_lo + k 2^-10 and inv_dv = 1024, all exact


@functools.lru_cache(maxsize=None)
def edge_case(f32):
    """One spectrum at (0, -8, 0) looking along (0, 1, 0): vlos == vy bit for bit.  vy sits on each
    of the nine edges and one ulp of the column's dtype below it, and at -0.0.  Returns (case,
    the record every row must land in)."""
    dtype = np.float32 if f32 else np.float64
    nv, v_lo, v_hi = EDGE_BINS
    edges = (v_lo + np.arange(nv + 1)*2.0**-10).astype(dtype)
    assert np.array_equal(edges.astype(np.float64), v_lo + np.arange(nv + 1)*2.0**-10)
    below = np.nextafter(edges, dtype(-np.inf))
    vy = np.concatenate([edges, below, [dtype(-0.0)]])
    # on edge k: t == k, record 1 + k (nv + 1 on the last); -0.0 is edge nv/2.  One ulp below edge
    # k: record k -- when the rule's subtraction vlos - v_lo keeps the ulp.  A float32 ulp survives
    # it except below the edge at 0, where it is a denormal; a float64 ulp below edges 3 .. 8 is
    # half an ulp of the difference or less and rounds back onto the edge.  So the rule is
    # evaluated here, in Python floats.
    record = np.array([0 if t < 0 else 1 + int(t) if t < nv else nv + 1
                       for t in ((float(v) - v_lo)*(nv/(v_hi - v_lo)) for v in vy)])
    assert list(record[:nv + 1]) == list(range(1, nv + 2)) and record[-1] == 1 + nv//2
    assert record[nv + 1] == 0 and np.all(np.isin(record[nv + 1:-1] - np.arange(nv + 1), (0, 1)))
    kept = record[nv + 1:-1] == np.arange(nv + 1)
    assert list(np.nonzero(~kept)[0]) == ([nv//2] if f32 else list(range(3, nv + 1)))
    ids = np.repeat(np.arange(4, dtype=np.int64), (1, 7, 8, 3))
    assert len(ids) == len(vy) == 19
    smp = dict(LC.cloud(ids, 5))
    smp['vx'], smp['vz'] = velocities(len(ids), 5)
    smp['vy'] = vy.astype(np.float64)
    c = build(smp, ids, *ALONG_Y, bins=EDGE_BINS, f32=f32, filled=False)
    assert c['cols']['vy'].dtype == dtype and np.array_equal(c['cols']['vy'], vy)
    assert np.signbit(c['cols']['vy'][-1]) and len(np.unique(c['cols']['frac'])) == 19
    # every row is a used pair of the spectrum, in the record worked out above
    assert c['want'].planes == {(0, r): int(k) for r, k in enumerate(record)}
    return c, record
