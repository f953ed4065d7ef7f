"""Inputs of the line-of-sight ages tests and the restatement's answer to them, made once and shared
read-only (tests/test_los_ages_cpu.py, tests/test_gpu_los_ages.py).  NumPy only.

The samples and spectra are those of tests/los_edge_cases.py -- a small ball beside the planet,
"hot" lines of sight that look at it, "cold" ones that look away -- with a time column: drawn over
[0, T0], a few rows later than T0 (a negative age: plane 0) and a few that are not a number (plane
NA + 1).  The NA bins lie strictly inside (0, T0), so that a hot spectrum fills `below`, `above`
and every bin; build() asserts it on the restatement."""
import functools

import numpy as np
import pandas as pd

from tests import los_edge_cases as LC
from tests.los_ages_restatement import age_plane, los_ages

D_LINES = (5891, 5897)
T0 = 3000.0
NA, A_LO, A_HI = 7, 400.0, 2500.0
COLUMNS = ('time', 'x', 'y', 'z', 'vy', 'frac')
LATE, NANS = 5, 4                          # rows with time > T0, rows with time = NaN


def times(P, seed=0):
    """The time column of P rows: uniform over [0, T0]; where there are rows enough, LATE of them
    after T0 and NANS of them not a number."""
    rng = np.random.default_rng(5000 + seed)
    t = rng.uniform(0.0, T0, P)
    if P >= 8*(LATE + NANS):
        odd = rng.choice(P, LATE + NANS, replace=False)
        t[odd[:LATE]] = T0 + rng.uniform(1.0, 500.0, LATE)
        t[odd[LATE:]] = np.nan
    return t


def build(smp, ids, pos, look, lines=D_LINES, bins=(NA, T0, A_LO, A_HI), f32=False, filled=True,
          n_index=None):
    """The case of samples ``smp`` (dict of the six COLUMNS, float64), index column ``ids`` (or
    None: one packet, `included` by row) and spectra at ``pos`` looking along ``look``.  f32: the
    device gets float32 columns, the restatement their widened values.  filled: assert that some
    spectrum fills every record.  n_index: packets, where the index column does not name the last."""
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
    if n_index is None:
        n_index = int(ids.max()) + 1 if ids is not None else P
    wide = {c: cols[c].astype(np.float64) for c in COLUMNS}
    wide['Index'] = ids if ids is not None else np.arange(P)
    scd = {c: spectra[c].values for c in spectra.columns}
    want = los_ages(wide, scd, dphi, LC.OUTEREDGE, f.vrplanet, gt, f.R_km*1e5, *bins,
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
    smp['time'] = times(len(ids), seed)
    pos, look = LC.lines_of_sight(S, hot, seed)
    c = build(smp, ids if use_index else None, pos, look, lines, f32=f32)
    cold = np.setdiff1d(np.arange(S), hot)
    assert (c['want'].npackets[cold] == 0).all() and (c['want'].npackets[list(hot)] > 0).all()
    if len(ids) >= 8*(LATE + NANS):
        # the first hot spectrum sees the whole ball: the late rows and the NaN rows among them
        late = np.nonzero(smp['time'] > T0)[0]
        nans = np.nonzero(np.isnan(smp['time']))[0]
        assert len(late) == LATE and len(nans) == NANS
        assert all(c['want'].planes[(hot[0], int(r))] == 0 for r in late)
        assert all(c['want'].planes[(hot[0], int(r))] == NA + 1 for r in nans)
    return c


ALONG_Y = (np.array([[0.0, -8.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
EDGE_BINS = (8, 1024.0, 128.0, 640.0)      # edges a_lo + 64 k and inv_da = 2^-6, all exact


@functools.lru_cache(maxsize=None)
def edge_case(f32):
    """One spectrum at (0, -8, 0) looking along (0, 1, 0), which sees every row.  The times sit on
    each of the nine edges (time = t0 - edge), one ulp of the column's dtype below and above it,
    and at -0.0 (an age of t0: above the range).  Returns (case, the record every row must land
    in), the record by the header's rule in Python floats: whether an ulp of the time survives
    t0 - time depends on the dtype, so nothing else is assumed of it than that the edge itself
    opens its bin."""
    dtype = np.float32 if f32 else np.float64
    na, t0, a_lo, a_hi = EDGE_BINS
    edges = a_lo + np.arange(na + 1)*64.0
    assert edges[-1] == a_hi and float(na)/(a_hi - a_lo) == 2.0**-6
    on = (t0 - edges).astype(dtype)
    assert np.array_equal(on.astype(np.float64), t0 - edges)
    time = np.concatenate([on, np.nextafter(on, dtype(-np.inf)), np.nextafter(on, dtype(np.inf)),
                           [dtype(-0.0)]])
    record = np.array([age_plane(float(t), na, t0, a_lo, a_hi) for t in time])
    assert list(record[:na + 1]) == list(range(1, na + 2)) and record[-1] == na + 1
    # an earlier time is an older row: never a younger bin than the edge's; a later one never an older
    assert np.all(np.isin(record[na + 1:2*na + 2] - record[:na + 1], (0,)))
    assert np.all(np.isin(record[2*na + 2:-1] - record[:na + 1], (-1, 0)))
    assert record[2*na + 2] == 0                              # an ulp younger than a_lo
    assert sorted(set(record)) == list(range(na + 2))         # every record is met
    ids = np.repeat(np.arange(4, dtype=np.int64), (1, 7, 8, 12))
    assert len(ids) == len(time) == 28
    smp = dict(LC.cloud(ids, 5))
    smp['time'] = time.astype(np.float64)
    c = build(smp, ids, *ALONG_Y, bins=EDGE_BINS, f32=f32, filled=False)
    assert c['cols']['time'].dtype == dtype and np.array_equal(c['cols']['time'], time)
    assert np.signbit(c['cols']['time'][-1]) and len(np.unique(c['cols']['frac'])) == 28
    # every row is a used pair of the spectrum, in the record worked out above
    assert c['want'].planes == {(0, r): int(k) for r, k in enumerate(record)}
    return c, record
