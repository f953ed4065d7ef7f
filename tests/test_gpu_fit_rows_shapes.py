"""nxc_fit_rows at the row counts where a stable compaction goes wrong: one row, either side of
a wave and of a 256-row tile, several tiles.  The source store has exactly n rows (n planted
packets without time left, through the adaptive driver's uncompressed row store); a third of the
packets is seen by spectra with a positive ratio, a third by spectra with a negative one, a third
by none.  Expected rows, index, lengths and total: NumPy on the downloaded store and the
downloaded multipliers, bit for bit."""
import numpy as np
import pandas as pd
import pytest

from nexoclom_amd.LOSResult import BORESIGHT, POSITION, arccos_threshold, los_geometry
from tests import helpers as H

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257, 3*256 + 17]
DPHI = np.radians(3.0)
# where the three classes of packets sit, and the spectra that look at the first two from
# further out along the same axis (a line of sight is cut at the planet, so neither group sees
# the other's packets nor those below the planet)
SPOTS = np.array([[3., 0., 0.], [0., 0., 3.], [0., 0., -3.]])
SC_AT = np.array([[6., 0., 0.], [5.5, 0., 0.], [7., 0., 0.], [0., 0., 6.], [0., 0., 5.5], [0., 0., 7.]])
SC_LOOK = np.array([[-1., 0., 0.]]*3 + [[0., 0., -1.]]*3)
RATIO = np.array([2.0, 1.5, 2.5, -0.5, -0.25, -0.75])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def planted(n, classes):
    """n packets without time left: class k sits within 0.01 of SPOTS[k]."""
    rng = np.random.default_rng(1000 + n)
    X0 = H.sample_x0(n, 40 + n, 3000.)
    X0[:, 0] = 0.0
    X0[:, 1:4] = SPOTS[classes] + rng.uniform(-0.01, 0.01, (n, 3))
    X0[:, 5] = rng.normal(0, 2e-4, n)
    X0[:, 7] = rng.uniform(0.1, 1.0, n)
    return X0


def source_store(ctx, X0, narrow):
    H.set_ctx_forces(ctx, H.mercury_forces('Na', 1.3))
    ctx.set_bounce(None)
    ctx.set_bodies(None)
    ctx.upload_packets(X0)
    ctx.integrate_var(1e-4, 25.0, resident=True)
    store, kept = ctx.var_rows_build(narrow=narrow, compress=False)
    assert store.total == len(X0) and kept.all() and store.narrow == narrow
    return store


def seen_pairs(ctx, store, n, pairs):
    """The unfitted line-of-sight pass over the store into `pairs`."""
    f = H.mercury_forces('Na', 1.3)
    spectra = pd.DataFrame(dict(zip(POSITION + BORESIGHT, list(SC_AT.T) + list(SC_LOOK.T))))
    cut, lengths, ladder = los_geometry(spectra, 25., DPHI)
    sc = np.vstack([SC_AT.T, SC_LOOK.T, cut, lengths.astype(float)])
    gt = H.g_tables('Na', f.aplanet, f.R_km, (5891, 5897))
    ctx.los_accumulate(DPHI, np.sin(DPHI), np.sin(2*DPHI), arccos_threshold(DPHI), f.vrplanet,
                       f.R_km*1e5, gt, ladder, sc, n_index=n, rows=(store, 0, n, 0), pairs=pairs)


def check_fit_rows(ctx, n, classes, narrow):
    """Both forms of nxc_fit_rows over a store of n rows; returns the f > 0 mask."""
    store = source_store(ctx, planted(n, classes), narrow)
    pairs = ctx.pairs_create(3*n)
    try:
        seen_pairs(ctx, store, n, pairs)
        assert pairs.count == 3*int((classes < 2).sum())             # three spectra per class
        ctx.fit_set(SC_AT.T, RATIO, np.ones(len(RATIO), dtype=bool))
        ctx.fit_source(rows=(store, 0, n, 0))
        mult = ctx.fit_packets(pairs, n)['mult']
        rows, idx = store.download()
        assert np.array_equal(idx, np.arange(n))
        f = rows[7].astype(np.float64)*mult[idx]
        for compress in (True, False):
            keep = f > 0 if compress else np.ones(n, dtype=bool)
            new, lengths = ctx.fit_rows(n, compress=compress)
            try:
                assert new.total == int(keep.sum()) and new.narrow == narrow
                assert np.array_equal(lengths, np.bincount(idx[keep], minlength=n))
                if new.total:
                    got_rows, got_idx = new.download()
                    assert got_rows.dtype == rows.dtype and got_idx.dtype == idx.dtype
                    assert np.array_equal(got_idx, idx[keep])
                    want = rows[:, keep].copy()
                    want[7] = f[keep].astype(rows.dtype)
                    assert np.array_equal(bits(got_rows), bits(want))
            finally:
                new.free()
    finally:
        pairs.free()
        store.free()
    return f > 0


@pytest.mark.parametrize('narrow', [True, False])
@pytest.mark.parametrize('n', COUNTS)
def test_fit_rows_at_wave_and_tile_boundaries(ctx, n, narrow):
    classes = np.arange(n) % 3
    pos = check_fit_rows(ctx, n, classes, narrow)
    assert np.array_equal(pos, classes == 0)       # the mean of the ratios seen is positive
    if n >= 72:
        assert pos[56:72].any() and not pos[56:72].all()             # across lanes 63 | 64
    if n >= 264:
        assert pos[248:264].any() and not pos[248:264].all()         # across rows 255 | 256


@pytest.mark.parametrize('narrow', [True, False])
@pytest.mark.parametrize('what', ['nothing', 'everything'])
def test_fit_rows_keep_nothing_and_everything(ctx, what, narrow):
    n = 257
    classes = np.full(n, 2 if what == 'nothing' else 0)
    pos = check_fit_rows(ctx, n, classes, narrow)
    assert pos.sum() == (0 if what == 'nothing' else n)
