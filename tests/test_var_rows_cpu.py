"""Output.frame_var_rows: X of an adaptive-step Output framed from its resident rows must be the
frame variable_step_size_driver() builds and save() filters and narrows -- names, order, dtypes,
labels, values.  Host arrays only: no GPU."""
import numpy as np
import pandas as pd
import pytest

from nexoclom_amd.Output import NARROW, STATE_COLS, Output, frame_var_rows

HOST_X0 = STATE_COLS + ['v', 'longitude', 'latitude', 'local_time', 'altitude', 'azimuth']
DEVICE_X0 = STATE_COLS + ['v']                 # what the device sampler leaves (Output._adopt_x0)


def host_path_frame(X0, final, hs, narrow):
    """The host path, statement for statement: Output.__init__ / integrate_batch (X from X0),
    _finish_variable (finals, step_size, Index), save() (frac > 0 filter, 32-bit down-cast)."""
    X = X0.drop(['longitude', 'latitude', 'local_time'], axis=1, errors='ignore')
    X['lossfrac'] = np.zeros(len(final))
    for k, name in enumerate(STATE_COLS):
        X[name] = final[:, k]
    X['step_size'] = hs
    X['Index'] = X.index
    keep = X.frac.values > 0
    if len(X) > 0 and not keep.all():
        X = X[keep]
    return Output._recast(X, NARROW) if narrow else X


def store_arrays(final, narrow):
    """What nxc_var_rows_build delivers for these finals: rows (9, k), index (k,), kept (n,)."""
    kept = final[:, 7] > 0                     # on the 64-bit frac; False for NaN
    rows = np.vstack([final[kept].T, np.zeros((1, int(kept.sum())))])
    index = np.flatnonzero(kept)
    if narrow:
        with np.errstate(over='ignore'):
            return rows.astype(np.float32), index.astype(np.int32), kept
    return rows, index.astype(np.int64), kept


def make(n, columns, seed=5):
    rng = np.random.default_rng(seed)
    X0 = pd.DataFrame({c: rng.normal(size=n) for c in columns})
    final = rng.normal(size=(n, 8))
    final[:, 7] = rng.uniform(0.1, 1.0, n)
    hs = rng.uniform(1.0, 50.0, n)
    return X0, final, hs


FRACS = {
    'mixed': [0.5, 0.0, -0.0, np.nan, -0.5, 1e-300, 1e-46, 1e-10, 1.0, 0.0, 0.25],
    'none kept': [0.0, -0.0, np.nan, -1.0, 0.0, -0.5, 0.0, np.nan, 0.0, 0.0, -2.0],
    'all kept': None,
}


@pytest.mark.parametrize('narrow', [True, False])
@pytest.mark.parametrize('columns', [HOST_X0, DEVICE_X0, []], ids=['host', 'device', 'no X0'])
@pytest.mark.parametrize('case', list(FRACS))
def test_frame_equals_host_path(case, columns, narrow):
    n = 11
    X0, final, hs = make(n, columns)
    if FRACS[case] is not None:
        final[:, 7] = FRACS[case]
    final[2, 1] = 1e39                         # inf in float32
    final[5, 2] = 1.0 + 2.0**-24               # a float32 rounding tie (to even: 1.0)
    with np.errstate(over='ignore'):
        want = host_path_frame(X0.copy(), final, hs, narrow)
    rows, index, kept = store_arrays(final, narrow)
    got = frame_var_rows(rows, index, X0, hs, kept)
    assert list(got.columns) == list(want.columns)
    assert [got[c].dtype for c in got] == [want[c].dtype for c in want]
    assert np.array_equal(got.index.values, want.index.values)
    assert got.index.dtype == want.index.dtype
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert len(got) == {'mixed': 6, 'none kept': 0, 'all kept': n}[case]
    if case == 'mixed' and narrow:
        assert got['frac'].values[2] == 0.0    # 1e-46: kept on the 64-bit frac, narrows to 0


def test_mixed_case_keeps_what_save_keeps():
    X0, final, hs = make(11, HOST_X0)
    final[:, 7] = FRACS['mixed']
    rows, index, kept = store_arrays(final, True)
    got = frame_var_rows(rows, index, X0, hs, kept)
    assert list(got.index) == [0, 5, 6, 7, 8, 10]
    assert list(got['Index']) == [0, 5, 6, 7, 8, 10] and got['Index'].dtype == np.int32
    assert got['frac'].values[2] == 0.0 and got['frac'].values[1] == 0.0    # underflow, kept
    assert np.array_equal(got['v'].values, X0['v'].values[kept].astype(np.float32))
    assert np.array_equal(got['step_size'].values, hs[kept].astype(np.float32))
    assert not got['lossfrac'].values.any()


def test_frame_from_an_already_narrowed_x0():
    """save() narrows X0 before X is first asked for: the extra columns are the same float32."""
    X0, final, hs = make(9, HOST_X0)
    final[3, 7] = 0.0
    want = host_path_frame(X0.copy(), final, hs, True)
    rows, index, kept = store_arrays(final, True)
    got = frame_var_rows(rows, index, Output._recast(X0, NARROW), hs, kept)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
