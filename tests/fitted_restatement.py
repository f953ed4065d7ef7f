"""A NumPy / pandas restatement of LOSResultFitted.determine_source_from_data's per-Output loop
(data_simulation/LOSResultFitted.py:136-214), written for the tests: what the GPU fit and the
CPU stand-in are held to.  It walks the spectra one by one as the reference does, over the
`used` rows of the unfitted iteration (oracle.np_oracle.los_iteration), with np.add.at in place of
the reference's one `.loc` update per (pair, spectrum)."""
import numpy as np
import pandas as pd

from oracle import np_oracle as O


def pair_weights(mode, rows, X, spectrum):
    """The reference's per-pair weights of one spectrum (LOSResultFitted.py:152-168)."""
    if mode in ('dist', 'dist2'):
        d = np.sqrt((X['x'].values[rows] - spectrum['x'])**2 +
                    (X['y'].values[rows] - spectrum['y'])**2 +
                    (X['z'].values[rows] - spectrum['z'])**2)
        return 1/d if mode == 'dist' else 1/d**2
    if mode == 'sigma':
        return np.ones(len(rows))/spectrum['sigma']*2
    return np.ones(len(rows))


def refit_output(X, X0_frac, npackets, nsteps, used, data, unfit_radiance, mask, mode, dphi,
                 unit_cm, vrplanet, g_tables, compress=True):
    """One Output.  X: its rows widened to float64 (x, y, z, vy, frac, Index = packet within the
    Output), in stored order; X0_frac: X0's frac (None: every packet started with 1); used[j]:
    positions in X of the rows with weight > 0 for spectrum j.  Returns dict(num, den, cnt,
    mult, frac_fit (fp64, every row), keep (rows save() keeps), frac0_fit, totalsource,
    radiance (not scaled))."""
    index = X['Index'].values.astype(np.int64)
    ratio = (data['radiance'] / unfit_radiance).fillna(0)
    num, den = np.zeros(npackets), np.zeros(npackets)
    cnt = np.zeros(npackets, dtype=np.int64)
    for j in np.flatnonzero(np.asarray(mask, dtype=bool)):
        rows = np.asarray(used[j], dtype=np.int64)
        if len(rows) == 0:
            continue
        w = pair_weights(mode, rows, X, data.iloc[j])
        np.add.at(num, index[rows], ratio.iloc[j]*w)
        np.add.at(den, index[rows], w)
        np.add.at(cnt, index[rows], 1)
    seen = den > 0
    f = np.zeros(npackets)
    f[seen] = num[seen]/den[seen]
    mult = f/f[seen].mean() if seen.any() else np.zeros(npackets)
    frac_fit = X['frac'].values.astype(np.float64)*mult[index]
    keep = frac_fit > 0 if compress else np.ones(len(frac_fit), dtype=bool)
    frac0 = np.ones(npackets) if X0_frac is None else np.asarray(X0_frac, dtype=np.float64)
    frac0_fit = frac0*mult
    totalsource = frac0_fit.sum()*nsteps
    radvel = X['vy'].values + vrplanet
    radiance = pd.Series(np.zeros(len(data)), index=data.index)
    for j in range(len(data)):
        rows = np.asarray(used[j], dtype=np.int64)
        if len(rows) == 0:
            continue
        sp = data.iloc[j]
        rel = np.stack([X[c].values[rows] - sp[c] for c in ('x', 'y', 'z')], axis=1)
        d = np.linalg.norm(rel, axis=1)
        weight = O.packet_weights(frac_fit[rows], radvel[rows], 1., 'radiance', g_tables)
        Apix = np.pi*(d*np.sin(dphi))**2*unit_cm**2
        radiance.iloc[j] = (weight/Apix).sum()
    return dict(num=num, den=den, cnt=cnt, mult=mult, frac_fit=frac_fit, keep=keep,
                frac0_fit=frac0_fit, totalsource=totalsource, radiance=radiance.values)
