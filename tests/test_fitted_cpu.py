"""LOSResultFitted without a GPU: make_mask, determine_source_rate, and the fitted flow
(LOSResultFitted.determine_source_from_data) on a NumPy stand-in of the device -- the pairs come
from oracle.np_oracle.los_iteration's `used` -- against the pandas restatement of
LOSResultFitted.py:136-214 (tests/fitted_restatement.py); a two-rank run over gloo equals one
rank; the ctypes layout of nxc_fit_desc matches the header."""
import contextlib
import ctypes as C
import io
import multiprocessing as mp
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

import nexoclom_amd
from nexoclom_amd import Input, LOSResult, LOSResultFitted, SpacecraftData, hip_api
from oracle import np_oracle as O
from tests.fitted_restatement import refit_output
from tests.oracle_context import OracleContext, OracleRowStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(os.path.dirname(nexoclom_amd.__file__), 'inputfiles',
                     'Na.mercury.bench.input')
N, SIZE = 1000, 500                      # two Outputs of 500 packets


class StandInPairs:
    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.pairs = np.zeros((2, 0), dtype=np.int64)

    @property
    def count(self):
        return self.pairs.shape[1]

    def download(self):
        return self.pairs.copy()

    def free(self):
        pass


def _stand_in():
    class FitContext(OracleContext):
        """The C-oracle stand-in plus NumPy versions of the pair list and the fit_* calls."""

        def pairs_create(self, capacity):
            return StandInPairs(capacity)

        def los_accumulate(self, dphi, sin_dphi, sin_2dphi, cos_threshold, vrplanet, unit_cm,
                           g_tables, ladder, sc, x=None, y=None, z=None, vy=None, frac=None,
                           index=None, n_index=0, used_cap=0, rows=None, pairs=None):
            if rows is not None:
                store, first, count, shift = rows
                r, idx = store.download(first, count)
                x, y, z, vy, frac = r[1], r[2], r[3], r[5], r[7]
                index = idx.astype(np.int64) - shift
            smp = dict(x=np.asarray(x, float), y=np.asarray(y, float), z=np.asarray(z, float),
                       vy=np.asarray(vy, float), frac=np.asarray(frac, float))
            if index is not None:
                smp['Index'] = np.asarray(index)
            scd = dict(zip(('x', 'y', 'z', 'xbore', 'ybore', 'zbore'), np.asarray(sc)[:6]))
            radiance, npackets, included, used = O.los_iteration(
                smp, scd, dphi, self.los_outeredge, vrplanet, list(g_tables), unit_cm,
                n_index=n_index or None)
            if pairs is not None:
                spec = np.concatenate([np.full(len(u), j) for j, u in enumerate(used)])
                row = np.concatenate(used)
                pairs.pairs = np.stack([spec, row]).astype(np.int64)
                if pairs.count > pairs.capacity:
                    raise hip_api.HipError('pair list overflow', hip_api.NXC_ERR_OVERFLOW)
            return dict(radiance=radiance, npackets=npackets, included=included, used=None,
                        n_used=0)

        def fit_set(self, position, ratio, mask, weight_mode=None, weight=None):
            self._fit = dict(pos=np.asarray(position, float).reshape(3, -1),
                             ratio=np.asarray(ratio, float), mask=np.asarray(mask, bool),
                             mode=weight_mode, weight=None if weight is None else
                             np.asarray(weight, float))
            self._fit_rad = np.zeros(len(self._fit['ratio']))

        def fit_source(self, x=None, y=None, z=None, vy=None, frac=None, index=None, rows=None):
            self._src_rows = rows
            if rows is not None:
                store, first, count, shift = rows
                r, idx = store.download(first, count)
                x, y, z, vy, frac = r[1], r[2], r[3], r[5], r[7]
                index = idx.astype(np.int64) - shift
            self._src = dict(x=np.asarray(x, float), y=np.asarray(y, float),
                             z=np.asarray(z, float), vy=np.asarray(vy, float),
                             frac=np.asarray(frac, float), index=np.asarray(index, np.int64))

        def fit_packets(self, pairs, n_packets):
            F, s = self._fit, self._src
            spec, row = pairs.pairs
            on = F['mask'][spec]
            spec, row = spec[on], row[on]
            pk = s['index'][row]
            if F['mode'] in ('dist', 'dist2'):
                d = np.sqrt((s['x'][row] - F['pos'][0][spec])**2 + (s['y'][row] - F['pos'][1][spec])**2
                            + (s['z'][row] - F['pos'][2][spec])**2)
                w = 1/d if F['mode'] == 'dist' else 1/(d*d)
            elif F['mode'] == 'sigma':
                w = F['weight'][spec]
            else:
                w = np.ones(len(spec))
            num, den = np.zeros(n_packets), np.zeros(n_packets)
            np.add.at(num, pk, F['ratio'][spec]*w)
            np.add.at(den, pk, w)
            cnt = np.bincount(pk, minlength=n_packets).astype(np.int32)
            seen = den > 0
            f = np.zeros(n_packets)
            f[seen] = num[seen]/den[seen]
            mult = f/f[seen].mean() if seen.any() else np.zeros(n_packets)
            self._mult = mult
            return dict(num=num, den=den, cnt=cnt, mult=mult, f_sum=float(f[seen].sum()),
                        n_seen=int(seen.sum()))

        def fit_radiance(self, pairs, dphi, sin_dphi, vrplanet, unit_cm, g_tables):
            s, F = self._src, self._fit
            spec, row = pairs.pairs
            frac = s['frac'][row]*self._mult[s['index'][row]]
            w = O.packet_weights(frac, s['vy'][row] + vrplanet, 1., 'radiance', g_tables)
            d = np.sqrt((s['x'][row] - F['pos'][0][spec])**2 + (s['y'][row] - F['pos'][1][spec])**2
                        + (s['z'][row] - F['pos'][2][spec])**2)
            np.add.at(self._fit_rad, spec, w/(np.pi*(d*sin_dphi)**2*unit_cm**2))

        def fit_rows(self, n_packets, compress=True):
            store, first, count, shift = self._src_rows
            r, idx = store.download(first, count)
            f = r[7].astype(np.float64)*self._mult[idx.astype(np.int64) - shift]
            keep = f > 0 if compress else np.ones(len(f), dtype=bool)
            rows = r[:, keep].copy()
            rows[7] = f[keep].astype(rows.dtype)
            lengths = np.bincount(idx[keep].astype(np.int64) - shift, minlength=n_packets)
            return OracleRowStore(self, rows, idx[keep].copy(), store.narrow), lengths

        def fit_download(self):
            return self._fit_rad.copy()
    return FitContext


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def spacecraft(n=40, seed=4, **columns):
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2*np.pi, n, endpoint=False)
    pos = np.stack([np.cos(th), 2*np.sin(th)*0.6 - 0.4, 2*np.sin(th)*0.8], 1)
    look = -pos + 0.6*rng.normal(size=pos.shape)
    look /= np.linalg.norm(look, axis=1)[:, None]
    return SpacecraftData(*pos.T, *look.T, **columns)


def inputs_():
    inputs = Input(INPUT)
    inputs.options.endtime = type(inputs.options.endtime)(6000., 's')
    return inputs


def unfitted_flow(ctx, cp=None, mode=None, seed=77, data_seed=3, masking=None):
    """Input.run, the unfitted LOSResult + determine_source_rate, then LOSResultFitted."""
    inputs = inputs_()
    with quiet():
        inputs.run(N, packs_per_it=SIZE, seed=seed, context=ctx, cp=cp)
    sc0 = spacecraft()
    probe = LOSResult(sc0, inputs, dphi=np.radians(3.0), context=ctx)
    with quiet():
        probe.simulate_data_from_inputs(sc0, cp=cp, reduce='host')
    rng = np.random.default_rng(data_seed)
    radiance = probe.radiance.values*rng.uniform(0.5, 1.5, len(sc0))
    sigma = 0.1*np.abs(radiance) + 0.01
    sc = spacecraft(radiance=radiance, sigma=sigma, alttan=np.linspace(0, 1, len(sc0)))
    los = LOSResult(sc, inputs, dphi=np.radians(3.0), context=ctx, label='unfit',
                    masking=masking)
    with quiet():
        los.simulate_data_from_inputs(sc, cp=cp, reduce='host')
    los.determine_source_rate(sc, use_weight=False)
    sc.add_model_result(los, 'unfit')
    fitted = LOSResultFitted(sc, 'unfit', dphi=np.radians(2.0), context=ctx)
    with quiet():
        fitted.determine_source_from_data(sc, use_weight=mode, cp=cp, reduce='host')
    return inputs, sc, los, fitted


def restated(los, sc, mode, fitted_dphi, runs):
    data = sc.data
    mask = data['mask_unfit'].values
    out = []
    for run in runs:
        X = run.X.copy()
        X = X.astype({c: np.float64 for c in X.columns if X[c].dtype == np.float32})
        smp = dict(x=X.x.values, y=X.y.values, z=X.z.values, vy=X.vy.values, frac=X.frac.values,
                   Index=X.Index.values)
        scd = {k: data[k].values for k in ('x', 'y', 'z', 'xbore', 'ybore', 'zbore')}
        vr = float(run.vrplanet)/los.unit_km
        g = los.g_tables(float(run.aplanet))
        used = O.los_iteration(smp, scd, los.dphi, 25., vr, g, los.unit_km*1e5,
                               n_index=int(run.npackets))[3]
        frac0 = run.X0['frac'].values if 'frac' in run.X0 else None
        out.append((X, refit_output(X, frac0, int(run.npackets), run.nsteps, used, data,
                                    los.radiance, mask, mode, fitted_dphi, los.unit_km*1e5, vr,
                                    g)))
    return out


# ---- make_mask / determine_source_rate -------------------------------------------------------
def _los(masking, **columns):
    sc = spacecraft(**columns)
    return LOSResult(sc, Input(INPUT), masking=masking), sc


def test_make_mask_types_and_combinations():
    rng = np.random.default_rng(1)
    rad = rng.uniform(0, 10, 40)
    rad[3] = np.nan
    sigma = rng.uniform(0.5, 2, 40)
    alt = np.linspace(-1, 1, 40)
    cols = dict(radiance=rad, sigma=sigma, alttan=alt)
    los, sc = _los(None, **cols)
    mask, lim = los.make_mask(sc.data)
    assert mask.all() and lim is None
    los, sc = _los('minalt0.25', **cols)
    assert np.array_equal(los.make_mask(sc.data)[0], alt >= 0.25)
    los, sc = _los(' MinSNR3 ', **cols)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(los.make_mask(sc.data)[0], rad/sigma > 3)
    los, sc = _los('middle80', **cols)
    lo, hi = np.nanpercentile(rad, [10, 90])
    with np.errstate(invalid='ignore'):
        assert np.array_equal(los.make_mask(sc.data)[0], (rad >= lo) & (rad <= hi))
    los, sc = _los('minalt0; minsnr2;siglimit3.5', **cols)
    mask, lim = los.make_mask(sc.data)
    with np.errstate(invalid='ignore'):
        assert np.array_equal(mask, (alt >= 0) & (rad/sigma > 2)) and lim == 3.5
    los, sc = _los('maxalt3', **cols)
    with pytest.raises(ValueError):
        los.make_mask(sc.data)


def _lsq(x, y, w):
    return np.linalg.lstsq((w*x)[:, None], w*y, rcond=None)[0][0]


@pytest.mark.parametrize('use_weight', [True, False])
def test_determine_source_rate_against_lstsq(use_weight):
    rng = np.random.default_rng(2)
    model = rng.uniform(1, 5, 40)
    sigma = rng.uniform(0.1, 1, 40)
    data = 2.5*model + rng.normal(0, 0.2, 40)
    data[5] += 40                                             # an outlier for siglimit
    for masking in (None, 'minalt0.2', 'minalt0.2;siglimit3'):
        los, sc = _los(masking, radiance=data, sigma=sigma, alttan=np.linspace(0, 1, 40))
        los.radiance[:] = model
        los.determine_source_rate(sc, use_weight=use_weight)
        m = np.linspace(0, 1, 40) >= 0.2 if masking else np.ones(40, dtype=bool)
        w = 1/sigma**2 if use_weight else np.ones(40)
        k = _lsq(model[m], data[m], w[m])
        if masking and 'siglimit' in masking:
            m = m & (np.abs((data - k*model)/sigma) < 3)
            assert not m[5]
            k = _lsq(model[m], data[m], w[m])
        np.testing.assert_allclose(float(los.sourcerate), k, rtol=1e-12)
        assert los.sourcerate.unit == '1e23/s'
        np.testing.assert_allclose(los.radiance.values, model*k, rtol=1e-12)
        assert np.array_equal(los.mask, m)
    los, sc = _los(None, radiance=data, sigma=sigma)          # all-zero model
    los.determine_source_rate(sc)
    assert float(los.sourcerate) == 0 and (los.radiance.values == 0).all() and los.mask.all()


# ---- the fitted flow on the stand-in -----------------------------------------------------------
@pytest.mark.parametrize('mode', [None, 'dist', 'dist2', 'sigma'])
def test_fitted_flow_matches_restatement(mode):
    inputs, sc, los, fitted = unfitted_flow(_stand_in()(), mode=mode)
    assert fitted.fitted and fitted.inputs.options.fitted and not inputs.options.fitted
    assert len(fitted.inputs._catalogue) == 2 and len(inputs._catalogue) == 2
    per = restated(los, sc, mode, np.radians(2.0), inputs._catalogue)
    radiance = np.zeros(len(sc.data))
    totalsource = 0.
    for it, fout, (X, r) in zip(fitted.iterations, fitted.inputs._catalogue, per):
        assert (r['cnt'] > 0).sum() > 20
        np.testing.assert_allclose(it['multiplier'], r['mult'], rtol=1e-12, atol=0)
        np.testing.assert_allclose(it['radiance'], r['radiance'], rtol=1e-10, atol=0)
        keep = r['keep']
        assert np.array_equal(fout.X.index.values, X.index.values[keep])
        assert np.array_equal(fout.X['frac'].values, r['frac_fit'][keep].astype(np.float32))
        np.testing.assert_allclose(fout.totalsource, r['totalsource'], rtol=1e-12)
        if 'frac' in fout.X0:
            np.testing.assert_allclose(fout.X0['frac'].values,
                                       r['frac0_fit'].astype(np.float32), rtol=1e-7)
        radiance += r['radiance']
        totalsource += r['totalsource']
    np.testing.assert_allclose(fitted.totalsource, totalsource, rtol=1e-12)
    scaled = radiance*(1e23/(totalsource/inputs.options.endtime.value))/1e3
    m = fitted.mask
    k = np.sum(scaled[m]*sc.data.radiance.values[m])/np.sum(scaled[m]**2)
    np.testing.assert_allclose(float(fitted.sourcerate), k, rtol=1e-10)
    np.testing.assert_allclose(fitted.radiance.values, scaled*k, rtol=1e-10, atol=0)
    assert fitted.unfit_outid == [1, 2] and len(fitted.outputfiles) == 2


def test_per_output_normalisation():
    """Each Output's multipliers average to 1 over its seen packets, whatever the other's."""
    inputs, sc, los, fitted = unfitted_flow(_stand_in()(), seed=78, data_seed=8)
    for it in fitted.iterations:
        seen = it['multiplier'] != 0
        np.testing.assert_allclose(it['multiplier'][seen].mean(), 1.0, rtol=1e-12)
    per = restated(los, sc, None, np.radians(2.0), inputs._catalogue)
    f_means = []
    for X, r in per:
        seen = r['den'] > 0
        f_means.append((r['num'][seen]/r['den'][seen]).mean())
    assert abs(f_means[0] - f_means[1]) > 1e-3*abs(f_means[0])       # they do differ


def test_output_without_pairs_gets_zero_and_warning():
    ctx = _stand_in()()
    inputs = inputs_()
    with quiet():
        inputs.run(N, packs_per_it=SIZE, seed=77, context=ctx)
    second = inputs._catalogue[1]
    second._spill()
    X = second.X.copy()
    X['x'] = X['x'] + np.float32(1000.)                      # nothing of it in any cone
    second.X = X
    sc0 = spacecraft()
    probe = LOSResult(sc0, inputs, dphi=np.radians(3.0), context=ctx)
    with quiet():
        probe.simulate_data_from_inputs(sc0)
    sc = spacecraft(radiance=2*probe.radiance.values, sigma=np.ones(len(sc0)))
    los = LOSResult(sc, inputs, dphi=np.radians(3.0), context=ctx, label='unfit')
    with quiet():
        los.simulate_data_from_inputs(sc)
    los.determine_source_rate(sc, use_weight=False)
    sc.add_model_result(los, 'unfit')
    fitted = LOSResultFitted(sc, 'unfit', dphi=np.radians(3.0), context=ctx)
    with quiet(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        fitted.determine_source_from_data(sc)
    assert any('multipliers are 0' in str(w.message) for w in caught)
    assert (fitted.iterations[1]['multiplier'] == 0).all()
    assert (fitted.iterations[0]['multiplier'] != 0).any()
    assert fitted.inputs._catalogue[1].totalsource == 0 and len(fitted.inputs._catalogue[1].X) == 0


def test_use_selected_and_bad_arguments_raise():
    inputs, sc, los, fitted = unfitted_flow(_stand_in()())
    with pytest.raises(NotImplementedError):
        fitted.determine_source_from_data(sc, use_selected=True)
    with pytest.raises(ValueError):
        fitted.determine_source_from_data(sc, use_weight='dist3')
    los.sourcerate = type(los.sourcerate)(0., '1e23/s')
    with pytest.raises(RuntimeError):
        fitted.determine_source_from_data(sc)


def test_spacecraft_data_columns_and_model_result():
    sc = SpacecraftData([2.], [0.], [0.], [-1.], [0.], [0.])
    assert list(sc.data.columns) == ['x', 'y', 'z', 'xbore', 'ybore', 'zbore']
    sc = spacecraft(5, radiance=np.arange(5.), sigma=np.ones(5), alttan=np.zeros(5))
    assert {'radiance', 'sigma', 'alttan'} <= set(sc.data.columns) and sc.model_result == {}

    class Result:
        radiance = pd.Series(np.arange(5.)*2)
        mask = np.array([True, False, True, True, False])
    sc.add_model_result(Result, 'lab')
    assert sc.model_result['lab'] is Result
    assert np.array_equal(sc.data['model_lab'].values, np.arange(5.)*2)
    assert np.array_equal(sc.data['mask_lab'].values, Result.mask)


def _worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from nexoclom_amd.distributed import ControlPlane
    cp = ControlPlane(world, rank, timeout=120)
    Ctx = _stand_in()
    inputs, sc, los, shared = unfitted_flow(Ctx(), cp=cp, mode='dist')
    assert len(inputs._catalogue) == 1 and len(shared.inputs._catalogue) == 1
    if rank == 0:
        _, _, _, alone = unfitted_flow(Ctx(), mode='dist')
        np.testing.assert_allclose(shared.radiance.values, alone.radiance.values, rtol=1e-12,
                                   atol=0)
        np.testing.assert_allclose(shared.totalsource, alone.totalsource, rtol=1e-14)
        np.testing.assert_allclose(float(shared.sourcerate), float(alone.sourcerate), rtol=1e-12)
        assert np.array_equal(shared.mask, alone.mask)
        open(os.path.join(tmpdir, 'ok'), 'w').write('ok')
    cp.barrier()
    cp.close()


def test_two_ranks_equal_one_rank(tmp_path):
    port = 29300 + os.getpid() % 150
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / 'ok').exists()


def test_fit_desc_layout_matches_header():
    d = hip_api.nxc_fit_desc
    # int64, 2 int32, 4 pointers
    assert C.sizeof(d) == 8 + 2*4 + 4*8
    assert d.weight_mode.offset == 8 and d.position.offset == 16 and d.ratio.offset == 24
    assert d.weight.offset == 32 and d.mask.offset == 40
    assert hip_api.NXC_ERR_OVERFLOW == -8
    text = open(os.path.join(ROOT, 'include', 'nexoclom_hip.h')).read()
    assert 'NXC_ERR_OVERFLOW = -8' in text
