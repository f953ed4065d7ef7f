"""LOSResultFitted: packet weights refitted to observed radiances, on the GPU.

Drop-in for data_simulation/LOSResultFitted.py:18-255 of the reference:
``LOSResultFitted(scdata, label_for_fitted, params=None, dphi=radians(1))`` then
``determine_source_from_data(scdata, use_weight=None | 'dist' | 'dist2' | 'sigma')``.  ``scdata``
holds the observed ``radiance`` (and ``sigma`` for 'sigma' weights) and, under
``label_for_fitted``, an unfitted LOSResult whose ``simulate_data_from_inputs`` and
``determine_source_rate`` have run (``scdata.add_model_result(result, label)``).

Per catalogued Output of the unfitted result:

1. its unfitted line-of-sight pass runs again with the UNFITTED result's dphi and set-up, and keeps
   the (spectrum, row) pairs with weight > 0 -- the reference's ``used`` set -- in a device pair
   list (capacity: the Output's sum of npackets over the spectra, which bounds it);
2. ratio_j = data_j / unfitted model_j (NaN -> 0); per packet i, over the pairs whose spectrum is
   in the mask: num_i = sum ratio_j w, den_i = sum w (w = 1, 1/d, 1/d^2 or 1/sigma_j*2, the
   reference's quirk kept), f_i = num_i / den_i where den_i > 0, else 0; mult_i = f_i / mean(f over
   den > 0) per Output (k_fit_packets, k_fit_norm);
3. every row's frac and X0's frac are multiplied by mult_i in fp64 (k_fit_rows for rows in HBM, a
   gather on the host for restored / variable-step Outputs), save()'s frac > 0 filter and
   down-cast follow; totalsource = X0.frac.sum() * nsteps (LOSResultFitted.py:189, as written);
4. the fitted radiance of every spectrum is summed over the same pairs with the new weights and
   this result's dphi in Apix (k_fit_radiance, no shadow factor).

The fitted Outputs are catalogued under ``self.inputs`` (a copy of the unfitted inputs with
options.fitted = True), so ``self.inputs.produce_image``, ``ModelImage`` and ``ModelDensity`` work
on them unchanged.  Then, as LOSResultFitted.py:239-253: radiance *= atoms_per_packet/1e3 and
``determine_source_rate(use_weight=False)``.

Deviations: an Output whose packets no masked pair sees gets multiplier 0 (with a warning) where
the reference would fill it with NaN; there is no database, so every call computes and
``overwrite`` only empties the fitted catalogue; ``use_selected`` (one random stored row per packet,
drawn in Python set order) is not restated and raises NotImplementedError.
"""
import copy
import os
import warnings

import numpy as np
import pandas as pd

from .LOSResult import LOSResult, POSITION

WEIGHTS = (None, 'dist', 'dist2', 'sigma')


def fitted_inputs(inputs):
    """A copy of ``inputs`` with options.fitted = True and a catalogue of its own (fitted Outputs
    are saved under <savepath>/fitted when the unfitted ones have a savepath)."""
    new = copy.copy(inputs)
    new.options = copy.copy(inputs.options)
    new.options.fitted = True
    new._catalogue, new._fused = [], []
    if getattr(inputs, 'savepath', None):
        new.savepath = os.path.join(inputs.savepath, 'fitted')
    return new


class LOSResultFitted(LOSResult):
    def __init__(self, scdata, label_for_fitted, params=None, dphi=np.radians(1.), **kwargs):
        if kwargs.get('profile') is not None:
            raise NotImplementedError('profile= is not supported by LOSResultFitted: the profile '
                                      'carries no fitted weights')
        if kwargs.get('ages') is not None:
            raise NotImplementedError('ages= is not supported by LOSResultFitted: the age sums '
                                      'carry no fitted weights')
        unfit = scdata.model_result[label_for_fitted]
        inputs = fitted_inputs(unfit.inputs)
        if 'context' not in kwargs and getattr(unfit, '_ctx', None) is not None:
            kwargs['context'] = unfit._ctx
        super().__init__(scdata, inputs, params=params, dphi=dphi, **kwargs)
        self.unfitted_label = label_for_fitted
        self.unfit_outid = None
        self.unfit_outputfiles = None

    def determine_source_from_data(self, scdata, overwrite=False, use_selected=False,
                                   use_weight=None, *, cp=None, reduce='rccl'):
        """LOSResultFitted.py:66-255.  ``cp``: the control plane of a shared run: each rank fits
        its own Outputs (the normalisation is per Output), the ratios use the all-reduced unfitted
        radiance, and the fitted radiance and totalsource are summed over the ranks with one
        all-reduce before the scaling."""
        if use_selected:
            raise NotImplementedError('use_selected draws from output.randgen in Python set order; '
                                      'it is not restated')
        if use_weight not in WEIGHTS:
            raise ValueError(f'use_weight must be one of {WEIGHTS}')
        unfit = scdata.model_result[self.unfitted_label]
        data = scdata.data
        if float(unfit.sourcerate) == 0:
            raise RuntimeError('The unfitted result has source rate 0: every data/model ratio '
                               'would be inf or NaN (call determine_source_rate first).')
        if overwrite:
            self.inputs.delete_files()
        runs = list(unfit.inputs._catalogue)
        if len(unfit.iterations) != len(runs):
            raise RuntimeError('The unfitted result has no iteration for every catalogued Output '
                               '(call simulate_data_from_inputs first).')
        print(f'LOSResultFitted: {len(runs)} unfitted files.')
        S = len(data)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = (data['radiance'] / unfit.radiance).fillna(0).values.astype(float)
        mask = np.asarray(data[f'mask_{self.unfitted_label}'], dtype=bool)
        weight = None
        if use_weight == 'sigma':
            weight = np.ones(S)/data['sigma'].values*2           # LOSResultFitted.py:163-165
        position = data[list(POSITION)].values.T.astype(float)
        ctx = self.context()
        cap = max([1] + [int(np.sum(it['npackets'])) for it in unfit.iterations])
        pairs = ctx.pairs_create(cap)
        try:
            fits = [self._fit_output(run, unfit, scdata, ctx, pairs, position, ratio, mask,
                                     use_weight, weight) for run in runs]
        finally:
            pairs.free()
        self.iterations = fits
        radiance = np.zeros(S)
        totalsource = 0.
        for it in fits:
            radiance += it['radiance']
            totalsource += it['totalsource']
        shared = cp is not None and cp.world > 1
        if shared:
            from .distributed import allreduce_small, guarded
            with guarded(cp, ctx):
                both = allreduce_small(np.concatenate([radiance, [totalsource]]), cp, ctx, reduce)
            radiance, totalsource = both[:S].copy(), float(both[S])
        self.radiance = pd.Series(radiance, index=data.index)
        self.totalsource = totalsource
        self.outid, self.outputfiles, self.npackets, _ = self.inputs.search()
        self.unfit_outid = [run.idnum for run in runs]
        self.unfit_outputfiles = [run.filename or run for run in runs]
        model_rate = self.totalsource/self.inputs.options.endtime.value   # :248-253
        self.atoms_per_packet = 1e23/model_rate
        self.radiance *= self.atoms_per_packet/1e3
        self.determine_source_rate(scdata, use_weight=False)
        print(self.totalsource, self.atoms_per_packet)

    def _fit_output(self, run, unfit, scdata, ctx, pairs, position, ratio, mask, use_weight,
                    weight):
        from .Output import Output
        # 1. the unfitted pass's used pairs, on the device
        unfit.compute_iteration(run, scdata, pairs=pairs)
        n_pairs = pairs.count
        view = run.resident_rows(ctx) if isinstance(run, Output) else None
        n_packets = int(run.npackets)
        ctx.fit_set(position, ratio, mask, use_weight, weight)
        if view is not None:
            ctx.fit_source(rows=view)
        else:
            X = run.X
            index = Output.packet_index(X)
            ctx.fit_source(*(X[c].values for c in ('x', 'y', 'z', 'vy', 'frac')), index=index)
        # 2. the multipliers
        res = ctx.fit_packets(pairs, n_packets)
        mult = res['mult']
        if res['n_seen'] == 0:
            warnings.warn(f'LOSResultFitted: no masked line of sight sees a packet of Output '
                          f'{run.idnum}: its multipliers are 0 (the reference would make them NaN)')
        # 4. the fitted radiance of every spectrum
        ctx.fit_radiance(pairs, self.dphi, np.sin(self.dphi), float(run.vrplanet)/self.unit_km,
                         self.unit_km*1e5, self.g_tables(float(run.aplanet)))
        radiance = ctx.fit_download()
        # 3. the fitted Output
        fitted = self._fitted_output(run, ctx, view, mult)
        fitted.save()
        return {'radiance': radiance, 'npackets': float(np.sum(fitted.X0['frac'].values))
                if 'frac' in fitted.X0 else float(np.sum(mult)),
                'totalsource': fitted.totalsource, 'outputfile': fitted.filename or fitted,
                'out_idnum': fitted.idnum, 'unfit_outputfile': run.filename or run,
                'unfit_outid': run.idnum, 'included': True, 'multiplier': mult,
                'n_pairs': n_pairs, 'n_seen': res['n_seen']}

    def _fitted_output(self, run, ctx, view, mult):
        """A new Output: ``run`` with frac' = frac * mult[packet] in its rows and X0."""
        from .Output import Output
        fitted = copy.copy(run)
        fitted.inputs = self.inputs
        fitted.filename, fitted.idnum = None, None
        fitted.__dict__.pop('_store', None)
        fitted.__dict__.pop('_X', None)
        nsteps = run.nsteps if run.nsteps else 1
        X0 = run.X0
        if len(X0) and 'frac' in X0:
            frac0 = X0['frac'].values
            new0 = frac0.astype(np.float64)*mult
            X0 = X0.copy()
            X0['frac'] = new0.astype(frac0.dtype)
            fitted.totalsource = float(np.sum(new0))*nsteps
        else:
            # the device sampler's X0 was not kept: every packet started with frac = 1
            fitted.totalsource = float(np.sum(mult))*nsteps
        fitted.X0 = X0
        if view is not None:
            store, lengths = ctx.fit_rows(len(mult), compress=getattr(run, 'compress', True))
            fitted._attach_rows(store, 0, lengths, view[3])
        else:
            X = run.X
            if len(X) and 'frac' in X:
                index = Output.packet_index(X)
                frac = X['frac'].values
                new = frac.astype(np.float64)*mult[index]
                X = X.copy()
                X['frac'] = new.astype(frac.dtype)
                if getattr(run, 'compress', True):
                    X = X[new > 0]
            fitted._X = X
        return fitted
