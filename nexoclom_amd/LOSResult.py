"""LOSResult: modelled radiance along spacecraft lines of sight, accumulated on the GPU.

Drop-in for data_simulation/LOSResult.py:19-105,202-276 and compute_iteration.py:90-240 of the
reference on the path from catalogued Outputs to ``radiance`` / ``npackets`` per spectrum.  The
reference takes a ``MESSENGERdata`` object (external package, unavailable); anything with the same
duck type works here: ``.data`` (DataFrame with x, y, z, xbore, ybore, zbore in planet radii, model
frame), ``.species``, ``.query``, ``.set_frame()``, ``len()``.  ``SpacecraftData`` is a minimal one
for synthetic geometries.

Division of labour: everything per SPECTRUM that involves libm trigonometry -- the planet cut-off,
the geometric ladder of pre-selection spheres along the line of sight, the cone-angle threshold --
is set up here with NumPy (``los_geometry``, ``arccos_threshold``), so that the thresholds are the
reference's own doubles; every (sample, spectrum) pair test runs in the HIP kernel
(``nxc_los_accumulate``).

``make_mask`` and ``determine_source_rate`` restate LOSResult.py:171-200,278-308; the source-rate
fit is NOT called by ``simulate_data_from_inputs`` here (the reference calls it at the end): call it
explicitly before handing the result to ``LOSResultFitted`` (LOSResultFitted.py).
``make_source_map`` restates LOSResult.py:310-458 with make_source_map.py on the GPU (sourcemap.py).
The PostgreSQL caching of iterations is out of scope.

``profile=(v_lo_kms, v_hi_kms, nbins)`` (an extension; include/nexoclom_hip.h, "Line-of-sight
profile") adds the line profile of every spectrum -- its radiance per bin of the packets' velocity
along the boresight -- and the line's shift, width, skewness and effective packet number, from the
same pass over the samples.  Velocities are in the planet frame: the spacecraft's own velocity is not
subtracted.

``ages=(a_lo_s, a_hi_s, nbins)`` (an extension; include/nexoclom_hip.h, "Line-of-sight ages") files
every pair's contribution under the age of its row as well: ``age_profile`` is each spectrum's
response to a pulse of the source rate, and ``transient(history)`` gives the radiance of every
spectrum at its own epoch for a source whose rate changed with time (transient.py).
"""
import numpy as np
import pandas as pd

from .ModelImage import (ModelResult, cube_from_sums, parse_cube, pixel_moments_from_sums)
from .transient import (TransientRadiance, ages_from_sums, parse_ages, refuse_ages_of,
                        refuse_ages_with, spectrum_times)
from .units import Quantity

POSITION = ('x', 'y', 'z')
BORESIGHT = ('xbore', 'ybore', 'zbore')


class SpacecraftData:
    """Minimal stand-in for MESSENGERuvvs.MESSENGERdata: positions and boresights per spectrum,
    optionally the observed ``radiance`` [kR], its ``sigma``, the tangent altitude ``alttan`` and
    the ``time`` [s] at which each spectrum was taken, on the clock of a source history
    (data columns of the same names), and the model results fitted to it (``model_result``)."""

    def __init__(self, x, y, z, xbore, ybore, zbore, species='Na', query='synthetic', *,
                 radiance=None, sigma=None, alttan=None, time=None):
        columns = dict(zip(POSITION + BORESIGHT, (x, y, z, xbore, ybore, zbore)))
        for name, values in (('radiance', radiance), ('sigma', sigma), ('alttan', alttan),
                             ('time', time)):
            if values is not None:
                columns[name] = values
        self.data = pd.DataFrame(columns, dtype=float)
        self.species, self.query, self.frame = species, query, 'Model'
        self.model_result = {}

    def add_model_result(self, result, label):
        """Keep ``result`` under ``label`` with its radiance and mask as data columns
        model_<label>, mask_<label> (what LOSResultFitted reads, LOSResultFitted.py:21,140).  A
        result without a mask (determine_source_rate not called) masks nothing."""
        self.model_result[label] = result
        self.data['model_' + label] = np.asarray(result.radiance, dtype=float)
        mask = getattr(result, 'mask', None)
        self.data['mask_' + label] = (np.ones(len(self.data), dtype=bool) if mask is None
                                      else np.asarray(mask, dtype=bool))

    def set_frame(self, frame):
        self.frame = frame

    def __len__(self):
        return len(self.data)


def arccos_threshold(dphi):
    """Smallest double c with arccos(c) <= dphi: the reference's ``ang <= dphi`` with
    ``ang = np.arccos(cosang)`` (compute_iteration.py:181-185) is then exactly ``cosang >= c`` for
    this NumPy's (monotone) arccos, so the kernel needs no arccos."""
    below, reached = 0.0, 1.0                # arccos(below) > dphi >= arccos(reached)
    assert np.arccos(below) > dphi >= np.arccos(reached)
    while True:
        middle = 0.5*(below + reached)
        if middle in (below, reached):
            return reached
        if np.arccos(middle) <= dphi:
            reached = middle
        else:
            below = middle


def ladder_to(limit, first, ratio):
    """t_0 = first, t_{k+1} = t_k + t_k * ratio, up to and including the first rung >= limit
    (compute_iteration.py:164-167: sample points spaced in proportion to their distance)."""
    rungs = [first]
    while rungs[-1] < limit:
        rungs.append(rungs[-1] + rungs[-1] * ratio)
    return rungs


def los_geometry(data, outeredge, dphi):
    """Per-spectrum set-up of compute_iteration.py:101-115,157-167.  Returns
    (dist_from_plan, ladder lengths, longest ladder): the distance at which a line of sight that
    hits the planet is cut (1e30 when it misses), and the ladder out to where the line leaves the
    sphere r = outeredge -- all spectra share one geometric ladder, they differ in its length."""
    at = data[list(POSITION)].values.astype(float)
    look = data[list(BORESIGHT)].values.astype(float)
    x, y, z = at.T
    xb, yb, zb = look.T
    dist_from_plan = np.sqrt(x**2 + y**2 + z**2)
    with np.errstate(invalid='ignore'):
        off_centre = np.arccos((-x*xb - y*yb - z*zb) / dist_from_plan)
        planet_size = np.arcsin(1. / dist_from_plan)
    dist_from_plan = np.where(off_centre > planet_size, 1e30, dist_from_plan)
    step = np.sin(dphi)
    far = np.empty(len(at))
    for k, (x_sc, bore) in enumerate(zip(at, look)):
        # far root of |x_sc + t bore| = outeredge
        b = 2*np.sum(x_sc*bore)
        c = np.linalg.norm(x_sc)**2 - outeredge**2
        with np.errstate(invalid='ignore'):
            far[k] = (-b + np.sqrt(b**2 - 4*1*c))/2
    # every spectrum climbs the same rungs and stops at its own `far`: one ladder to the largest,
    # a spectrum's length = the rungs below its limit plus the one that reaches it (a line that
    # never meets the sphere has a NaN root and, like the reference's loop, just the first rung)
    reach = np.nanmax(far) if np.isfinite(far).any() else step
    ladder = np.array(ladder_to(reach, step, step))
    lengths = np.where(np.isnan(far), 1, np.searchsorted(ladder, far, side='left') + 1)
    lengths = np.minimum(lengths, len(ladder)).astype(np.int64)
    return dist_from_plan, lengths, ladder[:lengths.max()]


def parse_profile(profile, n_spectra):
    """``(v_lo_kms, v_hi_kms, nbins)`` of a ``profile=`` argument, by parse_cube's rules;
    ValueError also when ``n_spectra`` spectra would have more records than the device addresses
    (S (nbins + 2) < 2^31)."""
    try:
        v_lo, v_hi, nbins = parse_cube(profile)
    except ValueError as err:
        raise ValueError(str(err).replace('cube=', 'profile=')) from None
    if n_spectra*(nbins + 2) >= 2**31:
        raise ValueError('profile=: len(scdata)*(nbins + 2) must stay below 2^31')
    return v_lo, v_hi, nbins


def parse_los_ages(ages, n_spectra):
    """``(a_lo_s, a_hi_s, nbins)`` of an ``ages=`` argument, by parse_ages's rules; ValueError also
    when ``n_spectra`` spectra would have more records than the device addresses
    (S (nbins + 2) < 2^31)."""
    a_lo, a_hi, nbins = parse_ages(ages)
    if n_spectra*(nbins + 2) >= 2**31:
        raise ValueError('ages=: len(scdata)*(nbins + 2) must stay below 2^31')
    return a_lo, a_hi, nbins


class LOSResult(ModelResult):
    _ages = None              # (a_lo_s, a_hi_s, nbins): the passes also fill age_sums
    _times = None             # the spectra's ``time`` column as simulate_data_from_inputs saw it

    def __init__(self, scdata, inputs, params=None, dphi=np.radians(1.), *, device=0,
                 context=None, profile=None, ages=None, **kwargs):
        scdata.set_frame('Model')
        self._profile = None if profile is None else parse_profile(profile, len(scdata.data))
        if ages is not None:
            refuse_ages_with(profile=profile)
            self._ages = parse_los_ages(ages, len(scdata.data))
            refuse_ages_of(inputs)
        super().__init__(inputs, {'quantity': 'radiance'} if params is None else params)
        if self.quantity != 'radiance':
            assert False, 'Other quantities not set up.'      # compute_iteration.py:213
        self.type = 'LineOfSight'
        self.species, self.query = scdata.species, scdata.query
        self.dphi = float(dphi)
        self._oedge = np.min([self.inputs.options.outeredge*2, 100])
        self.fitted = self.inputs.options.fitted
        rows = scdata.data.index
        self.radiance = pd.Series(np.zeros(len(rows)), index=rows)
        self.npackets_los = pd.Series(np.zeros(len(rows), dtype=np.int64), index=rows)
        self.included = None
        self.mask = None
        self.goodness_of_fit = None
        self.masking = kwargs.get('masking', None)                    # LOSResult.py:101
        self.label = kwargs.get('label', 'LOSResult')
        self._ctx, self._device = context, device
        self.iterations = []
        self._geometry = None

    def compute_iteration(self, output, scdata, used_cap=0, pairs=None, profile=False, ages=False):
        """One catalogued Output against all spectra (compute_iteration.py:90-240).  ``pairs``: a
        device pair list (hip_api.PairList) that receives the pairs with weight > 0.  ``profile``:
        the pass also adds to the context's enabled line-of-sight profile; ``ages``: to its enabled
        line-of-sight ages."""
        from .Output import Output
        if not isinstance(output, Output):       # a file; a catalogued Output is used as stored:
            output = Output.restore(output)      # the binding widens just the columns it sends
        spectra = scdata.data
        if self._geometry is None or self._geometry[0] is not spectra:
            # the same for every Output of a run (compute_iteration.py recomputes it per file)
            self._geometry = (spectra, los_geometry(spectra, self.inputs.options.outeredge,
                                                    self.dphi))
        cut, lengths, ladder = self._geometry[1]
        sc = np.vstack([spectra[list(POSITION + BORESIGHT)].values.T.astype(float), cut,
                        lengths.astype(float)])
        setup = (self.dphi, np.sin(self.dphi), np.sin(self.dphi*2), arccos_threshold(self.dphi),
                 float(output.vrplanet)/self.unit_km, self.unit_km*1e5,
                 self.g_tables(float(output.aplanet)), ladder, sc)
        extra = {} if pairs is None else {'pairs': pairs}
        velocity = ()
        if profile:                            # the profile's entries, which read vx and vz too
            extra['profile'] = True
            velocity = ('vx', 'vz')
        if ages:                               # the ages' entries, which read the rows' time too
            extra['ages'] = True
            velocity = ('time',)
        view = output.resident_rows(self.context())
        if view is not None:
            # the Output's rows are still in HBM: no host round trip
            store, first, count, packet0 = view
            res = self.context().los_accumulate(*setup, n_index=int(output.npackets),
                                                used_cap=used_cap,
                                                rows=(store, first, count, packet0), **extra)
        else:
            samples = output.X
            index = Output.packet_index(samples)
            n_index = int(len(output.X0)) if len(output.X0) else int(index.max()) + 1
            res = self.context().los_accumulate(
                *setup, *(samples[c].values for c in ('x', 'y', 'z', 'vy', 'frac')),
                index=index, n_index=n_index, used_cap=used_cap,
                **{c: samples[c].values for c in velocity}, **extra)
        assert self.context().counters()['nonfinite'] == 0, 'Non-finite weights'
        res['totalsource'] = output.totalsource
        for key in ('radiance', 'npackets'):
            res[key] = pd.Series(res[key], index=spectra.index)
        return res

    def simulate_data_from_inputs(self, scdata, distribute=None, *, cp=None, reduce='rccl'):
        """LOSResult.py:202-276: sum the iterations of every catalogued Output, then scale to kR
        for a source rate of 1e23 atoms/s.  ``cp``: the control plane of a shared run
        (``Input.run(..., cp=cp)``): this rank's catalogue is its share of the Outputs; the
        per-spectrum radiances and packet counts and the source totals are summed over the ranks
        where the reference sums over the files (LOSResult.py:264-266) -- S + S + 2 doubles, one
        all-reduce.  ``iterations`` (with their `included` flags) stay those of the local Outputs."""
        if distribute in (True, 'delay', 'delayed'):
            assert False, "Don't do this"
        if self._profile is not None and cp is not None:
            raise NotImplementedError('profile= does not support cp=: there is no all-reduce of the '
                                      'profile yet')
        if self._ages is not None:
            refuse_ages_with(cp=cp)
        self.outid, self.outputfiles, self.npackets, self.totalsource = self.inputs.search()
        print(f'LOSResult: {len(self.outid)} output files found.')
        shared = cp is not None and cp.world > 1
        if self.npackets == 0 and not shared:
            raise RuntimeError('No packets found for these Inputs.')
        if self._profile is not None:
            # one profile for the whole run: every Output's pass adds to it on the device
            v_lo, v_hi, nbins = self._profile
            self.context().los_profile_enable(len(scdata.data), nbins, v_lo/self.unit_km,
                                              v_hi/self.unit_km)
        if self._ages is not None:
            # one block for the whole run, like the profile's
            a_lo, a_hi, nbins = self._ages
            self.context().los_ages_enable(len(scdata.data), nbins,
                                           float(self.inputs.options.endtime.value), a_lo, a_hi)
            self._times = (np.array(scdata.data['time'], dtype=float) if 'time' in scdata.data
                           else None)
        modes = {key: True for key, on in (('profile', self._profile), ('ages', self._ages))
                 if on is not None}
        self.iterations = [self.compute_iteration(run, scdata, **modes)
                           for run in self.inputs._catalogue]
        if self._ages is not None:
            self.age_sums = self.context().los_ages_download()
            self.context().los_ages_enable(len(scdata.data), 0)
        if self._profile is not None:
            self.profile_sums, self.moment_sums = self.context().los_profile_download()
            self.context().los_profile_enable(len(scdata.data), 0)
        for it in self.iterations:
            assert len(it['radiance']) == len(scdata.data)
            self.radiance += it['radiance']
            self.npackets_los += it['npackets']
        if shared:
            from .distributed import allreduce_small, guarded
            S = len(scdata.data)
            with guarded(cp, self.context()):
                both = allreduce_small(np.concatenate([
                    np.asarray(self.radiance, dtype=float), np.asarray(self.npackets_los, dtype=float),
                    [float(self.totalsource), float(self.npackets)]]), cp, self.context(), reduce)
            self.radiance[:] = both[:S]
            self.npackets_los[:] = np.rint(both[S:2*S]).astype(self.npackets_los.dtype)
            self.totalsource, self.npackets = float(both[2*S]), int(round(both[2*S + 1]))
            if self.npackets == 0:
                raise RuntimeError('No packets found for these Inputs.')
        per_second = self.totalsource / self.inputs.options.endtime.value
        self.atoms_per_packet = 1e23 / per_second
        if self._profile is not None:
            self._publish_profile(scdata.data.index)
        if self._ages is not None:
            self._publish_ages(scdata.data.index)
        self.radiance *= self.atoms_per_packet/1e3      # kR

    def _publish_profile(self, rows):
        """The profile's attributes from ``profile_sums`` and ``moment_sums``: the quotients are
        those of the pixel moments with S0 the unscaled radiance, the bins get the radiance's
        scaling; indexed like ``radiance``."""
        got = dict(pixel_moments_from_sums(np.asarray(self.radiance, dtype=float), self.moment_sums,
                                           self.unit_km))
        for name, value in cube_from_sums(self.profile_sums, self.atoms_per_packet/1e3,
                                          *self._profile[:2]).items():
            got[name.replace('cube', 'profile')] = value
        for name, value in got.items():
            if name not in ('velocity_edges', 'velocity_axis'):
                value = (pd.Series(value, index=rows) if value.ndim == 1
                         else pd.DataFrame(value, index=rows))
            setattr(self, name, value)

    def _publish_ages(self, rows):
        """The ages' attributes from ``age_sums`` (transient.ages_from_sums with the radiance's
        scaling): ``age_profile`` (S, nbins), ``age_below``, ``age_above`` and
        ``age_effective_packets``, indexed like ``radiance``; ``age_edges`` and ``age_axis`` [s]."""
        for name, value in ages_from_sums(self.age_sums, self.atoms_per_packet/1e3,
                                          *self._ages[:2]).items():
            if name not in ('age_edges', 'age_axis'):
                value = (pd.Series(value, index=rows) if value.ndim == 1
                         else pd.DataFrame(value, index=rows))
            setattr(self, name.replace('age_cube', 'age_profile'), value)

    def transient(self, history, times=None):
        """The radiance of every spectrum at its own epoch for a source whose rate relative to the
        nominal one was ``history = (t_nodes_s, rate_nodes)`` (transient.response_matrix): a
        TransientRadiance with times, kernel (nbins + 2, S), radiance [kR] and effective_packets.
        ``times``: (S,) seconds on the history's clock, or one number for all spectra; by default
        the ``time`` column the spacecraft data had in ``simulate_data_from_inputs``."""
        if self._ages is None:
            raise ValueError('transient() needs an object built with ages=(a_lo_s, a_hi_s, nbins)')
        if not hasattr(self, 'age_sums'):
            raise ValueError('transient() needs simulate_data_from_inputs first')
        times = spectrum_times(times, self._times, self.age_sums.shape[0])
        return TransientRadiance(times, self.age_edges, history, self.age_sums,
                                 self.atoms_per_packet/1e3, self.radiance.index)

    def transient_design(self, t_nodes, times=None):
        """(S, J) matrix A with ``A @ rates == transient((t_nodes, rates)).radiance`` up to
        rounding: column j is ``transient`` of the history with rate 1 at node j and 0 at the
        others.  What a non-negative least-squares fit of a source history to an observed scan
        needs; the fit itself is the caller's."""
        nodes = np.atleast_1d(np.asarray(t_nodes, dtype=float))
        columns = [np.asarray(self.transient((nodes, np.eye(len(nodes))[j]), times).radiance)
                   for j in range(len(nodes))]
        return np.stack(columns, axis=1)

    def make_mask(self, data):
        """(mask, sigma limit) of the ``masking`` keyword (LOSResult.py:171-200): ';'-separated
        'middle<p>', 'minalt<a>', 'minsnr<s>', 'siglimit<n>'.

        Deviation: 'middle<p>' keeps the spectra whose radiance lies within the central p per cent
        of the ``radiance`` column, np.nanpercentile at (100 - p)/2 and 100 - (100 - p)/2; the
        reference hands the whole DataFrame to astropy's PercentileInterval."""
        radiance = np.asarray(data['radiance'], dtype=float)
        mask = np.ones(len(radiance), dtype=bool)
        sigmalimit = None
        if self.masking is not None:
            for masktype in self.masking.split(';'):
                masktype = masktype.strip().lower()
                if masktype.startswith('middle'):
                    low = (100. - float(masktype[6:]))/2
                    lim = np.nanpercentile(radiance, [low, 100. - low])
                    mask = mask & (radiance >= lim[0]) & (radiance <= lim[1])
                elif masktype.startswith('minalt'):
                    mask = mask & (np.asarray(data['alttan'], dtype=float) >= float(masktype[6:]))
                elif masktype.startswith('minsnr'):
                    snr = radiance/np.asarray(data['sigma'], dtype=float)
                    mask = mask & (snr > float(masktype[6:]))
                elif masktype.startswith('siglimit'):
                    sigmalimit = float(masktype[8:])
                else:
                    raise ValueError(f'masking = {masktype} not defined.')
        return mask, sigmalimit

    def determine_source_rate(self, scdata, use_weight=True):
        """LOSResult.py:278-308: scale the model radiance to the data.  astropy's LinearLSQFitter
        on a Multiply model is the weighted least-squares factor sum(w^2 x y) / sum(w^2 x^2) with
        w = 1/sigma^2 (use_weight) or 1; with 'siglimit<n>' the spectra more than n sigma off the
        first fit are dropped and the factor fitted again (the weights then follow the narrowed
        mask; the reference passes the first mask's).  Sets radiance, sourcerate, mask."""
        data = scdata.data
        mask, sigmalimit = self.make_mask(data)
        model = np.asarray(self.radiance, dtype=float)
        observed = np.asarray(data['radiance'], dtype=float)
        sigma = np.asarray(data['sigma'], dtype=float) if 'sigma' in data else None

        def factor(m):
            w = 1./sigma[m]**2 if use_weight else np.ones(int(m.sum()))
            x, y = model[m], observed[m]
            return np.sum(w*w*x*y)/np.sum(w*w*x*x)

        if not np.all(model == 0):
            best = factor(mask)
            if sigmalimit is not None:
                diff = np.abs((observed - best*model)/sigma)
                mask = mask & (diff < sigmalimit)
                best = factor(mask)
            self.radiance *= best
            self.sourcerate = Quantity(float(best), '1e23/s')
        else:
            self.sourcerate = Quantity(0., '1e23/s')
        self.goodness_of_fit = None
        self.mask = mask

    def make_source_map(self, grid_params=None, normalize=True, do_source=True, do_available=True,
                        *, cp=None, reduce='rccl'):
        """LOSResult.py:310-458 with make_source_map.py:11-174 per Output (see sourcemap.py):
        returns (sourcemap, availablemap), each a SourceMap or None.  Works on the Outputs
        catalogued under ``self.inputs`` -- for a LOSResultFitted the fitted ones, whose X0.frac
        carries the multipliers.  ``normalize`` uses ``self.sourcerate`` (determine_source_rate).
        ``cp``: the control plane of a shared run: one small all-reduce agrees on the global vmax
        (each rank fills its slot of a world-length vector), each rank sums its own Outputs on
        that axis, one all-reduce sums the combined arrays.  The reference's ``distribute`` is
        not ported."""
        from . import sourcemap as SM
        todo = [t for t, on in (('source', do_source), ('available', do_available)) if on]
        grid = SM.SourceMapGrid(grid_params, self.unit_km)
        runs = []
        for run in self.inputs._catalogue:
            cols = SM.x0_columns(run)
            if cols is not None:
                runs.append((cols, SM.output_vmax(cols, grid.r_km)))
        shared = cp is not None and cp.world > 1
        ctx = self.context()
        vmax = max([v for _, v in runs], default=-np.inf)
        if shared:
            from .distributed import allreduce_small, guarded
            slots = np.zeros(cp.world)
            slots[cp.rank] = vmax if runs else np.nan
            with guarded(cp, ctx):
                slots = allreduce_small(slots, cp, ctx, reduce)
            vmax = float(np.nanmax(slots)) if np.isfinite(slots).any() else -np.inf
        if not np.isfinite(vmax):
            raise RuntimeError('make_source_map: no Output has an X0 packet')
        # the Outputs of this rank, sorted by cell once for both passes
        sorted_runs = []
        for cols, v in runs:
            order, cell_start = grid.bucket(cols['latitude'], cols['longitude'])
            sorted_runs.append(({c: cols[c][order] for c in SM.X0_COLUMNS}, cell_start, v))
        results = []
        for todo_ in todo:
            results.append(self._source_map_pass(grid, sorted_runs, vmax, todo_ == 'available',
                                                 normalize, ctx, cp if shared else None, reduce))
        out = dict(zip(todo, results))
        return out.get('source'), out.get('available')

    def _source_map_pass(self, grid, sorted_runs, vmax, available, normalize, ctx, cp, reduce):
        from . import sourcemap as SM
        nvel, nalt, naz = grid.nvel, grid.nalt, grid.naz
        top = SM.centres(SM.speed_edges(vmax, nvel)).max()
        ctx.source_map_set(grid)
        pieces, vmaxes = [], []
        for cols, cell_start, v in sorted_runs:
            factor = 2.0 if SM.centres(SM.speed_edges(v, nvel)).max() == top else 1.0
            pieces.append(ctx.source_map_accumulate(
                cols['latitude'], cols['longitude'], cols['v'], cols['altitude'], cols['azimuth'],
                cols['frac'], cell_start, SM.speed_edges(v, nvel), available, factor))
            vmaxes.append(v)
        acc, hist2d = ctx.source_map_download()
        if pieces:
            small, _ = SM.combine_small(pieces, vmaxes, nvel, vmax)
        else:
            small = dict(speed_dist=np.zeros(nvel), broadcast=np.zeros(nvel),
                         altitude_dist=np.zeros(nalt), azimuth_dist=np.zeros(naz))
        small['speed'] = SM.centres(SM.speed_edges(vmax, nvel))
        if cp is not None:
            from .distributed import allreduce_small, guarded
            flat = np.concatenate([acc.ravel(), hist2d, small['speed_dist'], small['broadcast'],
                                   small['altitude_dist'], small['azimuth_dist']])
            with guarded(cp, ctx):
                flat = allreduce_small(flat, cp, ctx, reduce)
            k = acc.size
            acc = flat[:k].reshape(acc.shape)
            hist2d = flat[k:k + hist2d.size]
            k += hist2d.size
            for key, n in (('speed_dist', nvel), ('broadcast', nvel), ('altitude_dist', nalt),
                           ('azimuth_dist', naz)):
                small[key] = flat[k:k + n].copy()
                k += n
        shape = (grid.nlon, grid.nlat)
        nb = nvel + nalt + naz
        d = dict(longitude=grid.lon.copy(), latitude=grid.lat.copy(), speed=small['speed'],
                 altitude=grid.altitude.copy(), azimuth=grid.azimuth.copy(),
                 speed_dist=small['speed_dist'], altitude_dist=small['altitude_dist'],
                 azimuth_dist=small['azimuth_dist'])
        d['speed_dist_map'] = (acc[:, :nvel] + small['broadcast']).reshape(shape + (nvel,))
        d['altitude_dist_map'] = acc[:, nvel:nvel + nalt].reshape(shape + (nalt,))
        d['azimuth_dist_map'] = acc[:, nvel + nalt:nb].reshape(shape + (naz,))
        d['n_total'] = acc[:, nb].reshape(shape)
        d['n_included'] = acc[:, nb + 1].reshape(shape)
        d['abundance_uncor'] = (acc[:, nb + 2] if grid.smear_abundance else hist2d).reshape(shape)
        d = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}
        SM.finish(d, normalize, getattr(self, 'sourcerate', 0.), self.unit_km)
        return SM.SourceMap(d, normalized=normalize)
