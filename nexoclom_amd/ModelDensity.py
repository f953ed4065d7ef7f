"""ModelDensity: number density at arbitrary points, accumulated on the GPU.

Drop-in for data_simulation/ModelDensity.py:18-85 of the reference:
``ModelDensity(inputs, xpts, ypts, zpts, dr=0.05)`` with the points and ``dr`` in planet radii and
the attributes type, origin, unit, dr, Vpix, density, packets, totalsource, atoms_per_packet,
sourcerate, outid and outputfiles.

The reference builds a KD-tree over every catalogued Output's rows and asks it for the rows within
``dr`` of each point (``query_ball_point``), then sums their ``frac``.  Here the POINTS are indexed
once (``DensityIndex``: a uniform grid of cell edge >= dr, built with NumPy) and the HIP kernel
k_density reads every row once, where it lies -- in HBM after ``Input.run`` or uploaded from the
host for restored / variable-step Outputs -- and adds {frac, 1} to each point whose ball holds it.
The membership test is query_ball_point's: with d = q - p in fp64,
``(dx*dx + dy*dy) + dz*dz <= dr*dr``.

Kept quirk of the reference (ModelDensity.py:56): ``Vpix = 4/3/pi * dr**3`` in cm^3, i.e.
(4/(3 pi)) dr^3 and not the volume of the ball (4 pi/3) dr^3.  The density is scaled by it as
written.  Bokeh display is out of scope.

EXTENSION (``moments=True``): the same pass also sums each hit's velocity moments
(k_density_moments: ``MOMENT_COLUMNS`` per point, the products formed in fp64 as f * v_a,
(f * v_a) * v_b and f * f), from which the bulk velocity, the velocity covariance, the kinetic
temperature and the effective number of packets follow per point (``moments_from_sums``).

EXTENSION (``spectrum=dict(...)``): what an in-situ mass spectrometer counts.  The pass
(k_density_spectrum) files every hit under its speed in the frame of a spacecraft moving with a
given velocity at that point, if the direction it arrives from lies within a cone around a
boresight: per point and speed bin the density of the atoms in view and their number flux
(``parse_spectrum``, ``spectrum_from_sums``).

EXTENSION (``ages=(a_lo_s, a_hi_s, nbins)``): the density for a source whose rate changes with time.
The pass (k_density_ages; include/nexoclom_hip.h, "Density ages") files every hit under the age of
its row as well: per point and age bin the density that atoms launched that long ago contribute.
``transient(epochs, history)`` contracts the block with the response matrix of a source history
(transient.py) into the density at every point per epoch, ``transient_track(history, times)`` reads
each point at its own time -- a spacecraft crossing the cloud -- and ``transient_design`` gives the
matrix a fit of the history to such a track needs.
"""
import operator

import numpy as np

from . import constants as const
from .ModelImage import ModelResult
from .atomicdata import atomicmass
from .catalogue import sample_pass
from .frames import MoonFrame, is_planet_origin, refuse_with_moon_origin
from .transient import (TransientDensity, TransientTrack, ages_from_sums, parse_ages,
                        refuse_ages_of, refuse_ages_with, response_matrix, spectrum_times)
from .units import Quantity

MAX_CELLS = 1 << 24           # cells of the point grid (int32 starts; cell coordinates < 2^24)
CELL_SLACK = 1.0 + 2.0**-20   # h >= dr * CELL_SLACK: the neighbour cells cover the ball despite rounding


class DensityIndex:
    """The query points sorted by the cell of a uniform grid (what nxc_density_set takes).

    ``points``: (Q, 3) in planet radii.  Points with a non-finite coordinate are left out of the
    index (their density is 0).  Attributes: ``order`` -- the input position of each indexed
    point, in index order; ``points`` -- those points (n, 3); ``cell_start`` -- int32, ncells + 1;
    ``origin``, ``h`` (cell edge), ``dims`` (cells along x, y, z).  Cell of q along an axis:
    floor((q - origin) * (1 / h)); linear cell (cz * ny + cy) * nx + cx.  The edge starts at
    dr * (1 + 2^-20) and only grows (to keep the grid under MAX_CELLS), which keeps every point
    within dr of a row in the row's cell or a neighbour of it."""

    def __init__(self, points, dr):
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        dr = float(dr)
        if not (np.isfinite(dr) and dr > 0):
            raise ValueError('dr must be a positive number')
        self.dr = dr
        finite = np.flatnonzero(np.isfinite(points).all(axis=1))
        P = points[finite]
        h = dr * CELL_SLACK
        if len(P) == 0:
            self.origin, self.h, self.dims = np.zeros(3), h, (1, 1, 1)
            self.order = np.zeros(0, dtype=np.int64)
            self.points = np.zeros((0, 3))
            self.cell_start = np.zeros(2, dtype=np.int32)
            return
        origin = P.min(axis=0)
        while True:
            top = np.floor((P.max(axis=0) - origin) * (1.0 / h)) + 1.0
            cells = float(np.prod(top))
            if cells <= MAX_CELLS:
                break
            h *= max(1.01, 1.001 * (cells / MAX_CELLS) ** (1.0 / 3.0))
        cell = np.floor((P - origin) * (1.0 / h)).astype(np.int64)
        dims = tuple(int(v) for v in cell.max(axis=0) + 1)
        linear = (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0]
        order = np.argsort(linear, kind='stable')
        ncells = dims[0] * dims[1] * dims[2]
        counts = np.bincount(linear, minlength=ncells)
        self.origin, self.h, self.dims = origin, h, dims
        self.order = finite[order]
        self.points = np.ascontiguousarray(P[order])
        self.cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    def scatter(self, values, size):
        """Per-indexed-point values back to the input's point order (0 for left-out points)."""
        out = np.zeros(size)
        out[self.order] = values
        return out


def vpix_cm3(dr, radius_km):
    """ModelDensity.py:56 as written: 4/3/pi * dr**3 [R^3] in cm^3 (not the ball's volume)."""
    R_cm = float(radius_km) * 1e5
    return 4/3/np.pi*dr**3 * R_cm**3


# the ten sums of ``moment_sums``, per point: f v_a, (f v_a) v_b, f f over the hits (f = frac)
MOMENT_COLUMNS = ('m1x', 'm1y', 'm1z', 'm2xx', 'm2yy', 'm2zz', 'm2xy', 'm2xz', 'm2yz', 'ff')


def moments_from_sums(s0, sums, unit_km, mass_kg):
    """(velocity (Q, 3) [km/s], velocity_covariance (Q, 3, 3) [km^2/s^2], temperature (Q,) [K],
    effective_packets (Q,)) from the frac sums ``s0`` (Q,) and the moment sums ``sums`` (Q, 10,
    ``MOMENT_COLUMNS``, velocities in R/s with R = ``unit_km``):

    u = S1 / S0, C_ab = S2_ab / S0 - u_a u_b, T = m (C_xx + C_yy + C_zz) / (3 k_B) with km^2/s^2
    taken to m^2/s^2, effective_packets = S0^2 / sum(f^2).  A point whose S0 is not > 0 gets NaN
    in the first three and 0 in the last."""
    s0 = np.asarray(s0, dtype=np.float64)
    sums = np.asarray(sums, dtype=np.float64).reshape(len(s0), 10)
    ok = s0 > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        u = sums[:, 0:3] / s0[:, None] * unit_km
        second = sums[:, 3:9] / s0[:, None] * (unit_km*unit_km)
        eff = np.where(ok, s0*s0 / sums[:, 9], 0.)
    cov = np.empty((len(s0), 3, 3))
    for col, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        cov[:, a, b] = cov[:, b, a] = second[:, col] - u[:, a]*u[:, b]
    temperature = mass_kg * (cov[:, 0, 0] + cov[:, 1, 1] + cov[:, 2, 2]) * 1e6 / (3*const.K_B)
    u[~ok], cov[~ok], temperature[~ok] = np.nan, np.nan, np.nan
    return u, cov, temperature, eff


SPECTRUM_KEYS = ('speed', 'velocity', 'boresight', 'half_angle')
MAX_SPECTRUM_RECORDS = 2**31      # the device's record index is an int
MAX_AGE_RECORDS = 2**31           # likewise


def _vectors(value, Q, name):
    """(Q, 3) float64 from a (3,) or (Q, 3) argument of ``spectrum=``; ValueError otherwise."""
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'spectrum=: {name} must be numbers of shape (3,) or ({Q}, 3)') from None
    if a.shape == (3,):
        a = np.broadcast_to(a, (Q, 3))
    if a.shape != (Q, 3):
        raise ValueError(f'spectrum=: {name} must have the shape (3,) or ({Q}, 3), not {a.shape}')
    if not np.isfinite(a).all():
        raise ValueError(f'spectrum=: {name} must be finite')
    return np.array(a)


def parse_spectrum(spectrum, Q):
    """A ``spectrum=`` argument for ``Q`` points as a dict: ``speed`` (s_lo_kms, s_hi_kms, nbins),
    ``velocity`` (Q, 3) [km/s], ``boresight`` (Q, 3) of unit length (zeros without one),
    ``cos_half`` and ``all_sky``.  ValueError for anything but a dict of ``SPECTRUM_KEYS`` with a
    ``speed``; a speed range that is not three numbers, not finite, negative or empty; a bin count
    that is no positive integer; velocities or boresights of another shape than (3,) or (Q, 3),
    not finite, or a boresight of length 0; ``'ram'`` where the velocity is 0; a ``half_angle``
    outside (0, 180] degrees; more than 2^31 records."""
    if not isinstance(spectrum, dict) or 'speed' not in spectrum:
        raise ValueError("spectrum= takes a dict with 'speed': (s_lo_kms, s_hi_kms, nbins)")
    unknown = sorted(set(spectrum) - set(SPECTRUM_KEYS))
    if unknown:
        raise ValueError(f'spectrum=: unknown keys {unknown}; it takes {SPECTRUM_KEYS}')
    try:
        s_lo, s_hi, nbins = spectrum['speed']
        s_lo, s_hi = float(s_lo), float(s_hi)
    except (TypeError, ValueError):
        raise ValueError('spectrum=: speed takes three numbers (s_lo_kms, s_hi_kms, nbins)') from None
    try:
        nbins = operator.index(nbins)
    except TypeError:
        raise ValueError('spectrum=: the number of bins must be an integer') from None
    if nbins < 1:
        raise ValueError('spectrum=: the number of bins must be at least 1')
    if not (np.isfinite(s_lo) and np.isfinite(s_hi) and np.isfinite(s_hi - s_lo)):
        raise ValueError('spectrum=: the speed range must be finite')
    if s_lo < 0:
        raise ValueError('spectrum=: s_lo_kms must not be negative (it is a speed)')
    if not s_lo < s_hi:
        raise ValueError('spectrum=: the speed range is empty (s_lo_kms must be below s_hi_kms)')
    if Q*(nbins + 2) >= MAX_SPECTRUM_RECORDS:
        raise ValueError('spectrum=: points * (nbins + 2) must stay below 2^31')
    velocity = _vectors(spectrum.get('velocity', (0., 0., 0.)), Q, 'velocity')
    try:
        half_angle = float(spectrum.get('half_angle', 180.))
    except (TypeError, ValueError):
        raise ValueError('spectrum=: half_angle must be a number of degrees') from None
    if not (np.isfinite(half_angle) and 0 < half_angle <= 180):
        raise ValueError('spectrum=: half_angle must lie in (0, 180] degrees')
    boresight = spectrum.get('boresight')
    if isinstance(boresight, str):
        if boresight != 'ram':
            raise ValueError("spectrum=: boresight is (3,), (Q, 3) or the string 'ram'")
        if not (np.linalg.norm(velocity, axis=1) > 0).all():
            raise ValueError("spectrum=: boresight 'ram' needs a velocity that is not 0 at every point")
        boresight = velocity
    all_sky = boresight is None or half_angle == 180
    if boresight is None:
        unit = np.zeros((Q, 3))
    else:
        unit = _vectors(boresight, Q, 'boresight')
        length = np.linalg.norm(unit, axis=1)
        if not (length > 0).all():
            raise ValueError('spectrum=: a boresight of length 0 has no direction')
        unit = unit / length[:, None]
    return {'speed': (s_lo, s_hi, nbins), 'velocity': velocity, 'boresight': unit,
            'cos_half': float(np.cos(np.radians(half_angle))), 'all_sky': bool(all_sky)}


def refuse_with_spectrum(**given):
    """NotImplementedError for what a spectrum pass cannot be combined with."""
    why = {'moments': 'spectrum= does not support moments=True: each is a pass of its own that adds '
                      'to the density, so two passes would add it twice; make two objects',
           'cp': 'spectrum= does not support cp=: there is no all-reduce of the spectrum yet'}
    for key, value in given.items():
        if value is not None and value is not False:
            raise NotImplementedError(why[key])


def spectrum_frames(parsed, unit_km, order):
    """(n, 8) frame records ux uy uz 0 bx by bz 0 of the indexed points (``order``: their input
    positions), the velocity in R/s."""
    frames = np.zeros((len(order), 8))
    frames[:, 0:3] = parsed['velocity'][order] / unit_km
    frames[:, 4:7] = parsed['boresight'][order]
    return frames


def spectrum_from_sums(spectrum_sums, scale, unit_km, s_lo_kms, s_hi_kms, mass_kg):
    """What a spectrum pass publishes, from ``spectrum_sums`` (2, Q, nbins + 2, 2): plane 0 holds
    {sum f, sum f f}, plane 1 {sum f s, sum (f s)^2} with s in R/s (R = ``unit_km``), per point and
    speed plane (0 below the range, 1..nbins the bins, nbins + 1 at or above it), over the rows
    in view.  ``scale`` = atoms_per_packet / Vpix, the scaling of ``density``.
      speed_edges, speed_axis    s_lo + k (s_hi - s_lo)/nbins and the bins' centres [km/s]
      energy_edges               m s^2 / 2 at the edges [eV]
      density_spectrum (Q, nbins), density_below, density_above (Q,)   sum f * scale [1/cm^3],
                                 per bin (not per km/s); density_in_view (Q,) their sum
      flux_spectrum, flux_below, flux_above, flux    sum f s * scale with s in cm/s [1/cm^2/s]
      spectrum_effective_packets, flux_effective_packets (Q, nbins)   sum^2 / sum of squares,
                                 0 where a bin is empty"""
    sums = np.asarray(spectrum_sums, dtype=np.float64)
    nbins = sums.shape[2] - 2
    edges = s_lo_kms + np.arange(nbins + 1)*(s_hi_kms - s_lo_kms)/nbins
    out = {'speed_edges': edges, 'speed_axis': (edges[:-1] + edges[1:])/2,
           'energy_edges': 0.5*mass_kg*(edges*1e3)**2 / const.EV}
    for plane, name, factor in ((0, 'density', scale), (1, 'flux', scale*unit_km*1e5)):
        S, ww = sums[plane, :, :, 0], sums[plane, :, :, 1]
        out[name + '_spectrum'] = S[:, 1:-1]*factor
        out[name + '_below'] = S[:, 0]*factor
        out[name + '_above'] = S[:, -1]*factor
        total = S.sum(axis=1)*factor
        out['density_in_view' if plane == 0 else 'flux'] = total
        filled = ww[:, 1:-1] != 0
        eff = np.where(filled, S[:, 1:-1]**2/np.where(filled, ww[:, 1:-1], 1.0), 0.0)
        out[('spectrum' if plane == 0 else 'flux') + '_effective_packets'] = eff
    return out


class ModelDensity:
    def __init__(self, inputs, xpts, ypts, zpts, dr=0.05, moments=False, *, cp=None,
                 reduce='rccl', context=None, device=0, spectrum=None, origin=None, ages=None):
        """Number density at the points (xpts, ypts, zpts) [planet radii] from every catalogued
        Output of ``inputs`` (ModelDensity.py:18-85).  ``cp``: the control plane of a shared run
        (``Input.run(..., cp=cp)``): each rank sums its own Outputs, then the per-point sums and
        the source totals are summed over the ranks before scaling.

        ``moments=True`` (EXTENSION) also fills, per point and in the planet-centred frame of the
        rows: ``velocity`` (Q, 3) [km/s], ``velocity_covariance`` (Q, 3, 3) [km^2/s^2],
        ``temperature`` (Q,) [K] and ``effective_packets`` (Q,) -- ``density /
        sqrt(effective_packets)`` is the 1-sigma statistical error of ``density`` -- from
        ``moment_sums`` (Q, 10; ``MOMENT_COLUMNS``), accumulated in the same pass over the rows.
        A point without weight gets NaN, NaN, NaN and 0.

        ``spectrum=dict(speed=(s_lo_kms, s_hi_kms, nbins), velocity=..., boresight=...,
        half_angle=...)`` (EXTENSION) also fills, per point, the speed spectrum in the frame of a
        spacecraft that moves with ``velocity`` ((3,) or (Q, 3) [km/s], model frame; default 0)
        there, of the atoms that arrive within ``half_angle`` degrees (in (0, 180]; default 180) of
        ``boresight`` ((3,) or (Q, 3), normalised here, or ``'ram'`` for the direction of the
        velocity).  180 degrees or no boresight is the whole sky: ``density_in_view`` is then
        ``density`` up to the order of the additions.  Attributes: those of
        ``spectrum_from_sums`` and the raw ``spectrum_sums`` (2, Q, nbins + 2, 2).  It refuses
        ``moments=True`` and ``cp=``.

        ``origin=`` (EXTENSION): a moon among geometry.objects, by name or as an SSObject.  The
        rows are moved into the frame that co-rotates with the moon (frames.MoonFrame) before they
        are read: the points and ``dr`` are then in moon radii from the moon's centre, and the
        velocities of ``moments=`` and ``spectrum=`` are relative to the moon (a spacecraft's
        ``velocity`` likewise).  It refuses ``cp=``.  None or the planet: nothing changes.

        ``ages=(a_lo_s, a_hi_s, nbins)`` (EXTENSION; catalogued constant-step Outputs only) also
        files every hit under the age of its row, options.endtime minus its t_remaining: ``nbins``
        bins over [a_lo_s, a_hi_s) seconds.  Attributes: the raw ``age_sums`` (Q, nbins + 2, 2) =
        {sum f, sum f f} per point and plane (0 younger than the range, 1..nbins the bins,
        nbins + 1 at or above it; zeros at a point left out of the index) and, scaled as
        ``density`` is, ``age_density`` (Q, nbins), ``age_below``, ``age_above`` (Q,), with
        ``age_edges``, ``age_axis`` [s] and ``age_effective_packets`` (Q, nbins):
        ``age_density.sum(1) + age_below + age_above`` is ``density`` up to the order of the
        additions.  ``transient``, ``transient_track`` and ``transient_design`` read them.  It
        refuses ``moments=True``, ``spectrum=`` and ``cp=``; a moon's ``origin=`` is allowed."""
        if ages is not None:
            refuse_ages_with(moments=moments, spectrum=spectrum, cp=cp)
            ages = parse_ages(ages)
            refuse_ages_of(inputs)
        if spectrum is not None:
            refuse_with_spectrum(moments=moments, cp=cp)
        self.type = 'density'
        self.inputs = inputs
        self.origin = inputs.geometry.planet
        if not is_planet_origin(inputs, origin):
            refuse_with_moon_origin(cp=cp)
            self.frame = MoonFrame.from_inputs(inputs, origin)
            self.origin = self.frame.origin
        self.unit = 'R_' + self.origin.object
        unit_km = float(self.origin.radius.value)
        dr = float(dr.to(self.unit)) if isinstance(dr, Quantity) and dr.unit else float(dr)
        self.dr = Quantity(dr, self.unit)
        self.Vpix = Quantity(vpix_cm3(dr, unit_km), 'cm3')
        xyz = [np.asarray(v, dtype=np.float64).ravel() for v in (xpts, ypts, zpts)]
        if not len(xyz[0]) == len(xyz[1]) == len(xyz[2]):
            raise ValueError('xpts, ypts and zpts must have the same length')
        Q = len(xyz[0])
        self._spectrum = None if spectrum is None else parse_spectrum(spectrum, Q)
        if ages is not None and Q*(ages[2] + 2) >= MAX_AGE_RECORDS:
            raise ValueError('ages=: points * (nbins + 2) must stay below 2^31')
        self._ages = ages
        self.density = np.zeros(Q)
        self.packets = np.zeros(Q)
        self.totalsource = 0.
        self._ctx, self._device = context, device
        self._moments = bool(moments)
        self.counters = {}

        self.outid, self.outputfiles, self.npackets, _ = inputs.search()
        shared = cp is not None and cp.world > 1
        if self.npackets == 0 and not shared:
            raise RuntimeError('No packets found for these Inputs.')
        index = DensityIndex(np.stack(xyz, axis=1), dr)
        frames = None if self._spectrum is None else spectrum_frames(self._spectrum, unit_km,
                                                                      index.order)
        sums, counts, extra = self._accumulate(index, self._moments, frames)
        if self._ages is not None:
            self._index = index                   # transient() sets it up again with it
            self.age_sums = np.zeros((Q, self._ages[2] + 2, 2))
            if extra is not None:
                self.age_sums[index.order] = extra
        if self._spectrum is not None:
            self.spectrum_sums = np.zeros((2, Q, self._spectrum['speed'][2] + 2, 2))
            self.spectrum_sums[:, index.order] = extra
        self.density += index.scatter(sums, Q)
        self.packets += index.scatter(counts, Q)
        if self._moments:
            self.moment_sums = np.zeros((Q, 10))
            self.moment_sums[index.order] = extra
        if shared:
            from .distributed import allreduce_small, guarded
            parts = [self.density, self.packets, [float(self.totalsource), float(self.npackets)]]
            if self._moments:
                parts.append(self.moment_sums.ravel())
            with guarded(cp, self.context()):
                both = allreduce_small(np.concatenate(parts), cp, self.context(), reduce)
            self.density, self.packets = both[:Q].copy(), both[Q:2*Q].copy()
            self.totalsource, self.npackets = float(both[2*Q]), int(round(both[2*Q + 1]))
            if self._moments:
                self.moment_sums = both[2*Q + 2:].reshape(Q, 10).copy()
            if self.npackets == 0:
                raise RuntimeError('No packets found for these Inputs.')
        if self._moments:        # quotients of the summed sums; self.density is still the frac sum
            mass_kg = atomicmass(inputs.options.species).value * const.AMU
            (self.velocity, self.velocity_covariance, self.temperature,
             self.effective_packets) = moments_from_sums(self.density, self.moment_sums, unit_km,
                                                         mass_kg)
        mod_rate = self.totalsource / inputs.options.endtime.value
        self.atoms_per_packet = 1e23 / mod_rate
        self.sourcerate = Quantity(1., '1e23/s')
        self.density = self.density * self.atoms_per_packet/float(self.Vpix)
        if self._spectrum is not None:
            s_lo, s_hi, _ = self._spectrum['speed']
            mass_kg = atomicmass(inputs.options.species).value * const.AMU
            for name, value in spectrum_from_sums(self.spectrum_sums,
                                                  self.atoms_per_packet/float(self.Vpix), unit_km,
                                                  s_lo, s_hi, mass_kg).items():
                setattr(self, name, value)
        if self._ages is not None:
            for name, value in ages_from_sums(self.age_sums, self.atoms_per_packet/float(self.Vpix),
                                              *self._ages[:2]).items():
                setattr(self, name.replace('age_cube', 'age_density'), value)

    context = ModelResult.context         # the catalogue's shared context, found once and kept
    frame, slab_rows = None, ModelResult.slab_rows       # a moon's frame, as the images have it
    _frame_pass = ModelResult._frame_pass
    _ages_transient = ModelResult._ages_transient
    _ages = None              # (a_lo_s, a_hi_s, nbins): the pass also fills age_sums
    _ages_token = None        # what Context.ages_owner holds while the block is this object's total

    def _accumulate(self, index, moments=False, frames=None):
        """(frac sums, counts, moment sums | spectrum sums | age sums | None) per indexed point
        over this process's catalogue (ModelDensity.py:62-82).  Rows in HBM are read where they
        are, one launch per run of adjacent slices of a store; other Outputs upload X's x, y, z,
        frac (with moments or a spectrum -- ``frames``, the indexed points' frame records: and vx,
        vy, vz; with ages: and time)."""
        ctx = self.context()
        self._set_index(ctx, index)
        columns, add = ('x', 'y', 'z', 'frac'), ctx.density_accumulate
        ages = self._ages is not None and len(index.points) > 0    # no block without a point
        if ages:
            columns, add = ('time', 'x', 'y', 'z', 'frac'), ctx.density_ages_accumulate
        if moments:
            ctx.density_moments_enable()
            columns, add = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'), ctx.density_moments_accumulate
        if frames is not None:
            (s_lo, s_hi, nbins), unit_km = self._spectrum['speed'], float(self.origin.radius.value)
            ctx.density_spectrum_enable(nbins, s_lo/unit_km, s_hi/unit_km, self._spectrum['cos_half'],
                                        self._spectrum['all_sky'], frames)
            columns, add = ('x', 'y', 'z', 'vx', 'vy', 'vz', 'frac'), ctx.density_spectrum_accumulate

        runs = list(self.inputs._catalogue)
        if runs:        # (without runs __init__ has raised, or a shared run leaves this rank none)
            # k_density* leave the context's counters alone: nothing to total
            sample_pass(self, runs, lambda ctx, **samples: add(**samples), columns, counters=False,
                        **self._frame_pass())
        extra = ctx.density_spectrum_download() if frames is not None else \
            ctx.density_moments_download() if moments else None
        if ages:       # the resident block is this object's total until the context says otherwise
            extra = ctx.density_ages_download()
            ctx.ages_owner['density'] = self._ages_token = object()
        return (*ctx.density_download(), extra)

    def _set_index(self, ctx, index):
        """The point index and, with ``ages=``, a zeroed age block in the context."""
        ctx.density_set(index.points, index.cell_start, index.origin, index.h, index.dr,
                        index.dims)
        if self._ages is not None and len(index.points):
            a_lo, a_hi, nbins = self._ages
            ctx.density_ages_enable(nbins, float(self.inputs.options.endtime.value), a_lo, a_hi)

    def _need_ages(self, what):
        if self._ages is None:
            raise ValueError(f'{what}() needs an object built with ages=(a_lo_s, a_hi_s, nbins)')
        return self.atoms_per_packet/float(self.Vpix)

    def transient(self, epochs, history):
        """The density at every point at ``epochs`` [s] for a source whose rate relative to the
        nominal one was ``history = (t_nodes_s, rate_nodes)`` (transient.response_matrix): a
        TransientDensity with epochs, kernel (nbins + 2, E), density (E, Q), scaled as ``density``
        is, and effective_packets (E, Q).  The age block is contracted where it is (k_ages_apply)
        while this object's sums are the ones resident in its context; when another product has
        replaced them since, the index is set up again and ``age_sums`` uploaded once.  The device
        works in the index's point order; the result is in the input's."""
        scale = self._need_ages('transient')
        K = response_matrix(self.age_edges, epochs, history)
        index, Q = self._index, len(self.age_sums)
        sums = np.zeros((K.shape[1], Q, 2))
        if len(index.points):
            sums[:, index.order] = self._ages_transient(
                'density', lambda ctx: self._set_index(ctx, index),
                lambda: self.age_sums[index.order], K)
        return TransientDensity(epochs, K, sums, scale)

    def transient_track(self, history, times):
        """The trajectory's product: point q read at its own time.  ``times``: (Q,) seconds on the
        history's clock, or one number for all points.  A TransientTrack with times, kernel
        (nbins + 2, Q) -- column q the response at the time of point q --, density (Q,) =
        scale * sum_k S[q][k] K[k][q], scaled as ``density`` is, and effective_packets (Q,).  The
        sums run over the planes from 0 upwards, from 0.0, on the host: a track has 1e4 points."""
        scale = self._need_ages('transient_track')
        times = spectrum_times(times, None, len(self.age_sums))
        return TransientTrack(times, self.age_edges, history, self.age_sums, scale)

    def transient_design(self, t_nodes, times):
        """(Q, J) matrix A with ``A @ rates == transient_track((t_nodes, rates), times).density``
        up to rounding: column j is ``transient_track`` of the history with rate 1 at node j and
        0 at the others.  What a non-negative least-squares fit of a source history to the
        densities measured along a track needs; the fit itself is the caller's."""
        nodes = np.atleast_1d(np.asarray(t_nodes, dtype=float))
        columns = [self.transient_track((nodes, np.eye(len(nodes))[j]), times).density
                   for j in range(len(nodes))]
        return np.stack(columns, axis=1)
