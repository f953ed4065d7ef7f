"""ModelResult / ModelImage: column-density and radiance images, accumulated on the GPU.

Drop-in for data_simulation/ModelResult.py:10-170 and data_simulation/ModelImage.py:26-105,
229-274,367-384 of the reference: ``ModelImage(inputs, params, overwrite=False, distribute=None)``
with ``params`` a dict or a ``key = value`` file (quantity, dims, center, width, subobslongitude,
subobslatitude, wavelength, g) and the attributes image, packet_image, xaxis, zaxis, Apix,
totalsource, atoms_per_packet, sourcerate, dims, center, width.

Two ways to get the packets:
* catalogued Outputs that hold trajectories (``inputs.run(...)``): each one is restored
  (float32 -> float64, Output.py:555-570) and binned by the HIP image kernel -- the reference's
  create_image data flow;
* STREAMING (keyword ``npackets``): integrate and bin in one persistent kernel; the trajectory
  tensor is never built.  ``downcast=True`` (default) applies the reference's float32
  save/restore rounding to every sample before binning, so the image is the one the reference's
  two-stage pipeline produces.  ``shard=(lo, hi)`` restricts the run to those global packet
  indices (multi-GPU, nexoclom_amd.distributed).

``moments=True`` (catalogued Outputs only; an extension beyond the reference) adds four velocity
moments per pixel in the same pass: ``moment_sums`` and, from them, ``velocity`` (the line's Doppler
shift, km/s, positive receding), ``velocity_variance`` / ``velocity_dispersion`` (its width),
``velocity_skewness`` and ``effective_packets`` (``image / sqrt(effective_packets)`` is the 1-sigma
statistical error of ``image``).  include/nexoclom_hip.h ("Pixel moments") holds the definition.

``cube=(v_lo_kms, v_hi_kms, nbins)`` (catalogued Outputs only; an extension) adds the line profile of
every pixel in the same pass: ``cube`` (nx, nz, nbins), the image's quantity per Doppler bin of the
line-of-sight velocity (planet frame, positive receding), ``cube_below`` / ``cube_above`` for what
falls outside the range, ``velocity_edges`` / ``velocity_axis`` [km/s], ``cube_effective_packets``
(the error bars: ``cube / sqrt(cube_effective_packets)``) and the unscaled ``cube_sums``.
include/nexoclom_hip.h ("Velocity cube") holds the definition.

``ages=(a_lo_s, a_hi_s, nbins)`` (catalogued constant-step Outputs only; an extension) files every
sample's weight under its age -- a row at t_remaining = t is a packet launched t0 - t seconds before
the epoch, t0 = options.endtime -- in the same pass: ``age_cube`` (nx, nz, nbins), the image's
response to a pulse of the source, ``age_below`` / ``age_above``, ``age_edges`` / ``age_axis`` [s],
``age_effective_packets`` and the unscaled ``age_sums``; ``transient(epochs, history)`` contracts
it with the response matrix of a source history into one image per epoch (transient.py).
include/nexoclom_hip.h ("Age cube") holds the definition.

``params['origin']`` (catalogued Outputs only; an extension where the reference stops at planets
with moons): the planet, or a moon among geometry.objects.  A moon makes ``center`` and ``width``
lengths in moon radii around the moon, which then occults and shadows; the stored rows are moved
into the frame that co-rotates with the moon before they are binned (frames.MoonFrame,
catalogue.sample_pass(..., frame=), in slabs of ``slab_rows`` rows), and ``moments`` / ``cube``
velocities are relative to the moon.  include/nexoclom_hip.h ("Moon-centred frame") holds the
definition.

Bokeh display / PostgreSQL caching of the reference are out of scope.
"""
import copy
import operator
import json
import os

import numpy as np

from .atomicdata import gValue
from .catalogue import framed_columns, framed_slabs, run_g_values, sample_pass, shared_context
from .frames import MoonFrame, is_planet_origin, refuse_with_moon_origin
from .input_classes import InputError
from .transient import (TransientImages, ages_from_sums, new_age_sums, parse_ages, refuse_ages_of,
                        refuse_ages_with, response_matrix)
from .units import Quantity

HOST_SAMPLER_THREADS = 4        # chunks drawn ahead of the device by the streaming image
QUANTITIES = ('column', 'radiance', 'density', 'difrad')
EMISSION = ('radiance', 'difrad')
# resonance lines [Angstrom] summed when params name none (ModelResult.py:124-129)
DEFAULT_LINES = {'Na': (5891, 5897), 'Ca': (4227,), 'Mg': (2852,)}
# the four sums per pixel of a moments pass, with w the sample's weight and v its line-of-sight
# velocity [R/s]: sum w v, sum (w v) v, sum ((w v) v) v, sum w w
PIXEL_MOMENT_COLUMNS = ('m1', 'm2', 'm3', 'ww')
MOMENT_ATTRIBUTES = ('velocity', 'velocity_variance', 'velocity_dispersion', 'velocity_skewness',
                     'effective_packets')


def pixel_moments_from_sums(S0, sums, unit_km):
    """Per-pixel quotients of the moment sums: ``S0`` the unscaled image sum (sum w), ``sums``
    (..., 4) in PIXEL_MOMENT_COLUMNS order, ``unit_km`` the length unit [km] that turns R/s into
    km/s.  Returns a dict of
      velocity             u = m1/S0                                  [km/s]
      velocity_variance    m2/S0 - u^2, unclamped                     [km^2/s^2]
      velocity_dispersion  sqrt(max(variance, 0))                     [km/s]
      velocity_skewness    (m3/S0 - 3 u m2/S0 + 2 u^3)/variance^1.5 where variance > 0, else NaN
      effective_packets    S0^2/ww
    A pixel with S0 == 0 gets NaN for the velocity quantities and 0 effective packets."""
    S0 = np.asarray(S0, dtype=float)
    sums = np.asarray(sums, dtype=float)
    m1, m2, m3, ww = (sums[..., k] for k in range(4))
    filled = S0 != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        safe = np.where(filled, S0, np.nan)
        u, q2, q3 = m1/safe, m2/safe, m3/safe
        variance = q2 - u*u
        central3 = q3 - 3*u*q2 + 2*u*u*u
        skewness = np.where(variance > 0, central3/np.where(variance > 0, variance, np.nan)**1.5,
                            np.nan)
        effective = np.where(filled, S0*S0/np.where(filled, ww, 1.0), 0.0)
    return {'velocity': u*unit_km,
            'velocity_variance': variance*unit_km**2,
            'velocity_dispersion': np.sqrt(np.maximum(variance, 0))*unit_km,
            'velocity_skewness': skewness,
            'effective_packets': effective}


def refuse_moments_with(**given):
    """NotImplementedError for what a moments pass cannot be combined with."""
    why = {'npackets': 'moments=True reads catalogued Outputs only: streaming (npackets=) bins inside '
                       'the fused integrate kernel, which carries no velocity moments',
           'shard': 'moments=True does not support shard=: the moment sums are not reduced over '
                    'shards',
           'cp': 'moments=True does not support cp=: there is no all-reduce of the moment sums yet'}
    for key, value in given.items():
        if value is not None:
            raise NotImplementedError(why[key])


def parse_cube(cube):
    """``(v_lo_kms, v_hi_kms, nbins)`` of a ``cube=`` argument as (float, float, int); ValueError
    for anything but three numbers, a bin count that is no positive integer, or a range that is
    empty or not finite."""
    try:
        v_lo, v_hi, nbins = cube
        v_lo, v_hi = float(v_lo), float(v_hi)
    except (TypeError, ValueError):
        raise ValueError('cube= takes three numbers (v_lo_kms, v_hi_kms, nbins)') from None
    try:
        nbins = operator.index(nbins)
    except TypeError:
        raise ValueError('cube=: the number of bins must be an integer') from None
    if nbins < 1:
        raise ValueError('cube=: the number of bins must be at least 1')
    if not (np.isfinite(v_lo) and np.isfinite(v_hi) and np.isfinite(v_hi - v_lo)):
        raise ValueError('cube=: the velocity range must be finite')
    if not v_lo < v_hi:
        raise ValueError('cube=: the velocity range is empty (v_lo_kms must be below v_hi_kms)')
    return v_lo, v_hi, nbins


def refuse_cube_with(**given):
    """NotImplementedError for what a cube pass cannot be combined with."""
    why = {'npackets': 'cube= reads catalogued Outputs only: streaming (npackets=) bins inside the '
                       'fused integrate kernel, which carries no velocity cube',
           'shard': 'cube= does not support shard=: the cube is not reduced over shards',
           'cp': 'cube= does not support cp=: there is no all-reduce of the cube yet',
           'moments': 'cube= does not support moments=True: each is a pass of its own that adds to '
                      'the image, so two passes would add it twice; make two objects'}
    for key, value in given.items():
        if value is not None and value is not False:
            raise NotImplementedError(why[key])


def cube_from_sums(cube_sums, atoms_per_packet, v_lo_kms, v_hi_kms):
    """What a cube pass publishes, from ``cube_sums`` (nx, nz, nbins + 2, 2) = {sum w, sum w w} per
    pixel and plane (plane 0 below the range, 1..nbins the bins, nbins + 1 at or above it):
      cube, cube_below, cube_above   sum w times ``atoms_per_packet``, the image's scaling
      velocity_edges, velocity_axis  v_lo + k (v_hi - v_lo)/nbins and the bins' centres [km/s]
      cube_effective_packets         (sum w)^2 / sum w w per bin, 0 where a bin is empty"""
    cube_sums = np.asarray(cube_sums, dtype=float)
    nbins = cube_sums.shape[-2] - 2
    S, ww = cube_sums[..., 1:-1, 0], cube_sums[..., 1:-1, 1]
    filled = ww != 0
    edges = v_lo_kms + np.arange(nbins + 1)*(v_hi_kms - v_lo_kms)/nbins
    return {'cube': S*atoms_per_packet,
            'cube_below': cube_sums[..., 0, 0]*atoms_per_packet,
            'cube_above': cube_sums[..., -1, 0]*atoms_per_packet,
            'velocity_edges': edges,
            'velocity_axis': (edges[:-1] + edges[1:])/2,
            'cube_effective_packets': np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)}


def new_cube_sums(dims, cube):
    """Zeroed ``cube_sums`` for an image of ``dims`` pixels; ValueError when the cube has more
    records than the device addresses (nx nz (nbins + 2) < 2^31)."""
    if dims[0]*dims[1]*(cube[2] + 2) >= 2**31:
        raise ValueError('cube=: dims[0]*dims[1]*(nbins + 2) must stay below 2^31')
    return np.zeros(tuple(dims) + (cube[2] + 2, 2))


def rotation_matrix(theta, axis):
    """Rotation by theta about axis, element for element math/rotation_matrix.py:5-14 (the image
    must bin with the same 3 x 3 doubles as the reference)."""
    u = axis/np.linalg.norm(axis)
    lx, ly, lz = u[0], u[1], u[2]
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[lx**2+(1-lx**2)*c, lx*ly*(1-c)+lz*s, lx*lz*(1-c)-ly*s],
                     [lx*ly*(1-c)-lz*s, ly**2+(1-ly**2)*c, ly*lz*(1-c)+lx*s],
                     [lx*lz*(1-c)+ly*s, ly*lz*(1-c)-lx*s, lz**2+(1-lz**2)*c]])


def read_params(params):
    """The format description of a model result: a dict as given, or the ``key = value`` lines of
    a file (``;`` / ``#`` comments, keys lower-cased; ModelResult.py:77-101)."""
    if isinstance(params, dict):
        return params
    if not isinstance(params, str):
        raise TypeError('ModelResult.__init__', 'params must be a dict or filename.')
    if not os.path.exists(params):
        raise FileNotFoundError('ModelResult.__init__', 'params file not found.')
    table = {}
    with open(params, 'r') as handle:
        for raw in handle:
            text = raw.split(';' if ';' in raw else '#', 1)[0]
            key, eq, value = text.partition('=')
            if eq:
                table[key.strip().lower()] = value.strip()
    return table


def _two(text, convert):
    first, second = str(text).split(',')[:2]
    return [convert(first), convert(second)]


class Histogram2dResult:
    """What math/histogram.py:28-39 exposes: histogram, bin centres x,y and widths dx,dy."""

    def __init__(self, histogram, xedges, yedges):
        self.histogram = histogram
        self.dx, self.dy = xedges[1]-xedges[0], yedges[1]-yedges[0]
        self.x = xedges[:-1] + self.dx/2
        self.y = yedges[:-1] + self.dy/2


class ModelResult:
    """What an image and a line-of-sight result share: the parsed ``params``, the observed
    quantity and, for emission, which lines' g-values weight the packets."""

    def __init__(self, inputs, params):
        self.inputs = copy.copy(inputs)
        self.outid, self.outputfiles, _, _ = inputs.search()
        self.npackets = 0
        self.totalsource = 0.
        self.atoms_per_packet = 0.
        self.sourcerate = Quantity(0., '1e23/s')
        self.params = read_params(params)
        self.quantity = self.params.get('quantity')
        if self.quantity not in QUANTITIES:
            raise InputError('ModelImage.__init__', "quantity must be 'column' or 'radiance'")
        self.g = self.params.get('g', None)
        emits = self.quantity in EMISSION
        self.mechanism = ['resonant scattering'] if emits else None
        self.wavelength = self._lines(inputs.options.species) if emits else None
        self.unit = 'R_' + inputs.geometry.planet.object
        self.unit_km = inputs.geometry.planet.radius.value

    frame = None              # a frames.MoonFrame: the rows are moved into it before they are read

    def _set_origin(self, **refused):
        """``params['origin']``: the planet (the default; nothing changes) or a moon among
        geometry.objects.  A moon makes ``origin``, ``unit`` and ``unit_km`` the moon's -- every
        length of ``params`` is then in moon radii, as the reference's ModelImage.__init__ has it
        for ``origin`` -- and ``frame`` the frame the rows are moved into; it is refused together
        with the keywords ``refused`` that are not None.  Any other origin: NotImplementedError."""
        self.origin = self.params.get('origin', self.inputs.geometry.planet)
        if is_planet_origin(self.inputs, self.origin):
            return
        try:
            frame = MoonFrame.from_inputs(self.inputs, self.origin)
        except ValueError as err:
            raise NotImplementedError(f'{err}: a product is centred on the planet or on a moon '
                                      'that takes part in the run') from None
        refuse_with_moon_origin(**refused)
        self.frame, self.origin = frame, frame.origin
        self.unit, self.unit_km = frame.unit, frame.unit_km

    slab_rows = 1 << 26       # rows moved into a moon's frame at a time (catalogue.framed_slabs)

    def _frame_pass(self):
        """What ``sample_pass`` is told beyond the planet-centred pass: nothing, or the frame."""
        return {} if self.frame is None else dict(frame=self.frame, slab_rows=self.slab_rows)

    def _vr_kms(self, vr_kms):
        """The vrplanet [km/s] a kernel is set with: in a moon's frame the rows carry moon-relative
        velocities, and the Sun-relative one of a row adds the moon's own (frames.MoonFrame)."""
        return vr_kms if self.frame is None else vr_kms + self.frame.radvel_shift_kms

    def _lines(self, species):
        if 'wavelength' in self.params:
            return tuple(sorted(int(w.strip()) for w in str(self.params['wavelength']).split(',')))
        if species is None:
            raise InputError('ModelImage.__init__',
                             'Must provide either species or params.wavelength')
        if species not in DEFAULT_LINES:
            raise InputError('ModelResult.__init__',
                             f'Default wavelengths not available for {species}')
        return DEFAULT_LINES[species]

    def g_tables(self, aplanet):
        """[(velocity [R/s], g [1/s])] per emission line (ModelResult.py:152-157: gValue tables
        with the velocity axis converted to the packets' unit); a constant ``g`` in params is a
        flat two-point table, which makes every packet's g that constant."""
        if self.quantity not in EMISSION:
            return []
        if self.g is not None:
            flat = float(self.g)
            return [(np.array([-1e30, 1e30]), np.array([flat, flat]))]
        species = self.inputs.options.species
        lines = (gValue(species, w, aplanet) for w in self.wavelength)
        return [(line.velocity/self.unit_km, line.g) for line in lines]

    def context(self):
        if self._ctx is None:
            self._ctx = shared_context(self.inputs, self._device)
        return self._ctx

    def _scale(self):
        """atoms_per_packet for a source rate of 1e23 atoms/s (ModelImage.py:102-105)."""
        per_second = self.totalsource / self.inputs.options.endtime.value
        self.atoms_per_packet = 1e23 / per_second if per_second > 0 else 0.
        self.sourcerate = Quantity(1., '1e23/s')

    # ---- the pixels of ModelImage and CameraImage; ``prefix``: the context's 'image' or 'camera'
    moments = False           # True: the pass over the rows also fills moment_sums
    cube = None               # (v_lo_kms, v_hi_kms, nbins): the pass also fills cube_sums
    ages = None               # (a_lo_s, a_hi_s, nbins): the pass also fills age_sums
    _ages_setup = None        # ctx -> None: the last set + enable of this object's age block
    _ages_token = None        # what Context.ages_owner holds while the block is this object's total
    _ages_collects = 0        # downloads added into age_sums

    def _new_pixel_sums(self, moments, cube, ages=None):
        self.image = np.zeros(self.dims)
        self.packet_image = np.zeros(self.dims)
        self.moments = bool(moments)
        if self.moments:
            self.moment_sums = np.zeros(tuple(self.dims) + (len(PIXEL_MOMENT_COLUMNS),))
        self.cube = cube
        if self.cube is not None:
            self.cube_sums = new_cube_sums(self.dims, self.cube)
        self.ages = ages
        if self.ages is not None:
            self.age_sums = new_age_sums(self.dims, self.ages)
            self._ages_token = object()

    def _enable_velocity(self, ctx, prefix):
        if self.moments:
            getattr(ctx, prefix + '_moments_enable')()
        if self.cube is not None:
            v_lo, v_hi, nbins = self.cube
            getattr(ctx, prefix + '_cube_enable')(nbins, v_lo/self.unit_km, v_hi/self.unit_km)
        if self.ages is not None:
            a_lo, a_hi, nbins = self.ages
            getattr(ctx, prefix + '_ages_enable')(nbins, float(self.inputs.options.endtime.value),
                                                  a_lo, a_hi)

    def _collect_pixels(self, ctx, prefix):
        """Add the context's resident sums to the host's; the downloaded image."""
        image, counts = getattr(ctx, prefix + '_download')()
        self.image += image
        self.packet_image += counts.astype(float)
        if self.moments:
            self.moment_sums += getattr(ctx, prefix + '_moments_download')()
        if self.cube is not None:
            self.cube_sums += getattr(ctx, prefix + '_cube_download')()
        if self.ages is not None:
            self.age_sums += getattr(ctx, prefix + '_ages_download')()
            self._collected_ages(ctx, prefix)
        return image

    def _collected_ages(self, ctx, prefix):
        """The resident block has just been added into ``age_sums``: after the first time it IS
        this object's total, which the context is told (every set, clear, enable, pass and upload
        there drops the claim); after a second one it is a part only."""
        self._ages_collects += 1
        if self._ages_collects == 1:
            ctx.ages_owner[prefix] = self._ages_token
        else:
            ctx.ages_owner.pop(prefix, None)

    def _publish_ages(self):
        if self.ages is not None:
            vars(self).update(ages_from_sums(self.age_sums, self.atoms_per_packet, *self.ages[:2]))

    def _ages_transient(self, prefix, setup, sums, K):
        """``Context.ages_transient`` on this object's context for its token.  Called through the
        class: any context that answers ``<prefix>_ages_upload`` / ``_apply`` and keeps an
        ``ages_owner`` is re-seated by the one rule."""
        from .hip_api import Context
        return Context.ages_transient(self.context(), prefix, self._ages_token, setup, sums, K)

    def transient(self, epochs, history, prefix='image'):
        """The images at ``epochs`` [s] for a source whose rate relative to the nominal one was
        ``history = (t_nodes_s, rate_nodes)`` (transient.response_matrix): a TransientImages with
        epochs, kernel, images (E, nx, nz), effective_packets and light_curve.  The age block is
        contracted where it is (k_ages_apply) while this object's sums are the ones resident in its
        context; sums that were added on the host (several stretches of g-values) or that another
        product has replaced since are set up again and uploaded once."""
        if self.ages is None:
            raise ValueError('transient() needs an object built with ages=(a_lo_s, a_hi_s, nbins)')
        if not hasattr(self, 'age_edges'):
            raise ValueError('transient() needs the finalized object (finalize())')
        K = response_matrix(self.age_edges, epochs, history)
        if self._ages_setup is None:                       # nothing was ever binned
            sums = np.zeros((K.shape[1],) + tuple(self.dims) + (2,))
        else:
            sums = self._ages_transient(prefix, self._ages_setup, lambda: self.age_sums, K)
        return TransientImages(epochs, K, sums, self.atoms_per_packet)


class ModelImage(ModelResult):
    def __init__(self, inputs, params, overwrite=False, distribute=None, *, npackets=None,
                 seed=None, packs_per_it=None, downcast=True, device=0, context=None,
                 sampler='numpy', shard=None, finalize=True, generator='philox', moments=False,
                 cube=None, slab_rows=None, ages=None):
        if ages is not None:
            refuse_ages_with(npackets=npackets, shard=shard, moments=moments, cube=cube)
            ages = parse_ages(ages)
            refuse_ages_of(inputs)
        if cube is not None:
            refuse_cube_with(npackets=npackets, shard=shard, moments=moments)
            cube = parse_cube(cube)
        if moments:
            refuse_moments_with(npackets=npackets, shard=shard)
        super().__init__(inputs, params)
        self.type = 'image'
        if slab_rows is not None:
            if operator.index(slab_rows) < 1:
                raise ValueError('slab_rows must be at least 1')
            self.slab_rows = operator.index(slab_rows)
        self._set_origin(npackets=npackets, shard=shard)
        self._frame()
        self._new_pixel_sums(moments, cube, ages)
        self.blimits = None
        self.xaxis = None
        self.zaxis = None
        self._ctx = context
        self._device = device
        self.counters = {}
        if npackets is not None:
            total = int(npackets)
            lo, hi = (0, total) if shard is None else (int(shard[0]), int(shard[1]))
            if not 0 <= lo <= hi <= total:
                raise ValueError('shard must be an index range inside [0, npackets]')
            self._stream(total, seed, packs_per_it, downcast, sampler, lo, hi, generator)
        else:
            self._from_catalogue()
        if finalize:
            self.finalize()

    def _frame(self):
        """Image plane from params (ModelImage.py:53-78): dims (default 800 x 800), center and
        width in planet radii (0,0 and 8 x 8), the sub-observer point (longitude 0, latitude
        pi/2: looking down on the north pole), the bin edges and the pixel area in cm^2."""
        get = self.params.get
        length = lambda text: Quantity(float(text), self.unit)          # noqa: E731
        self.dims = _two(get('dims', '800,800'), int)
        self.center = _two(get('center', '0,0'), length)
        self.width = _two(get('width', '8,8'), length)
        self.subobslongitude = Quantity(float(get('subobslongitude', '0')), 'rad')
        self.subobslatitude = Quantity(float(get('subobslatitude', np.pi/2)), 'rad')
        self.xrange, self.zrange = ([c - w/2, c + w/2] for c, w in zip(self.center, self.width))
        pixel = [w/d for w, d in zip(self.width, self.dims)]
        R_cm = self.unit_km*1e5
        self.Apix = Quantity(pixel[0]*pixel[1]*R_cm**2, 'cm2')
        self.xedges = np.linspace(self.xrange[0], self.xrange[1], self.dims[0]+1)
        self.zedges = np.linspace(self.zrange[0], self.zrange[1], self.dims[1]+1)

    def _from_catalogue(self):
        """Sum of the images of every catalogued Output (ModelImage.py:85-98)."""
        runs = list(self.inputs._catalogue)
        if not runs:
            print('No model outputs found for these inputs.')
        if self._from_resident(runs):
            return
        for run in runs:
            print(f'Output filename: {run.filename}')
            weighted, counted = self.create_image(run)
            self.image += weighted.histogram
            self.packet_image += counted.histogram
            if self.moments:
                self.moment_sums += self._last_moment_sums
            if self.cube is not None:
                self.cube_sums += self._last_cube_sums
            if self.ages is not None:
                self.age_sums += self._last_age_sums
                self._collected_ages(self.context(), 'image')
            self.totalsource += run.totalsource
            self.xaxis, self.zaxis = weighted.x, weighted.y

    def _from_resident(self, runs):
        """The same sum when every run's rows are still in HBM and the runs share their geometry
        (one Input.run): the image pair stays on the device across the runs -- it IS the running
        sum of ModelImage.py:96-98 -- and comes to the host once.  False: not applicable."""
        from .Output import Output
        if not runs or not all(isinstance(run, Output) for run in runs):
            return False
        ctx = self.context()
        if any(run.resident_rows(ctx) is None for run in runs) or \
                len({run_g_values(run) for run in runs}) != 1:
            return False

        def set_up(ctx, aplanet, vr_kms):
            vr = self._vr_kms(vr_kms)/self.unit_km
            self._set_image(ctx, aplanet, vr, downcast=False)      # clears it

        # the Outputs of a launch group are consecutive slices of one store: one kernel launch per
        # run of adjacent slices instead of one per Output
        self._ages_collects = 0
        sample_pass(self, runs, lambda ctx, rows: self._accumulate(ctx, rows=rows), (), set_up,
                    **self._frame_pass())
        image = self._collect_pixels(ctx, 'image')
        h = Histogram2dResult(image, self.xedges, self.zedges)
        self.xaxis, self.zaxis = h.x, h.y
        return True

    def finalize(self):
        """Scale to a source rate of 1e23 atoms/s (ModelImage.py:102-105); deferred by the
        multi-GPU path until the shards are summed."""
        self._scale()
        if self.moments:         # the quotients are of the unscaled sums
            vars(self).update(pixel_moments_from_sums(self.image, self.moment_sums, self.unit_km))
        if self.cube is not None:
            vars(self).update(cube_from_sums(self.cube_sums, self.atoms_per_packet, *self.cube[:2]))
        self._publish_ages()
        self.image *= self.atoms_per_packet

    # ---- GPU plumbing ---------------------------------------------------------------------
    def image_rotation(self):
        """Sun frame -> observer frame (ModelImage.py:367-384): the rotation that carries the
        sub-solar direction (0,-1,0) onto the sub-observer direction."""
        lon, lat = float(self.subobslongitude), float(self.subobslatitude)
        sun = np.array([0., -1., 0.])
        observer = np.array([np.sin(lon)*np.cos(lat), -np.cos(lon)*np.cos(lat), np.sin(lat)])
        if np.array_equal(sun, observer):
            return np.eye(3)
        cosine = np.dot(sun, observer)/np.linalg.norm(sun)/np.linalg.norm(observer)
        return rotation_matrix(np.arccos(np.clip(cosine, -1, 1)), np.cross(sun, observer))

    def _set_image(self, ctx, aplanet, vrplanet_Rs, downcast):
        ctx.set_image(self.image_rotation(), vrplanet_Rs, float(self.Apix), self.quantity,
                      self.xedges, self.zedges, self.g_tables(aplanet), downcast_f32=downcast)
        if self.ages is not None:
            self._ages_setup = lambda ctx: self._set_image(ctx, aplanet, vrplanet_Rs, downcast)
        self._enable_velocity(ctx, 'image')

    def _accumulate(self, ctx, samples=(), rows=None):
        """One pass over host columns or ``rows = (RowStore, first, count)`` through the entry this
        image asked for: the cube's, the moments' or the plain one."""
        if self.ages is not None:
            ctx.image_ages_accumulate(*samples, rows=rows)
        elif self.cube is not None:
            ctx.image_cube_accumulate(*samples, rows=rows)
        elif self.moments:
            ctx.image_moments_accumulate(*samples, rows=rows)
        elif rows is not None:
            ctx.image_accumulate_rows(*rows)
        else:
            ctx.image_accumulate(*samples)

    def create_image(self, output):
        """ModelImage.py:229-274 for one catalogued Output (or .npz path): the restored sample
        columns are rotated, masked, weighted and binned inside one HIP kernel."""
        from .Output import Output
        ctx = self.context()
        view = output.resident_rows(ctx) if isinstance(output, Output) else None
        if view is not None and view[2] > 0:
            # the rows are still in HBM as save() would have stored them: bin them where they are
            aplanet, vrplanet_kms = float(output.aplanet), float(output.vrplanet)
            self._set_image(ctx, aplanet, self._vr_kms(vrplanet_kms)/self.unit_km, downcast=False)
            if self.frame is None:
                self._accumulate(ctx, rows=tuple(view[:3]))
                self.counters = ctx.counters()
            else:           # moved into the moon's frame slab by slab; every launch clears the counters
                self.counters = {}
                for moved in framed_slabs(ctx, self.frame, tuple(view[:3]), self.slab_rows):
                    self._accumulate(ctx, rows=moved)
                    for key, v in ctx.counters().items():
                        self.counters[key] = self.counters.get(key, 0) + v
        else:
            velocity = self.moments or self.cube is not None
            columns = Output.AGE_COLS if self.ages is not None else \
                Output.MOMENT_COLS if velocity else Output.IMAGE_COLS
            if self.frame is not None:
                samples = framed_columns(ctx, self.frame, output, columns)
                aplanet, vrplanet_kms = run_g_values(output)
            elif self.ages is not None:
                samples = Output.sample_columns(output, columns)
                aplanet, vrplanet_kms = run_g_values(output)
            else:
                samples, aplanet, vrplanet_kms = Output.image_columns(output, velocity=velocity)
            if samples is None or len(samples[0]) == 0:
                raise ValueError('this Output holds no trajectory (it was run with '
                                 'keep_trajectory=False); use ModelImage(..., npackets=N) instead')
            vr =self._vr_kms(vrplanet_kms)/self.unit_km   # km/s -> R/s (ModelImage.py:242-243)
            self._set_image(ctx, aplanet, vr, downcast=False)
            self._accumulate(ctx, samples)
            self.counters = ctx.counters()
        assert self.counters['nonfinite'] == 0, 'Non-finite weights'
        image, counts = ctx.image_download()
        if self.moments:
            self._last_moment_sums = ctx.image_moments_download()
        if self.cube is not None:
            self._last_cube_sums = ctx.image_cube_download()
        if self.ages is not None:
            self._last_age_sums = ctx.image_ages_download()
        return (Histogram2dResult(image, self.xedges, self.zedges),
                Histogram2dResult(counts.astype(float), self.xedges, self.zedges))

    def _stream(self, total, seed, packs_per_it, downcast, sampler='numpy', lo=0, hi=None,
                generator='philox'):
        """Fused integrate + image over the packets [lo, hi) of a run of ``total`` packets.

        The run is cut into chunks like Input.run does (Input.py:243-246); the chunk grid depends
        only on ``total`` and ``packs_per_it`` (distributed.chunk_plan), and chunk k of the host
        sampler is drawn from the generator seeded ``seed + k``, so the packets with global index
        in [lo, hi) are the same packets whether this process handles the whole run or one shard
        of it.  The device sampler is counter-based on the global index
        (generator='philox') or follows the host's streams (generator='pcg64'): draws.py."""
        from .Output import Output, n_output_steps
        from .distributed import chunk_plan
        from .draws import DrawAhead, Draws
        inputs = self.inputs
        opt = inputs.options
        # step_size = 0: the adaptive driver keeps one final row per packet; a chunk's rows are
        # built in HBM as save() would store them, binned from there and dropped
        variable = opt.step_size == 0
        hi = total if hi is None else hi
        ctx = self.context()
        rule = Draws(sampler, generator, seed)          # (an unseeded device run: one fresh key)
        self.seed = seed = rule.seed
        chunk = int(packs_per_it) if packs_per_it else max(1, min(total, 20_000_000))
        nsteps, n_iter = (1, 0) if variable else \
            n_output_steps(opt.endtime.value, float(opt.step_size))
        totals = {}
        plan = list(chunk_plan(total, chunk, lo, hi))
        # host-sampled chunks are independent generators (seed + k): the next ones are drawn by
        # worker threads (NumPy releases the GIL) while the device integrates the current one
        ahead = None if sampler == 'device' or len(plan) < 2 else DrawAhead(
            lambda piece: rule.chunk_output(inputs, ctx, piece), plan,
            min(len(plan), HOST_SAMPLER_THREADS))
        try:
            for piece in plan:
                a, n = piece[3], piece[4] - piece[3]
                if ahead is not None:
                    ahead.fill(HOST_SAMPLER_THREADS)
                    out = ahead.popleft().result()
                else:
                    out = rule.chunk_output(inputs, ctx, piece)
                if variable:
                    assert out._bounce is None, 'Not set up'             # Output.py:312-315
                if piece is plan[0]:
                    ctx.set_forces(**out.forces_kwargs())
                    # (adaptive step: the rows come narrowed from their store, not from the kernel)
                    self._set_image(ctx, out.aplanet, out.vrplanet,
                                    downcast and not variable)           # clears the image
                rule.upload_chunk(ctx, out, piece)       # (device draws are resident)
                ctx.set_bounce(out._bounce)
                ctx.set_bodies(out._bodies)
                ctx.set_first_index(a)
                if variable:
                    self._var_chunk(ctx, opt, downcast, totals)
                else:
                    ctx.integrate_const(float(opt.step_size), n_iter, opt.outeredge, image=True)
                    for key, v in ctx.counters().items():
                        totals[key] = totals.get(key, 0) + v
                # Output.py:434; the adaptive driver has no nsteps factor: X0.frac.sum()
                self.totalsource += n * nsteps
                self.npackets += n
        finally:
            if ahead is not None:
                ahead.pool.shutdown(cancel_futures=True)
        self.counters = totals
        assert totals.get('nonfinite', 0) == 0, 'Non-finite weights'
        if not plan:    # an empty shard still owns a resident (zero) image for the reduce
            out = Output(inputs, 0, seed=seed, integrate=False, save=False, context=ctx)
            ctx.set_forces(**out.forces_kwargs())
            self._set_image(ctx, out.aplanet, out.vrplanet, downcast)
        image, counts = ctx.image_download()
        self.image += image
        self.packet_image += counts.astype(float)
        h = Histogram2dResult(image, self.xedges, self.zedges)
        self.xaxis, self.zaxis = h.x, h.y

    @staticmethod
    def _var_chunk(ctx, opt, downcast, totals):
        """The resident packets through the adaptive driver and into the image: finals and rows
        stay in HBM (float32 rows with ``downcast``, like a saved Output's)."""
        ctx.integrate_var(float(opt.resolution), opt.outeredge, resident=True)
        ctr = ctx.counters()
        assert ctr.get('nonfinite', 0) == 0, '\n\tInfinite values of emax or a non-finite impact'
        assert ctr.get('neg_frac', 0) == 0, 'Found new values of frac that are negative'
        assert ctr.get('bad_step', 0) == 0, 'Bad step size'
        assert ctr.get('unfinished', 0) == 0, 'variable-step integration did not finish'
        store, _ = ctx.var_rows_build(narrow=downcast, compress=True)
        try:
            if store.total:
                ctx.image_accumulate_rows(store)
                for key, v in ctx.counters().items():
                    ctr[key] = ctr.get(key, 0) + v
        finally:
            store.free()
        for key, v in ctr.items():
            totals[key] = totals.get(key, 0) + v

    def export(self, filename='image.json'):
        if not filename.endswith('.json'):
            raise TypeError('Not an valid file format')
        with open(filename, 'w') as handle:
            json.dump({k: getattr(self, k).tolist() for k in ('image', 'xaxis', 'zaxis')}, handle)
