"""ShellMap: the cloud in planet-facing coordinates -- density on spherical shells and the zenith
column per local time and latitude, accumulated on the GPU.

An extension beyond the reference, whose products all look at the cloud from outside.
``ShellMap(inputs, params)`` bins every stored sample of the catalogued Outputs into cells of
solar-fixed longitude (local time) x sin(latitude) x altitude around the planet's centre, in one
pass over the rows.  The longitude is the package's: 0 at the sub-solar point (noon), pi/2 at dusk,
the convention of the source maps and the sticking maps.  Latitude bands are uniform in
sin(latitude), so every cell has the same solid angle.  include/nexoclom_hip.h ("ShellMap") holds
the definition operation by operation; the HIP kernel is k_shell.

``params`` (a dict or a ``key = value`` file, like ModelImage's):

    quantity     'column' or 'radiance'
    dims         'nlon,nlat'      default '72,36'
    altitude     'lo,hi,nbins'    planet radii above the surface, 0 <= lo < hi (required)
    g / wavelength                as ModelResult
    origin       the planet (default) or a moon among geometry.objects: the rows are moved into the
                 frame that co-rotates with the moon (frames.MoonFrame) and the shells lie around
                 the moon, altitude in moon radii above its surface

Attributes: longitude, local_time (hours; 12 at longitude 0, 18 at pi/2), latitude (asin of the
band centres, rad), lon_edges, mu_edges, altitude_edges, altitude_axis (planet radii above the
surface; altitude_edges_km, altitude_axis_km), solid_angle (sr per cell), column (nlon, nlat: the zenith column
atoms_per_packet sum w/r^2 / (solid_angle R_cm^2) -- atoms/cm^2, or the zenith radiance in
ModelImage's units), packets, density (nlon, nlat, nalt: atoms_per_packet sum w / V_k with V_k =
solid_angle (r_{k+1}^3 - r_k^3)/3 R_cm^3 -- atoms/cm^3, or the radiance per cm of path),
column_profile (the zenith column per shell) with column_below and column_above
(column_profile.sum(-1) + column_below + column_above is column), density_effective_packets and
column_effective_packets ((sum a)^2 / sum a^2 per cell and shell, 0 where a shell is empty),
shell_sums (the unscaled download), totalsource, atoms_per_packet, sourcerate, counters.

``ShellMap(inputs, params, moments=True)``: the same single pass (k_shell_moments; "ShellMap
moments" in the header) also files every sample's velocity, resolved in the local basis (radial up,
east toward increasing longitude, north), under its cell and altitude bin.  Then also: velocity
(nlon, nlat, nalt, 3) [km/s], velocity_covariance (..., 3, 3) [km^2/s^2], temperature [K],
shell_moment_sums (the unscaled download, ``SHELL_MOMENT_COLUMNS``), and for 'column' flux_up,
flux_down, flux_net [atoms cm^-2 s^-1] with flux_up_effective_packets and
flux_down_effective_packets, and shell_rate_up, shell_rate_down, shell_rate_net (nalt,) [atoms/s]:
the number rate through each shell -- at the top shell the escape rate, ``down`` at the bottom
shell the return rate to the surface (``shell_moments_from_sums``).  For 'radiance' the moments are
emission-weighted and the fluxes and rates are None.  With ``origin`` a moon the velocities are
relative to the moon.

``ShellMap(inputs, params, ages=(a_lo_s, a_hi_s, nbins))`` (catalogued constant-step Outputs only):
the same single pass (k_shell_ages; "ShellMap ages" in the header) also files both records of every
sample under its age, options.endtime minus the row's t_remaining: ``nbins`` bins over [a_lo_s,
a_hi_s) seconds.  Then also (``shell_ages_from_sums``): shell_age_sums (2, nlon, nlat, nalt + 2,
nbins + 2, 2; the unscaled block), age_density (nlon, nlat, nalt, nbins) with age_density_below and
age_density_above (the ages outside the range), age_column_profile (nlon, nlat, nalt, nbins),
age_column (nlon, nlat, nbins) with age_column_below and age_column_above, age_edges, age_axis [s],
age_density_effective_packets and age_column_effective_packets: age_density.sum(-1) +
age_density_below + age_density_above is density and age_column.sum(-1) + age_column_below +
age_column_above is column, up to the order of the additions.  ``transient(epochs, history)``
contracts the block with the response matrix of a source history (transient.py) on the device: the
density, the zenith column and the content inside the altitude range per epoch (a
transient.TransientShells).  It refuses ``moments=True`` (make two objects); a moon's ``origin`` is
allowed.

Not supported, and refused: streaming (``npackets=``), shared runs (``cp=`` / ``shard=``).
"""
import numpy as np

from . import constants as const
from .ModelDensity import moments_from_sums
from .ModelImage import ModelResult
from .Output import Output
from .atomicdata import atomicmass
from .catalogue import sample_pass
from .input_classes import InputError
from .transient import (TransientShells, parse_ages, refuse_ages_of, refuse_ages_with,
                        response_matrix)

MAX_DIM = 8192
UNSUPPORTED = {
    'npackets': 'streaming (npackets=) is not supported: run the inputs first (Input.run)',
    'cp': 'shared runs (cp=) are not supported by ShellMap',
    'shard': 'shards are not supported by ShellMap',
    'reduce': 'shared runs (cp=) are not supported by ShellMap',
}


def parse_dims(text):
    """``'nlon,nlat'`` as two ints in 1..8192."""
    try:
        dims = [int(v) for v in str(text).split(',')]
    except ValueError:
        dims = []
    if len(dims) != 2:
        raise InputError('ShellMap.__init__', "dims must be two integers 'nlon,nlat'")
    if not all(1 <= d <= MAX_DIM for d in dims):
        raise InputError('ShellMap.__init__', f'dims must be 1..{MAX_DIM}')
    return dims


def parse_altitude(text):
    """``'lo,hi,nbins'`` [planet radii above the surface] as (float, float, int)."""
    parts = str(text).split(',')
    try:
        lo, hi = float(parts[0]), float(parts[1])
        nbins = int(parts[2])
    except (ValueError, IndexError):
        parts = []
    if len(parts) != 3:
        raise InputError('ShellMap.__init__',
                         "altitude must be 'lo,hi,nbins' (two numbers and an integer)")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise InputError('ShellMap.__init__', 'altitude: lo and hi must be finite')
    if not 0.0 <= lo < hi:
        raise InputError('ShellMap.__init__', 'altitude: 0 <= lo < hi is required')
    if nbins < 1:
        raise InputError('ShellMap.__init__', 'altitude: nbins must be at least 1')
    return lo, hi, nbins


def shell_axes(nlon, nlat, alt_lo, alt_hi, nalt):
    """The grid of a shell map: a dict of lon_edges, mu_edges, r_edges [R from the centre] and what
    follows from them (longitude, local_time, latitude, solid_angle, shell volumes in R^3)."""
    lon_edges = np.linspace(0, 2*np.pi, nlon + 1)
    mu_edges = np.linspace(-1, 1, nlat + 1)
    r_lo, r_hi = 1.0 + alt_lo, 1.0 + alt_hi
    r_edges = r_lo + np.arange(nalt + 1)*(r_hi - r_lo)/nalt
    r_edges[-1] = r_hi
    longitude = 0.5*(lon_edges[:-1] + lon_edges[1:])
    solid_angle = (2*np.pi/nlon)*(2.0/nlat)
    return {'lon_edges': lon_edges, 'mu_edges': mu_edges, 'r_edges': r_edges,
            'longitude': longitude,
            'local_time': (12.0 + longitude*12.0/np.pi) % 24.0,
            'latitude': np.arcsin(0.5*(mu_edges[:-1] + mu_edges[1:])),
            'solid_angle': solid_angle,
            'volume': solid_angle*(r_edges[1:]**3 - r_edges[:-1]**3)/3}


def _effective(S, ww):
    filled = ww != 0
    return np.where(filled, S*S/np.where(filled, ww, 1.0), 0.0)


def shell_from_sums(column_sum, shell_sums, atoms_per_packet, solid_angle, volume, R_cm):
    """What a shell map publishes, from ``column_sum`` (nlon, nlat) = sum w/r^2 and ``shell_sums``
    (2, nlon, nlat, nalt + 2, 2) = {sum w, sum w w} and {sum c, sum c c}, c = w/r^2, per cell and
    altitude record (record 0 below the range, 1..nalt the bins, nalt + 1 at or above it);
    ``volume`` (nalt) in R^3, ``R_cm`` the planet's radius."""
    shell_sums = np.asarray(shell_sums, dtype=float)
    A, B = shell_sums[0], shell_sums[1]
    per_area = atoms_per_packet/(solid_angle*R_cm**2)
    return {'column': np.asarray(column_sum, dtype=float)*per_area,
            'density': A[..., 1:-1, 0]*atoms_per_packet/(np.asarray(volume)*R_cm**3),
            'column_profile': B[..., 1:-1, 0]*per_area,
            'column_below': B[..., 0, 0]*per_area,
            'column_above': B[..., -1, 0]*per_area,
            'density_effective_packets': _effective(A[..., 1:-1, 0], A[..., 1:-1, 1]),
            'column_effective_packets': _effective(B[..., 1:-1, 0], B[..., 1:-1, 1])}


# the twelve sums of ``shell_moment_sums`` per cell and altitude record, plane by plane and half by
# half: u_a = w v_a in the local basis (r up, e east, n north), up = u_r where v_r > 0, dn = -u_r
# where v_r < 0 (include/nexoclom_hip.h, "ShellMap moments")
SHELL_MOMENT_COLUMNS = ('ur', 'ue', 'un', 'urr', 'uee', 'unn', 'ure', 'urn', 'uen', 'up', 'upup',
                        'dndn')


def shell_moments_from_sums(shell_sums, moment_sums, atoms_per_packet, volume, r_edges, unit_km,
                            mass_kg, quantity='column'):
    """What ``ShellMap(moments=True)`` publishes, from ``shell_sums`` (2, nlon, nlat, nalt + 2, 2,
    plane A = {sum w, sum w w}) and ``moment_sums`` (6, nlon, nlat, nalt + 2, 2), the twelve sums of
    ``SHELL_MOMENT_COLUMNS`` with velocities in R/s, R = ``unit_km``; ``volume`` (nalt) in R^3,
    ``r_edges`` (nalt + 1) in R, ``mass_kg`` the atom's.

    Per cell and altitude bin, over plane A's sum w of the same record (NaN where it is not > 0), as
    ModelDensity.moments_from_sums forms them: ``velocity`` (..., 3) [km/s] in the order (radial,
    east, north), ``velocity_covariance`` (..., 3, 3) [km^2/s^2], ``temperature`` [K] =
    m tr C / (3 k_B).  For ``quantity`` 'column' also the fluxes [atoms cm^-2 s^-1]
    atoms_per_packet S / (V_k R_cm^2) with S = sum up (``flux_up``), sum up - sum u_r
    (``flux_down``) and sum u_r (``flux_net``); their effective packets (sum)^2 / sum of squares, 0
    where empty; and per shell the number rates [atoms/s] through it, atoms_per_packet sum_cells S /
    dr (``shell_rate_up``, ``shell_rate_down``, ``shell_rate_net``): the volume estimator.  For
    'radiance' the moments are emission-weighted and the fluxes and rates are None."""
    A = np.asarray(shell_sums, dtype=float)[0][..., 1:-1, :]
    M = np.moveaxis(np.asarray(moment_sums, dtype=float), 0, -2)[..., 1:-1, :, :]
    shape = A.shape[:-1]
    M = M.reshape(shape + (12,))
    col = {name: M[..., k] for k, name in enumerate(SHELL_MOMENT_COLUMNS)}
    ten = np.stack([col[c] for c in ('ur', 'ue', 'un', 'urr', 'uee', 'unn', 'ure', 'urn', 'uen')]
                   + [A[..., 1]], axis=-1)
    u, cov, temperature, _ = moments_from_sums(A[..., 0].reshape(-1), ten.reshape(-1, 10), unit_km,
                                               mass_kg)
    out = {'velocity': u.reshape(shape + (3,)), 'velocity_covariance': cov.reshape(shape + (3, 3)),
           'temperature': temperature.reshape(shape)}
    names = ('flux_up', 'flux_down', 'flux_net', 'flux_up_effective_packets',
             'flux_down_effective_packets', 'shell_rate_up', 'shell_rate_down', 'shell_rate_net')
    if quantity != 'column':
        out.update(dict.fromkeys(names))
        return out
    R_cm = unit_km*1e5
    S = {'up': col['up'], 'down': col['up'] - col['ur'], 'net': col['ur']}
    dr = np.diff(np.asarray(r_edges, dtype=float))
    for name, value in S.items():
        out['flux_' + name] = value*atoms_per_packet/(np.asarray(volume)*R_cm**2)
        out['shell_rate_' + name] = atoms_per_packet*value.sum(axis=(0, 1))/dr
    out['flux_up_effective_packets'] = _effective(S['up'], col['upup'])
    out['flux_down_effective_packets'] = _effective(S['down'], col['dndn'])
    return out


MAX_AGE_RECORDS = 2**31           # the device's record index is an int


def shell_ages_from_sums(shell_age_sums, atoms_per_packet, solid_angle, volume, R_cm, a_lo, a_hi):
    """What ``ShellMap(ages=...)`` publishes, from ``shell_age_sums`` (2, nlon, nlat, nalt + 2,
    nbins + 2, 2) = {sum w, sum w w} (age plane A) and {sum c, sum c c}, c = w/r^2 (age plane B) per
    cell, altitude record and age plane (plane 0 younger than the range, 1..nbins the bins,
    nbins + 1 at or above it); ``volume`` (nalt) in R^3, ``R_cm`` the planet's radius.  Scaled as
    ``shell_from_sums`` scales density and column:
      age_density (nlon, nlat, nalt, nbins), age_density_below, age_density_above (nlon, nlat, nalt)
      age_column_profile (nlon, nlat, nalt, nbins)
      age_column (nlon, nlat, nbins), age_column_below, age_column_above (nlon, nlat): plane B summed
                 over all nalt + 2 records of a cell, from record 0 upwards
      age_edges, age_axis [s]
      age_density_effective_packets (as age_density), age_column_effective_packets (as age_column):
                 (sum)^2 / sum of squares, 0 where empty"""
    sums = np.asarray(shell_age_sums, dtype=float)
    A, B = sums[0], sums[1]
    nbins = sums.shape[-2] - 2
    per_area = atoms_per_packet/(solid_angle*R_cm**2)
    volume_cm3 = np.asarray(volume)*R_cm**3               # density: sum * atoms_per_packet / V, as
                                                          # shell_from_sums forms it
    cell = np.zeros(B.shape[:2] + B.shape[3:])           # (nlon, nlat, nbins + 2, 2)
    for k in range(B.shape[2]):
        cell = cell + B[:, :, k]
    edges = a_lo + np.arange(nbins + 1)*(a_hi - a_lo)/nbins
    return {'age_density': A[:, :, 1:-1, 1:-1, 0]*atoms_per_packet/volume_cm3[:, None],
            'age_density_below': A[:, :, 1:-1, 0, 0]*atoms_per_packet/volume_cm3,
            'age_density_above': A[:, :, 1:-1, -1, 0]*atoms_per_packet/volume_cm3,
            'age_column_profile': B[:, :, 1:-1, 1:-1, 0]*per_area,
            'age_column': cell[:, :, 1:-1, 0]*per_area,
            'age_column_below': cell[:, :, 0, 0]*per_area,
            'age_column_above': cell[:, :, -1, 0]*per_area,
            'age_edges': edges,
            'age_axis': (edges[:-1] + edges[1:])/2,
            'age_density_effective_packets': _effective(A[:, :, 1:-1, 1:-1, 0],
                                                        A[:, :, 1:-1, 1:-1, 1]),
            'age_column_effective_packets': _effective(cell[:, :, 1:-1, 0], cell[:, :, 1:-1, 1])}


class ShellMap(ModelResult):
    moments = False           # True: the pass over the rows also fills shell_moment_sums

    def __init__(self, inputs, params, *, moments=False, ages=None, context=None, device=0,
                 **unsupported):
        if ages is not None:
            refuse_ages_with(moments=moments,
                             **{key: unsupported.get(key) for key in ('npackets', 'shard', 'cp')})
            ages = parse_ages(ages)
            refuse_ages_of(inputs)
        for key in unsupported:
            if key in UNSUPPORTED:
                raise NotImplementedError(UNSUPPORTED[key])
            raise TypeError(f'ShellMap() got an unexpected keyword argument {key!r}')
        super().__init__(inputs, params)
        self.type = 'shell map'
        if self.quantity not in ('column', 'radiance'):
            raise InputError('ShellMap.__init__', "quantity must be 'column' or 'radiance'")
        self._set_origin()          # (npackets=, shard= and cp= are refused above, whatever the origin)
        self._frame()
        self._column_sum = np.zeros(self.dims)
        self.packets = np.zeros(self.dims)
        self.shell_sums = np.zeros((2,) + tuple(self.dims) + (self.altitude[2] + 2, 2))
        self.moments = bool(moments)
        if self.moments:
            self.shell_moment_sums = np.zeros((6,) + self.shell_sums.shape[1:])
        self.ages = ages
        if self.ages is not None:
            records = self.dims[0]*self.dims[1]*(self.altitude[2] + 2)
            if records*(self.ages[2] + 2) >= MAX_AGE_RECORDS:
                raise ValueError('ages=: nlon*nlat*(altitude bins + 2)*(nbins + 2) must stay below '
                                 '2^31')
            self.shell_age_sums = np.zeros((2,) + tuple(self.dims) +
                                           (self.altitude[2] + 2, self.ages[2] + 2, 2))
            self._ages_token = object()
        self._ctx, self._device = context, device
        self.counters = {}
        self._from_catalogue()
        self.finalize()

    def _frame(self):
        get = self.params.get
        self.dims = parse_dims(get('dims', '72,36'))
        if 'altitude' not in self.params:
            raise InputError('ShellMap.__init__',
                             "params need altitude = 'lo,hi,nbins' [planet radii above the surface]")
        self.altitude = parse_altitude(get('altitude'))
        if self.dims[0]*self.dims[1]*(self.altitude[2] + 2) >= 2**31:
            raise InputError('ShellMap.__init__',
                             'nlon*nlat*(nbins + 2) must stay below 2^31 records')
        axes = shell_axes(*self.dims, *self.altitude)
        for name in ('lon_edges', 'mu_edges', 'longitude', 'local_time', 'latitude', 'solid_angle'):
            setattr(self, name, axes[name])
        self.r_edges = axes['r_edges']
        self._volume = axes['volume']
        self.altitude_edges = self.r_edges - 1.0                      # [self.unit]
        self.altitude_axis = 0.5*(self.r_edges[:-1] + self.r_edges[1:]) - 1.0
        self.altitude_edges_km = self.altitude_edges*self.unit_km
        self.altitude_axis_km = self.altitude_axis*self.unit_km

    def _from_catalogue(self):
        """Every catalogued Output through k_shell (with ``moments``: k_shell_moments, with ``ages``:
        k_shell_ages).  Rows in HBM are read where they are, one launch per run of adjacent slices
        of a store; other Outputs upload their five (seven, six) sample columns.  The sums stay on the device while (aplanet,
        vrplanet) -- the g-values -- stay the same, and are summed on the host across such groups."""
        def set_up(ctx, aplanet, vr_kms):
            ctx.shell_set(self._vr_kms(vr_kms)/self.unit_km, self.quantity, self.lon_edges, self.mu_edges,
                          self.r_edges[0], self.r_edges[-1], self.altitude[2],
                          self.g_tables(aplanet))
            if self.moments:
                ctx.shell_moments_enable()
            if self.ages is not None:
                self._ages_setup = lambda ctx: set_up(ctx, aplanet, vr_kms)
                a_lo, a_hi, nbins = self.ages
                ctx.shell_ages_enable(nbins, float(self.inputs.options.endtime.value), a_lo, a_hi)

        def collect(ctx):
            column, counts, sums = ctx.shell_download()
            self._column_sum += column
            self.packets += counts.astype(float)
            self.shell_sums += sums
            if self.moments:
                self.shell_moment_sums += ctx.shell_moments_download()
            if self.ages is not None:
                self.shell_age_sums += ctx.shell_ages_download()
                self._collected_ages(ctx, 'shell')

        def accumulate(ctx, **samples):
            if self.moments:
                ctx.shell_moments_accumulate(**samples)
            elif self.ages is not None:
                ctx.shell_ages_accumulate(**samples)
            else:
                ctx.shell_accumulate(**samples)

        sample_pass(self, list(self.inputs._catalogue), accumulate,
                    Output.MOMENT_COLS if self.moments else
                    Output.AGE_COLS if self.ages is not None else Output.IMAGE_COLS,
                    set_up, collect, **self._frame_pass())

    def finalize(self):
        """Scale to a source rate of 1e23 atoms/s, as ModelImage.finalize does."""
        self._scale()
        products = shell_from_sums(self._column_sum, self.shell_sums, self.atoms_per_packet,
                                   self.solid_angle, self._volume, self.unit_km*1e5)
        for name, value in products.items():
            setattr(self, name, value)
        if self.moments:
            mass_kg = atomicmass(self.inputs.options.species).value * const.AMU
            vars(self).update(shell_moments_from_sums(
                self.shell_sums, self.shell_moment_sums, self.atoms_per_packet, self._volume,
                self.r_edges, self.unit_km, mass_kg, self.quantity))
        if self.ages is not None:
            vars(self).update(shell_ages_from_sums(
                self.shell_age_sums, self.atoms_per_packet, self.solid_angle, self._volume,
                self.unit_km*1e5, *self.ages[:2]))

    def transient(self, epochs, history):
        """The shell map at ``epochs`` [s] for a source whose rate relative to the nominal one was
        ``history = (t_nodes_s, rate_nodes)`` (transient.response_matrix): a TransientShells with
        epochs, kernel (nbins + 2, E), density (E, nlon, nlat, nalt), column_profile, column (E,
        nlon, nlat), their effective packets and content (E,).  The age block is contracted where
        it is (k_ages_apply) while this object's sums are the ones resident in its context; sums
        that were added on the host (several stretches of g-values) or that another product has
        replaced since are set up again and uploaded once."""
        if self.ages is None:
            raise ValueError('transient() needs an object built with ages=(a_lo_s, a_hi_s, nbins)')
        if not hasattr(self, 'age_edges'):
            raise ValueError('transient() needs the finalized object (finalize())')
        K = response_matrix(self.age_edges, epochs, history)
        if self._ages_setup is None:                       # nothing was ever binned
            sums = np.zeros((2, K.shape[1]) + self.shell_age_sums.shape[1:4] + (2,))
        else:
            sums = self._ages_transient('shell', self._ages_setup, lambda: self.shell_age_sums, K)
        return TransientShells(epochs, K, sums, self.atoms_per_packet, self.solid_angle,
                               self._volume, self.unit_km*1e5, self.quantity)
