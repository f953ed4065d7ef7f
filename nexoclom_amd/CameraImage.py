"""CameraImage: what a pinhole camera at a finite distance sees, accumulated on the GPU.

An extension beyond the reference, whose ModelImage looks from infinity (orthographic) and whose
LOSResult sums one narrow cone per spectrum.  ``CameraImage(inputs, params)`` bins every stored
sample of the catalogued Outputs into the perspective (gnomonic) image of a camera at ``observer``:
column density or radiance along each pixel's line of sight, in ModelImage's units and scaling,
with the planet occulting what lies behind it as seen from the camera and, for radiance, the
planet's shadow as in ModelImage.  include/nexoclom_hip.h (nxc_camera_desc) holds the definition
operation by operation; the HIP kernel is k_camera.

``params`` (a dict or a ``key = value`` file, like ModelImage's):

    quantity     'column' or 'radiance'
    observer     'x,y,z'   camera position, planet radii, model frame (required, |o| >= 1)
    boresight    'x,y,z'   viewing direction (default: towards the planet's centre, -observer)
    up           'x,y,z'   which way is up in the image (default '0,0,1'; not parallel to boresight)
    fov          'fx,fz'   full field of view along the image's x and z, degrees, each in (0, 180)
    dims         'nx,nz'   default '256,256'
    g / wavelength         as ModelResult

Attributes: image, packet_image (nx x nz), uedges, vedges (tangent-plane bin edges), basis (rows
right, boresight, up), observer, pixel_solid_angle (nx x nz, sr), totalsource, atoms_per_packet,
sourcerate, counters.  The sample's weight is spread over the footprint of its pixel at the
sample's distance, so a pixel holds (1 / dOmega) * sum weight / r^2 -- the line-of-sight integral
of the density through that pixel.

``moments=True`` adds ModelImage's per-pixel velocity moments (moment_sums, velocity,
velocity_variance, velocity_dispersion, velocity_skewness, effective_packets) in the same pass
(k_camera_moments), with the line-of-sight velocity taken along each sample's own ray from the
camera, positive receding.  ``cube=(v_lo_kms, v_hi_kms, nbins)`` adds ModelImage's velocity cube
(cube_sums, cube, cube_below, cube_above, velocity_edges, velocity_axis, cube_effective_packets)
with the same velocity (k_camera_cube).

Not supported, and refused: streaming (``npackets=``), shared runs (``cp=`` / ``shard=``), the
LDS-tile accumulation, fisheye / all-sky projections (a gnomonic camera sees less than 180
degrees), moons as occulters.
"""
import numpy as np

from .ModelImage import (PIXEL_MOMENT_COLUMNS, ModelResult, cube_from_sums, new_cube_sums, parse_cube,
                         pixel_moments_from_sums, refuse_cube_with, refuse_moments_with)
from .catalogue import sample_spans, shared_context
from .input_classes import InputError
from .units import Quantity

MAX_DIM = 8192
UNSUPPORTED = {
    'npackets': 'streaming (npackets=) is not supported: run the inputs first (Input.run)',
    'cp': 'shared runs (cp=) are not supported by CameraImage',
    'shard': 'shards are not supported by CameraImage',
    'reduce': 'shared runs (cp=) are not supported by CameraImage',
    'tiles': 'the LDS-tile accumulation is ModelImage\'s; CameraImage uses one atomic pair per sample',
    'image_mode': 'the LDS-tile accumulation is ModelImage\'s; CameraImage uses one atomic pair per sample',
    'projection': 'only the gnomonic (pinhole) projection is implemented: no fisheye or all-sky views',
    'moons': 'moons do not occult in CameraImage',
}


def _vector(text, what):
    try:
        parts = [float(v) for v in str(text).split(',')]
    except ValueError:
        parts = []
    if len(parts) != 3 or not np.all(np.isfinite(parts)):
        raise InputError('CameraImage.__init__', f"{what} must be 'x,y,z' (three finite numbers)")
    return np.array(parts)


def _pair(text, convert, what):
    try:
        parts = [convert(v) for v in str(text).split(',')]
    except ValueError:
        parts = []
    if len(parts) != 2:
        raise InputError('CameraImage.__init__', f"{what} must be two numbers 'a,b'")
    return parts


def camera_basis(boresight, up):
    """Rows right, boresight, up of the camera frame (right x boresight = up, the handedness of
    ModelImage's observer frame: x to the right, y along the line of sight, z up)."""
    b = np.asarray(boresight, dtype=float)
    norm = np.linalg.norm(b)
    if not norm > 0:
        raise InputError('CameraImage.__init__', 'boresight must not be the zero vector')
    b = b/norm
    right = np.cross(b, np.asarray(up, dtype=float))
    norm = np.linalg.norm(right)
    if not norm > 1e-8*np.linalg.norm(up):
        raise InputError('CameraImage.__init__', 'up must not be parallel to the boresight')
    right = right/norm
    return np.stack([right, b, np.cross(right, b)])


class CameraImage(ModelResult):
    moments = False           # True: the pass over the rows also fills moment_sums
    cube = None               # (v_lo_kms, v_hi_kms, nbins): the pass also fills cube_sums

    def __init__(self, inputs, params, *, context=None, device=0, moments=False, cube=None,
                 **unsupported):
        if cube is not None:
            refuse_cube_with(moments=moments,
                             **{key: unsupported.get(key) for key in ('npackets', 'shard', 'cp')})
            cube = parse_cube(cube)
        if moments:
            refuse_moments_with(**{key: unsupported.get(key) for key in ('npackets', 'shard', 'cp')})
        for key in unsupported:
            if key in UNSUPPORTED:
                raise NotImplementedError(UNSUPPORTED[key])
            raise TypeError(f'CameraImage() got an unexpected keyword argument {key!r}')
        super().__init__(inputs, params)
        self.type = 'camera image'
        if self.quantity not in ('column', 'radiance'):
            raise InputError('CameraImage.__init__', "quantity must be 'column' or 'radiance'")
        self._frame()
        self.image = np.zeros(self.dims)
        self.packet_image = np.zeros(self.dims)
        self.moments = bool(moments)
        if self.moments:
            self.moment_sums = np.zeros(tuple(self.dims) + (len(PIXEL_MOMENT_COLUMNS),))
        self.cube = cube
        if self.cube is not None:
            self.cube_sums = new_cube_sums(self.dims, self.cube)
        self._ctx, self._device = context, device
        self.counters = {}
        self._from_catalogue()
        self.finalize()

    def _frame(self):
        get = self.params.get
        if str(get('projection', 'gnomonic')).strip().lower() != 'gnomonic':
            raise NotImplementedError(UNSUPPORTED['projection'])
        if get('origin', None) not in (None, self.inputs.geometry.planet):
            raise NotImplementedError('moon-centred camera frames are out of scope')
        if 'observer' not in self.params:
            raise InputError('CameraImage.__init__', "params need observer = 'x,y,z' [planet radii]")
        self.observer = _vector(get('observer'), 'observer')
        if not np.dot(self.observer, self.observer) >= 1.0:
            raise InputError('CameraImage.__init__', 'the observer must be outside the planet (|o| >= 1)')
        boresight = _vector(get('boresight'), 'boresight') if 'boresight' in self.params \
            else -self.observer
        self.basis = camera_basis(boresight, _vector(get('up', '0,0,1'), 'up'))
        if 'fov' not in self.params:
            raise InputError('CameraImage.__init__', "params need fov = 'fx,fz' [degrees]")
        self.fov = _pair(get('fov'), float, 'fov')
        if not all(0.0 < f < 180.0 for f in self.fov):
            raise InputError('CameraImage.__init__', 'each fov angle must be in (0, 180) degrees: '
                             'a pinhole camera has no all-sky view')
        self.dims = _pair(get('dims', '256,256'), int, 'dims')
        if not all(1 <= d <= MAX_DIM for d in self.dims):
            raise InputError('CameraImage.__init__', f'dims must be 1..{MAX_DIM}')
        half = [np.tan(np.radians(f)/2) for f in self.fov]
        self.uedges = np.linspace(-half[0], half[0], self.dims[0] + 1)
        self.vedges = np.linspace(-half[1], half[1], self.dims[1] + 1)
        self.du, self.dv = 2*half[0]/self.dims[0], 2*half[1]/self.dims[1]
        R_cm = self.unit_km*1e5
        self.pix_area_cm2 = self.du*self.dv*R_cm**2
        u = 0.5*(self.uedges[:-1] + self.uedges[1:])
        v = 0.5*(self.vedges[:-1] + self.vedges[1:])
        self.pixel_solid_angle = self.du*self.dv / (1 + u[:, None]**2 + v[None, :]**2)**1.5

    def pixel_boresights(self):
        """Unit vectors (nx, nz, 3), model frame, through the pixel centres: what a
        SpacecraftData / LOSResult cone along the same line of sight would be given."""
        u = 0.5*(self.uedges[:-1] + self.uedges[1:])
        v = 0.5*(self.vedges[:-1] + self.vedges[1:])
        right, bore, up = self.basis
        d = u[:, None, None]*right + bore + v[None, :, None]*up
        return d/np.linalg.norm(d, axis=2, keepdims=True)

    def context(self):
        if self._ctx is None:
            self._ctx = shared_context(self.inputs, self._device)
        return self._ctx

    def _from_catalogue(self):
        """Every catalogued Output through k_camera.  Rows in HBM are read where they are, one
        launch per run of adjacent slices of a store; other Outputs upload their five sample
        columns (seven with ``moments`` or ``cube``, through k_camera_moments / k_camera_cube).
        The image stays on the device while (aplanet, vrplanet) -- the g-values -- stay the same,
        and is summed on the host across such groups."""
        from .Output import Output
        runs = list(self.inputs._catalogue)
        if not runs:
            print('No model outputs found for these inputs.')
            return
        ctx = self.context()
        totals = {}

        def announced():
            for run in runs:
                print(f'Output filename: {getattr(run, "filename", run)}')
                self.totalsource += run.totalsource if isinstance(run, Output) else \
                    float(np.load(run, allow_pickle=False)['totalsource'])
                yield run

        def g_values(run):
            """(aplanet [au], vrplanet [km/s]): what the g-values of a run depend on"""
            if isinstance(run, Output):
                return float(run.aplanet), float(run.vrplanet)
            with np.load(run, allow_pickle=False) as data:
                return float(data['aplanet']), float(data['vrplanet_kms'])

        def collect():
            image, counts = ctx.camera_download()
            self.image += image
            self.packet_image += counts.astype(float)
            if self.moments:
                self.moment_sums += ctx.camera_moments_download()
            if self.cube is not None:
                self.cube_sums += ctx.camera_cube_download()

        velocity = self.moments or self.cube is not None
        accumulate = (ctx.camera_cube_accumulate if self.cube is not None else
                      ctx.camera_moments_accumulate if self.moments else ctx.camera_accumulate)
        is_set = False
        for kind, item in sample_spans(announced(), ctx, key=g_values):
            if kind == 'key':
                if is_set:
                    collect()
                aplanet, vr_kms = item
                ctx.camera_set(self.observer, self.basis, vr_kms/self.unit_km, self.pix_area_cm2,
                               self.quantity, self.uedges, self.vedges, self.g_tables(aplanet))
                if self.moments:
                    ctx.camera_moments_enable()
                if self.cube is not None:
                    v_lo, v_hi, nbins = self.cube
                    ctx.camera_cube_enable(nbins, v_lo/self.unit_km, v_hi/self.unit_km)
                is_set = True
                continue
            if kind == 'rows':
                accumulate(rows=item)
            else:
                samples = Output.image_columns(item, velocity=velocity)[0]
                if samples is None or not len(samples[0]):
                    continue
                names = Output.MOMENT_COLS if velocity else Output.IMAGE_COLS
                accumulate(**dict(zip(names, samples)))
            for key, v in ctx.counters().items():
                totals[key] = totals.get(key, 0) + v
        collect()
        self.counters = totals
        assert totals.get('nonfinite', 0) == 0, 'Non-finite weights'

    def finalize(self):
        """Scale to a source rate of 1e23 atoms/s, as ModelImage.finalize does."""
        per_second = self.totalsource / self.inputs.options.endtime.value
        self.atoms_per_packet = 1e23 / per_second if per_second > 0 else 0.
        self.sourcerate = Quantity(1., '1e23/s')
        if self.moments:         # the quotients are of the unscaled sums
            for name, value in pixel_moments_from_sums(self.image, self.moment_sums,
                                                       self.unit_km).items():
                setattr(self, name, value)
        if self.cube is not None:
            for name, value in cube_from_sums(self.cube_sums, self.atoms_per_packet,
                                              *self.cube[:2]).items():
                setattr(self, name, value)
        self.image *= self.atoms_per_packet
