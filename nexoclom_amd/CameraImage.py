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
    origin       the planet (default) or a moon among geometry.objects: the rows are moved into the
                 frame that co-rotates with the moon (frames.MoonFrame); observer is then in moon
                 radii from the moon's centre, and the moon is the sphere that occults and shadows

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
with the same velocity (k_camera_cube).  ``ages=(a_lo_s, a_hi_s, nbins)`` adds ModelImage's age
cube (age_sums, age_cube, age_below, age_above, age_edges, age_axis, age_effective_packets;
k_camera_ages) and with it ``transient(epochs, history)``: the camera's images for a source whose
rate changes with time (transient.py).

Not supported, and refused: streaming (``npackets=``), shared runs (``cp=`` / ``shard=``), the
LDS-tile accumulation, fisheye / all-sky projections (a gnomonic camera sees less than 180
degrees), moons as occulters.
"""
import numpy as np

from .ModelImage import ModelImage, ModelResult, parse_cube, refuse_cube_with, refuse_moments_with
from .transient import parse_ages, refuse_ages_of, refuse_ages_with
from .Output import Output
from .catalogue import sample_pass
from .input_classes import InputError

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
    def __init__(self, inputs, params, *, context=None, device=0, moments=False, cube=None,
                 ages=None, **unsupported):
        if ages is not None:
            refuse_ages_with(moments=moments, cube=cube,
                             **{key: unsupported.get(key) for key in ('npackets', 'shard', 'cp')})
            ages = parse_ages(ages)
            refuse_ages_of(inputs)
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
        self._set_origin()          # (npackets=, shard= and cp= are refused above, whatever the origin)
        self._frame()
        self._new_pixel_sums(moments, cube, ages)
        self._ctx, self._device = context, device
        self.counters = {}
        self._from_catalogue()
        self.finalize()

    def _frame(self):
        get = self.params.get
        if str(get('projection', 'gnomonic')).strip().lower() != 'gnomonic':
            raise NotImplementedError(UNSUPPORTED['projection'])
        if 'observer' not in self.params:
            raise InputError('CameraImage.__init__', "params need observer = 'x,y,z' [radii of the "
                             "origin: the planet, or the moon of params['origin']]")
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

    def _from_catalogue(self):
        """Every catalogued Output through k_camera.  Rows in HBM are read where they are, one
        launch per run of adjacent slices of a store; other Outputs upload their five sample
        columns (seven with ``moments`` or ``cube``, through k_camera_moments / k_camera_cube).
        The image stays on the device while (aplanet, vrplanet) -- the g-values -- stay the same,
        and is summed on the host across such groups."""
        velocity = self.moments or self.cube is not None

        def set_up(ctx, aplanet, vr_kms):
            ctx.camera_set(self.observer, self.basis, self._vr_kms(vr_kms)/self.unit_km,
                           self.pix_area_cm2,
                           self.quantity, self.uedges, self.vedges, self.g_tables(aplanet))
            if self.ages is not None:
                self._ages_setup = lambda ctx: set_up(ctx, aplanet, vr_kms)
            self._enable_velocity(ctx, 'camera')

        def accumulate(ctx, **samples):
            (ctx.camera_ages_accumulate if self.ages is not None else
             ctx.camera_cube_accumulate if self.cube is not None else
             ctx.camera_moments_accumulate if self.moments else ctx.camera_accumulate)(**samples)

        sample_pass(self, list(self.inputs._catalogue), accumulate,
                    Output.AGE_COLS if self.ages is not None else
                    Output.MOMENT_COLS if velocity else Output.IMAGE_COLS, set_up,
                    lambda ctx: self._collect_pixels(ctx, 'camera'), **self._frame_pass())

    def finalize(self):
        """Scale to a source rate of 1e23 atoms/s, as ModelImage.finalize does."""
        ModelImage.finalize(self)

    def transient(self, epochs, history):
        """ModelResult.transient on the camera's age block (k_ages_apply)."""
        return ModelResult.transient(self, epochs, history, prefix='camera')
