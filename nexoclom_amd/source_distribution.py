"""Initial packet states X0 on the host, draw-for-draw the reference's sequence.

What a seeded run must reproduce ("Seed parity") is the ORDER in which random
numbers are taken from ``output.randgen`` and the arithmetic that turns them into a state: release
time (variable-step runs only, drawn by Output before anything here) -> sin(latitude) -> longitude
-> speed -> sin(altitude) -> azimuth; each a whole ``npackets`` vector.  The reference spreads
this over initial_state/source_distribution.py:12-283, math/randomdeviates.py:8-83 and
math/distributions.py:7-21; here every kind of source is one small sampler function registered in
a table (``SURFACES``, ``SPEEDS``, ``DIRECTIONS``), and the three entry points the Output calls --
``surface_distribution``, ``speed_distribution``, ``angular_distribution`` -- look the sampler up,
run it and store the columns.  The order of generator calls is asserted by
tests/test_host.py::test_x0_sampling_is_seed_deterministic_and_in_reference_order.

Like the reference, the tabulated-density samplers ('maxwellian', 'sputtering', 'surface spot')
draw from the UNSEEDED process-global ``numpy.random`` (randomdeviates.py:33,63-65), so they are
statistically but not bitwise reproducible; the device sampler (nxc_packets_sample) covers them
with counter-based draws.  A 'maxwellian' at temperature 0 -- thermal speeds at the local surface
temperature, which the reference documents but never wrote -- is the exception: its one draw is a
seeded ``random(npackets)`` vector in the speed slot, where 'flat' draws, so it is reproducible
draw for draw and can be windowed.  So do the sources read from a file, 'surface map' (``mapfile``) and 'user
defined' speeds (``vdistfile``): the file is a SourceMap written by ``SourceMap.save`` (.npz) -- what
``LOSResult.make_source_map`` returns -- not the reference's pickled astropy quantities.

EXTENSION (the reference stops before it): ``SpeedDist.type = surface map`` and ``AngularDist.type =
surface map`` draw a packet's speed, altitude and azimuth from the per-point ``speed_dist_map``,
``altitude_dist_map`` and ``azimuth_dist_map`` of the map its launch point came from.  The joint
density is sum_c w_c A_c p_c over the four corner nodes c of the launch point's cell (w the bilinear
hat weights in (longitude, sin latitude), A the node's abundance, p its normalised 1-D tabulated
law), whose marginal is the launch-point law: given the point, the packet takes ONE corner with
probability w_c A_c / sum w A (``corner_nodes``) and all its per-point draws come from that node's
laws (``random_deviates_1d``'s law, row by row).  Unseeded, like the other map laws.
"""
import os

import numpy as np
import numpy.random as unseeded
from scipy.interpolate import interpn

from . import constants as const
from .input_classes import InputError

TWO_PI = 2*np.pi


# ---- a window of the seeded stream ---------------------------------------------------------------
class WindowGenerator:
    """Rows [a, b) of every ``n``-long uniform draw of ``numpy.random.default_rng(seed)``.

    The reference draws whole vectors, ``randgen.random(npackets)``, one after the other
    (Output.py:138-139; source_distribution.py:51-62,169-171,202-212), and each double consumes
    exactly one 64-bit output of the PCG64 stream: element i of draw j sits at stream position
    j*n + i.  A rank that owns only rows [a, b) of a chunk of n packets therefore jumps there with
    ``PCG64.advance`` (O(log) 128-bit multiplications) instead of drawing -- and discarding -- the
    whole chunk on every rank that overlaps it.  Bit-identical to slicing the full draw
    (tests/test_host.py).  Only ``random`` can be windowed: ``standard_normal`` (ziggurat) uses a
    data-dependent number of outputs, so gaussian sources draw whole chunks (``windowable``)."""

    def __init__(self, seed, n, a, b):
        if seed is None or not 0 <= a <= b <= n:
            raise ValueError('a window needs a seed and 0 <= a <= b <= n')
        self.n, self.a, self.b = int(n), int(a), int(b)
        self._start = np.random.PCG64(seed).state      # = default_rng(seed).bit_generator.state
        self._draws = 0

    def random(self, size):
        assert size == self.b - self.a, 'a windowed generator draws windows of whole vectors'
        engine = np.random.PCG64(0)
        engine.state = self._start
        engine.advance(self._draws*self.n + self.a)
        self._draws += 1
        return np.random.Generator(engine).random(size)

    def standard_normal(self, size):
        raise TypeError('standard_normal cannot be windowed (see WindowGenerator.windowable)')

    @staticmethod
    def windowable(inputs):
        """Whether every seeded draw these inputs make is a ``random(npackets)`` vector."""
        gaussian = inputs.speeddist.type.lower() == 'gaussian' and inputs.speeddist.sigma != 0.
        return not gaussian


class LaunchTable(dict):
    """X0 while it is being drawn: plain arrays by column name.  (Every column inserted into a
    pandas frame costs about a millisecond with the GIL held -- a third of the time it takes to
    draw an Output of 8e4 packets, and what kept several Outputs from being drawn side by side;
    Output builds the frame once, from the finished table.)  Scalars are broadcast like pandas
    broadcasts them."""

    def __init__(self, n):
        super().__init__()
        self.n = int(n)

    def __setitem__(self, name, value):
        column = np.asarray(value)
        if column.ndim == 0:
            column = np.full(self.n, column)
        super().__setitem__(name, column)

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def frame(self, columns):
        import pandas as pd
        return pd.DataFrame({c: self[c] for c in columns}, copy=False)


# ---- geometry helpers ---------------------------------------------------------------------------
def xyz_from_lonlat(lon, lat, isplan, exobase):
    """Surface point of longitude/latitude on the sphere r = exobase, as a (3, n) array
    (source_distribution.py:12-34).  Planet: longitude 0 is the subsolar point (0,-1,0), pi/2 the
    dusk terminator (+x).  Satellite: longitude 0 is the sub-planet point, pi/2 the leading
    point (-x)."""
    handed = 1.0 if isplan else -1.0
    xyz = np.array([handed * exobase * np.sin(lon) * np.cos(lat),
                    -exobase * np.cos(lon) * np.cos(lat),
                    exobase * np.sin(lat)])
    assert np.all(np.isfinite(xyz)), 'Non-Finite values of X0'
    return xyz


def _unit_rows(vectors):
    return vectors/np.linalg.norm(vectors, axis=1)[:, np.newaxis]


def local_frame(x, y, z):
    """Unit vectors (radial, east, north), each (n, 3), of the launch points."""
    nothing = np.zeros_like(z)
    radial = np.array([x, y, z]).transpose()
    east = np.array([y, -x, nothing]).transpose()
    north = np.array([-z*x, -z*y, x**2+y**2]).transpose()
    return _unit_rows(radial), _unit_rows(east), _unit_rows(north)


def _unit_columns(a, b, c):
    """(a, b, c)/|(a, b, c)| component by component.  The norm is formed like np.linalg.norm
    forms it for the rows of an (n, 3) array -- sqrt((a*a + b*b) + c*c) -- so the columns carry
    the bits `_unit_rows` would give, without the strided (n, 3) temporaries."""
    length = np.sqrt((a*a + b*b) + c*c)
    return a/length, b/length, c/length


def local_frame_columns(x, y, z):
    """`local_frame` as three tuples of 1-D arrays (bit-identical components)."""
    return (_unit_columns(x, y, z), _unit_columns(y, -x, np.zeros_like(z)),
            _unit_columns(-z*x, -z*y, x**2+y**2))


def _ascending(first, second):
    """An angular range that runs through 2 pi is unwrapped so that it ascends."""
    return (first, second) if first <= second else (first, second + TWO_PI)


# ---- densities and deviates (global generator) ------------------------------------------------
def _mass_kg(species):
    return const.ATOMIC_MASS[species] * const.AMU


def sputdist(velocity, U_eV, alpha, beta, species):
    """Sputtering flux density over velocity [km/s], peak-normalised (distributions.py:7-13):
    v^(2 beta + 1) / (v^2 + v_b^2)^alpha with v_b the speed of binding energy U."""
    v_b = np.sqrt(2*U_eV*const.EV/_mass_kg(species)) / 1e3
    density = velocity**(2*beta+1) / (velocity**2 + v_b**2)**alpha
    return density / np.max(density)


def MaxwellianDist(velocity, temperature, species):
    """Maxwellian FLUX density over velocity [km/s], peak-normalised (distributions.py:16-21)."""
    vth2 = 2*temperature*const.K_B/_mass_kg(species) / 1e6
    density = velocity**3 * np.exp(-velocity**2/vth2)
    return density / np.max(density)


def density_cdf(x, f_x):
    """(cdf, grid) of a density tabulated on x: running sum shifted to start at 0 and scaled to
    end at 1, on an even grid over x's range (randomdeviates.py:29-32)."""
    grid = np.linspace(x.min(), x.max(), f_x.shape[0])
    cdf = f_x.cumsum()
    cdf -= cdf.min()
    cdf /= cdf.max()
    return cdf, grid


def random_deviates_1d(x, f_x, num):
    """Inverse-CDF deviates of the density f_x tabulated on x (randomdeviates.py:8-33)."""
    cdf, grid = density_cdf(x, f_x)
    return np.interp(unseeded.rand(num), cdf, grid)


def random_deviates_2d(fdist, x0, y0, num):
    """Accept/reject deviates of a density map on (x0, y0): rounds of ``num`` candidate points
    under a box of height max(fdist) until ``num`` are accepted (randomdeviates.py:36-83)."""
    span_x, span_y = x0.max() - x0.min(), y0.max() - y0.min()
    ceiling = fdist.max()
    axes = (np.linspace(x0.min(), x0.max(), fdist.shape[0]),
            np.linspace(y0.min(), y0.max(), fdist.shape[1]))
    kept_x, kept_y = [], []
    while len(kept_x) < num:
        cand_x = unseeded.rand(num)*span_x + x0.min()
        cand_y = unseeded.rand(num)*span_y + y0.min()
        height = unseeded.rand(num)*ceiling
        under = height < interpn(axes, fdist, (cand_x, cand_y))
        kept_x.extend(cand_x[under])
        kept_y.extend(cand_y[under])
    return np.array(kept_x[:num]), np.array(kept_y[:num])


# ---- where packets start: (lon, lat) ------------------------------------------------------------
def spot_density_map(lon0, lat0, sigma):
    """exp(-angular distance / sigma) from the spot centre on a 1-degree (lon, lat) grid
    (source_distribution.py:96-113; the reference's map uses -sin(lat) for z, kept)."""
    centre = (np.sin(lon0)*np.cos(lat0), -np.cos(lon0)*np.cos(lat0), np.sin(lat0))
    lon = np.linspace(0, TWO_PI, 361)
    lat = np.linspace(-np.pi/2, np.pi/2, 181)
    cosine = (np.outer(np.sin(lon), np.cos(lat))*centre[0]
              + -np.outer(np.cos(lon), np.cos(lat))*centre[1]
              + -np.outer(np.ones_like(lon), np.sin(lat))*centre[2])
    return lon, lat, np.exp(-np.arccos(np.clip(cosine, -1, 1))/sigma)


def _surface_uniform(out, sd):
    n, rng = out.npackets, out.randgen
    s0, s1 = np.sin(sd.latitude[0]), np.sin(sd.latitude[1])
    lat = np.arcsin(s0 + (s1-s0) * rng.random(n))
    w0, w1 = _ascending(float(sd.longitude[0]), float(sd.longitude[1]))
    lon = (w0 + (w1-w0) * rng.random(n)) % TWO_PI
    return lon, lat


def _surface_spot(out, sd):
    lon, lat, density = spot_density_map(float(sd.longitude), float(sd.latitude),
                                         float(sd.sigma))
    return random_deviates_2d(density, lon, lat, out.npackets)


def source_file(parameter, path):
    """The SourceMap file an input parameter (``mapfile``, ``vdistfile``) names.  'default' stands
    for data files the reference does not ship either; a file that is not there is an InputError
    (source_distribution.py:173-176)."""
    from .sourcemap import SourceMap
    if path == 'default':
        raise InputError(parameter, f'{parameter} = default: there is no default file; name an '
                                    '.npz written by SourceMap.save')
    if not os.path.exists(path):
        raise InputError(parameter, f'{path} not found.')
    return SourceMap(path)


def _first_bad(values):
    """Index (as a tuple) and value of the first entry that is not a finite number >= 0."""
    bad = np.argwhere(~(np.isfinite(values) & (values >= 0)))
    return (None, None) if len(bad) == 0 else (tuple(int(k) for k in bad[0]), values[tuple(bad[0])])


def surface_map_density(sd, smap=None):
    """(longitude, latitude or None, abundance, coordinate_system) of ``spatialdist.mapfile``
    (``smap``: the file, where it has been read already), or
    the reason it cannot be launched from.  The reference's rejection loop would not end on a map
    without positive entries and draws nonsense from negative or non-finite ones
    (math/randomdeviates.py:59-78): those are ValueErrors here.  Planet-fixed maps are refused as
    in the reference (source_distribution.py:85-93)."""
    if smap is None:
        smap = source_file('mapfile', sd.mapfile)
    if smap.abundance is None or smap.longitude is None:
        raise ValueError(f'{sd.mapfile} holds no abundance map')
    abundance = np.asarray(smap.abundance, dtype=np.float64)
    longitude = np.asarray(smap.longitude, dtype=np.float64)
    latitude = None if smap.latitude is None else np.asarray(smap.latitude, dtype=np.float64)
    shape = (len(longitude),) if latitude is None else (len(longitude), len(latitude))
    if abundance.shape != shape or min(shape) < 2:
        raise ValueError(f'{sd.mapfile}: abundance{abundance.shape} does not fit its axes {shape} '
                         '(at least two nodes each)')
    where, value = _first_bad(abundance)
    if where is not None:
        raise ValueError(f'{sd.mapfile}: abundance{list(where)} = {value}; a source map must be '
                         'finite and >= 0 (make_source_map gives inf where no packet of a grid '
                         "point's ball was observed)")
    if not abundance.max() > 0:
        raise ValueError(f'{sd.mapfile}: abundance is zero everywhere')
    if 'planet' in smap.coordinate_system:
        if sd.subsolarlon is None:
            raise ValueError('inputs.spatialdist.subsolarlon is None')
        raise NotImplementedError('planet-fixed source maps: the reference stops here as well '
                                  "('Need to verify this works')")
    return longitude, latitude, abundance, smap.coordinate_system


def speed_file_density(vd):
    """(speed [km/s], speed_dist) of ``speeddist.vdistfile``."""
    smap = source_file('vdistfile', vd.vdistfile)
    if smap.speed is None or smap.speed_dist is None:
        raise ValueError(f'{vd.vdistfile} holds no speed distribution')
    speed = np.asarray(smap.speed, dtype=np.float64)
    density = np.asarray(smap.speed_dist, dtype=np.float64)
    if speed.ndim != 1 or speed.shape != density.shape or len(speed) < 2:
        raise ValueError(f'{vd.vdistfile}: speed and speed_dist must be 1-D and equally long')
    where, value = _first_bad(density)
    if where is not None or not np.all(np.isfinite(speed)):
        raise ValueError(f'{vd.vdistfile}: speed_dist{list(where or ())} = {value}; speed and '
                         'speed_dist must be finite, speed_dist >= 0')
    if not density.max() > 0:
        raise ValueError(f'{vd.vdistfile}: speed_dist is zero everywhere')
    return speed, density


def surface_map_cells(longitude, latitude, abundance):
    """What the device draws a 2-D map's launch points from (k_sample, spatial_type 2).  The law
    random_deviates_2d samples has its density proportional to the bilinear interpolant of
    ``abundance`` on the even node grid linspace(lon) x linspace(sin lat); the mass of a cell of
    that grid is its area (the same for all) times the mean of its four corners.  Returns the
    cumulated corner sums (a + b) + (c + d), lon-major, divided by their total, and the limits
    (lon0, lon1, s0, s1) of the two axes."""
    s = np.sin(latitude)
    corners = (abundance[:-1, :-1] + abundance[:-1, 1:]) + (abundance[1:, :-1] + abundance[1:, 1:])
    cdf = np.cumsum(corners.ravel())
    cdf /= cdf[-1]
    return cdf, (float(longitude.min()), float(longitude.max()), float(s.min()), float(s.max()))


# ---- per-point laws of a source map ------------------------------------------------------------------
NODE_LAWS = {'speed': 'speed_dist_map', 'altitude': 'altitude_dist_map',
             'azimuth': 'azimuth_dist_map'}


_NODE_LAWS_OF = {}       # the last map file's: {'stamp', 'map', 'density', law: (table, grid)}


def _node_laws_of(sd):
    """What `node_law_tables` keeps of ``spatialdist.mapfile``: the file as read once, its
    checked abundance, and the tables made from it so far.  One file at a time (a default map's
    tables take 22 MB); a file that changed on disk is read again."""
    path = os.path.abspath(sd.mapfile)
    stamp = None
    if os.path.exists(path):
        stat = os.stat(path)
        stamp = (path, stat.st_mtime_ns, stat.st_size)
    if stamp is None or _NODE_LAWS_OF.get('stamp') != stamp:
        _NODE_LAWS_OF.clear()
        smap = source_file('mapfile', sd.mapfile)
        _NODE_LAWS_OF.update(map=smap, density=surface_map_density(sd, smap), stamp=stamp)
    return _NODE_LAWS_OF


def node_law_tables(sd, law):
    """(cdf [nlon * nlat, n], grid [n]) of one per-point law (``law``: a key of NODE_LAWS) of
    ``spatialdist.mapfile``: row c = i_lon * nlat + j_lat holds density_cdf of node c's row of the
    *_dist_map, ``grid`` the even axis all rows share -- what random_deviates_1d interpolates in.
    The speed axis is the file's ``speed``; the angle axes are rebuilt from the map's last
    dimension (the centres of linspace(0, pi/2 | 2 pi, n + 1)), since a normalised map overwrites
    ``altitude`` / ``azimuth`` with distributions (sourcemap.py).  Rows of nodes without abundance
    are never drawn from (make_source_map(normalize=True) leaves NaN there): they become rows of
    zeros.  Any other row must be finite, >= 0 and not all zero -- beyond its first entry, whose
    mass density_cdf drops; else ValueError naming file, array and node.
    The file is read once for all three laws, and the tables (read-only arrays) are kept until
    another file is asked for or this one changes: every chunk of a run asks for them again."""
    kept = _node_laws_of(sd)
    if law not in kept:
        kept[law] = _node_law_table(sd.mapfile, kept['map'], kept['density'], law)
    return kept[law]


def _node_law_table(path, smap, density, law):
    from .sourcemap import centres
    name = NODE_LAWS[law]
    _, latitude, abundance, _ = density
    if latitude is None:
        raise ValueError(f'{path}: {name} launches need a 2-D map (longitude and latitude); this '
                         'one has no latitudes')
    values = getattr(smap, name)
    if values is None:
        raise ValueError(f'{path} holds no {name}')
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3 or values.shape[:2] != abundance.shape:
        raise ValueError(f'{path}: {name}{values.shape} does not fit abundance{abundance.shape}: '
                         'its leading dimensions must be the map\'s')
    n = values.shape[2]
    if law == 'speed':
        axis = None if smap.speed is None else np.asarray(smap.speed, dtype=np.float64)
        if axis is None or axis.ndim != 1 or len(axis) != n or n < 2 \
                or not np.all(np.isfinite(axis)):
            raise ValueError(f'{path}: speed must be 1-D, finite and as long as the last dimension '
                             f'of speed_dist_map{values.shape} (at least 2)')
    else:
        if n < 2:
            raise ValueError(f'{path}: {name}{values.shape} needs at least 2 bins')
        axis = centres(np.linspace(0, np.pi/2 if law == 'altitude' else TWO_PI, n + 1))
    live = abundance > 0
    rows = values[live]
    where, value = _first_bad(rows)
    if where is not None:
        i, j = (int(k) for k in np.argwhere(live)[where[0]])
        raise ValueError(f'{path}: {name}[{i}, {j}, {where[1]}] = {value}; the law of a node with '
                         'abundance > 0 must be finite and >= 0')
    cdf = rows.cumsum(axis=1)
    cdf -= cdf[:, :1].copy()
    empty = np.flatnonzero(~(cdf[:, -1] > 0))
    if len(empty):
        i, j = (int(k) for k in np.argwhere(live)[empty[0]])
        raise ValueError(f'{path}: {name}[{i}, {j}] is zero everywhere (beyond its first entry, '
                         'whose mass the tabulated law drops) at a node with abundance > 0')
    cdf /= cdf[:, -1:].copy()
    table = np.zeros((abundance.size, n))
    table[live.ravel()] = cdf
    grid = np.linspace(axis.min(), axis.max(), n)
    table.setflags(write=False)
    grid.setflags(write=False)
    return table, grid


def corner_nodes(abundance, i, j, tx, ty, u):
    """The node (i_lon * nlat + j_lat) each packet's per-point laws come from: a corner of its
    cell (i, j), in the order (i, j), (i, j+1), (i+1, j), (i+1, j+1) with weights (1-tx)(1-ty) a,
    (1-tx) ty b, tx (1-ty) c, tx ty d -- the first whose running sum exceeds u * total; the last
    with a positive weight if rounding leaves none; the corner with the largest abundance where the
    total is not > 0 (a point on a zero edge of its cell)."""
    a, b, c, d = abundance[i, j], abundance[i, j + 1], abundance[i + 1, j], abundance[i + 1, j + 1]
    w = np.array([(1.0 - tx)*(1.0 - ty)*a, (1.0 - tx)*ty*b, tx*(1.0 - ty)*c, tx*ty*d])
    running = np.cumsum(w, axis=0)
    total = running[3]
    over = running > u*total
    first = np.argmax(over, axis=0)
    last_positive = 3 - np.argmax(w[::-1] > 0, axis=0)
    k = np.where(over.any(axis=0), first, last_positive)
    k = np.where(total > 0, k, np.argmax(np.array([a, b, c, d]), axis=0))
    return (i + (k >> 1))*abundance.shape[1] + (j + (k & 1))


def node_deviates(cdf, grid, node, u):
    """np.interp(u, cdf[node], grid) packet by packet: random_deviates_1d's inversion on each
    packet's own row of a per-node cdf table."""
    order = np.argsort(node, kind='stable')
    ranked = node[order]
    starts = np.flatnonzero(np.r_[True, ranked[1:] != ranked[:-1]])
    out = np.empty(len(node))
    for first, last in zip(starts, np.r_[starts[1:], len(node)]):
        rows = order[first:last]
        out[rows] = np.interp(u[rows], cdf[ranked[first]], grid)
    return out


def _map_law_nodes(out):
    """The corner node of every packet of ``out``, drawn once (one corner serves all of a packet's
    per-point draws): cell and in-cell coordinates of the launch points already in X0 on the map's
    even node grid in (longitude, sin latitude), then `corner_nodes`."""
    if getattr(out, '_map_nodes', None) is None:
        sd = out.inputs.spatialdist
        longitude, latitude, abundance, _ = _node_laws_of(sd)['density']
        if latitude is None:
            raise ValueError(f'{sd.mapfile}: per-point laws need a 2-D map (longitude and latitude)')
        _, (lon0, lon1, s0, s1) = surface_map_cells(longitude, latitude, abundance)
        nlon, nlat = abundance.shape
        gx = (np.asarray(out.X0['longitude']) - lon0)/((lon1 - lon0)/(nlon - 1))
        gy = (np.sin(np.asarray(out.X0['latitude'])) - s0)/((s1 - s0)/(nlat - 1))
        i = np.clip(np.floor(gx), 0, nlon - 2).astype(np.int64)
        j = np.clip(np.floor(gy), 0, nlat - 2).astype(np.int64)
        tx, ty = np.clip(gx - i, 0.0, 1.0), np.clip(gy - j, 0.0, 1.0)
        out._map_nodes = corner_nodes(abundance, i, j, tx, ty, unseeded.rand(out.npackets))
    return out._map_nodes


def _surface_map(out, sd):
    longitude, latitude, abundance, system = surface_map_density(sd)
    out.inputs.spatialdist.coordinate_system = system                      # :71
    if latitude is None:
        return random_deviates_1d(longitude, abundance, out.npackets), np.zeros(out.npackets)
    lon, s = random_deviates_2d(abundance, longitude, np.sin(latitude), out.npackets)
    return lon, np.arcsin(s)


SURFACES = {'uniform': _surface_uniform, 'surface spot': _surface_spot,
            'surface map': _surface_map}


def surface_distribution(outputs):
    """Columns x, y, z, longitude, latitude, local_time of X0 (source_distribution.py:37-134)."""
    sd = outputs.inputs.spatialdist
    assert sd.type in SURFACES, "Can't get here"
    lon, lat = SURFACES[sd.type](outputs, sd)
    # The reference always uses the planet convention (:126).  With a moon as start point (our
    # extension) the satellite convention of xyz_from_lonlat applies.
    geo = outputs.inputs.geometry
    x, y, z = xyz_from_lonlat(lon, lat, geo.planet.object == geo.startpoint, sd.exobase)
    X0 = outputs.X0
    X0['x'], X0['y'], X0['z'] = x, y, z
    X0['longitude'], X0['latitude'] = lon, lat
    X0['local_time'] = (lon * 12/np.pi + 12) % 24


# ---- how fast: speed in km/s --------------------------------------------------------------------
def _speed_gaussian(out, vd, species):
    if vd.sigma == 0.:
        return np.zeros(out.npackets) + vd.vprob.value
    return out.randgen.standard_normal(out.npackets) * vd.sigma.value + vd.vprob.value


def _speed_flat(out, vd, species):
    return out.randgen.random(out.npackets)*2*vd.delv.value + vd.vprob.value - vd.delv.value


def tabulated_speed_density(vd, species):
    """(velocity grid [km/s], flux density) of the 'sputtering' and 'maxwellian' speed
    distributions on the reference's 5000-point grids (source_distribution.py:148-168)."""
    if vd.type == 'sputtering':
        grid = np.linspace(.1, 50, 5000)
        return grid, sputdist(grid, vd.U.value, vd.alpha, vd.beta, species)
    assert vd.type == 'maxwellian' and vd.temperature != 0, 'Not implemented yet'
    v_th = np.sqrt(2*vd.temperature.value*const.K_B/_mass_kg(species)) / 1e3
    grid = np.linspace(0.1, v_th*5, 5000)
    return grid, MaxwellianDist(grid, vd.temperature.value, species)


def _speed_tabulated(out, vd, species):
    return random_deviates_1d(*tabulated_speed_density(vd, species), out.npackets)


def thermal_source(inputs):
    """Whether the launch speeds are thermal: 'maxwellian' at temperature 0, a Maxwellian flux at
    the local surface temperature (what the reference documents but stops at, :165-168)."""
    vd = inputs.speeddist
    return vd.type == 'maxwellian' and vd.temperature == 0


def _speed_thermal(out, vd, species):
    """The speed below which a fraction u of a Maxwellian flux at the launch point's surface
    temperature leaves the surface: v = max(S(T, u), 0) with S the v(T, p) spline of thermally
    accommodated re-emission (surface.tabulate_thermal_speeds; bouncepackets.py:71-74 draws from
    it the same way), T from the longitude / latitude already drawn, u one seeded vector in the
    speed slot.  The clamp matters only at u = 0, where S is a few 1e-18 below zero at some T."""
    from .surface import surface_temperature, thermal_launch_spline
    spline = thermal_launch_spline(out.inputs)
    temperature = surface_temperature(out.inputs.geometry, out.X0['longitude'],
                                      out.X0['latitude'])
    return np.maximum(spline.ev(temperature, out.randgen.random(out.npackets)), 0.0)


def _speed_maxwellian(out, vd, species):
    if thermal_source(out.inputs):
        return _speed_thermal(out, vd, species)
    return _speed_tabulated(out, vd, species)


def _speed_from_file(out, vd, species):
    return random_deviates_1d(*speed_file_density(vd), out.npackets)


def _speed_from_map(out, vd, species):
    cdf, grid = node_law_tables(out.inputs.spatialdist, 'speed')
    return node_deviates(cdf, grid, _map_law_nodes(out), unseeded.rand(out.npackets))


SPEEDS = {'gaussian': _speed_gaussian, 'flat': _speed_flat, 'sputtering': _speed_tabulated,
          'maxwellian': _speed_maxwellian, 'user defined': _speed_from_file,
          'surface map': _speed_from_map}


def speed_distribution(outputs):
    """Column v of X0, in R/s (source_distribution.py:137-189)."""
    vd = outputs.inputs.speeddist
    kind = vd.type.lower() if vd.type.lower() == 'gaussian' else vd.type
    assert kind in SPEEDS, 'Distribtuion does not exist'
    v0 = SPEEDS[kind](outputs, vd, outputs.inputs.options.species) / outputs.unit_km
    outputs.X0['v'] = v0
    assert np.all(np.isfinite(v0)), 'Infinite values for v0'
    return v0


# ---- which way: altitude above the local horizon, azimuth from north through east ---------------
def _direction_radial(out, ad):
    n = out.npackets
    return np.zeros(n) + np.pi/2., np.zeros(n)


def _direction_isotropic(out, ad):
    n, rng = out.npackets, out.randgen
    s0, s1 = np.sin(ad.altitude[0]), np.sin(ad.altitude[1])
    alt = np.arcsin(rng.random(n) * (s1 - s0) + s0)
    a0, a1 = float(ad.azimuth[0]), float(ad.azimuth[1])
    lo, hi = (a0, a1) if a0 <= a1 else (a1, a0 + TWO_PI)     # the reference's unwrap (:209)
    return alt, lo + (hi-lo)*rng.random(n)


def _direction_planar(out, ad):
    c0, c1 = np.cos(ad.altitude[0]), np.cos(ad.altitude[1])
    return np.arccos(out.randgen.random(out.npackets) * (c1 - c0) + c0), None


def _direction_from_map(out, ad):
    nodes, n = _map_law_nodes(out), out.npackets
    return tuple(node_deviates(*node_law_tables(out.inputs.spatialdist, law), nodes,
                               unseeded.rand(n)) for law in ('altitude', 'azimuth'))


DIRECTIONS = {'radial': _direction_radial, 'isotropic': _direction_isotropic,
              '2d': _direction_planar, 'surface map': _direction_from_map}


def angular_distribution(outputs):
    """Columns vx, vy, vz, altitude, azimuth of X0 (source_distribution.py:192-283): the speed
    along (cos alt cos az) north + (cos alt sin az) east + (sin alt) radial; for '2d' sources the
    motion stays in the equatorial plane."""
    ad = outputs.inputs.angulardist
    if ad.type == 'none':
        return
    assert ad.type in DIRECTIONS, 'Angular Distribution not defined.'
    alt, az = DIRECTIONS[ad.type](outputs, ad)
    X0 = outputs.X0
    x, y, z = (np.asarray(X0[c]) for c in ('x', 'y', 'z'))
    speed = np.asarray(X0['v'])
    up, level = np.sin(alt), np.cos(alt)
    if ad.type == '2d':
        outward = _unit_rows(np.array([x, y]).transpose())
        along = _unit_rows(np.array([y, -x]).transpose())
        heading = level[:, np.newaxis]*along + up[:, np.newaxis]*outward
        assert np.all(np.isclose(np.sum(heading**2, axis=1), 1))
        X0['vx'], X0['vy'] = heading[:, 0] * speed, heading[:, 1] * speed
        X0['vz'] = np.zeros((outputs.npackets, ))
        X0['altitude'], X0['azimuth'] = alt, 0
        X0['v_radial'] = up * X0['v']
        X0['v_east'] = np.sqrt(X0['v']**2 - X0['v_radial']**2)
        X0['v_north'] = 0
        return
    radial, east, north = local_frame_columns(x, y, z)
    to_north, to_east = level * np.cos(az), level * np.sin(az)
    for name, r, e, n in zip(('vx', 'vy', 'vz'), radial, east, north):
        X0[name] = ((to_north*n + to_east*e) + up*r) * speed
    X0['altitude'], X0['azimuth'] = alt, az
