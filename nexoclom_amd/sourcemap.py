"""sourcemap: where on the surface the packets of a (fitted) result came from, built on the GPU.

Drop-in for data_simulation/make_source_map.py:11-174 and LOSResult.make_source_map
(data_simulation/LOSResult.py:310-458) of the reference, and the attributes of its
initial_state/SourceMap.py.  ``LOSResult.make_source_map`` drives it; this module holds the grid,
the packet bucketing, the combination across Outputs and the normalisation.

Per Output (X0 columns longitude, latitude, v, altitude, azimuth, frac as float64, the way
Output.restore gives them): vmax = ceil(max(v over ALL X0) * R_km); included = frac > 0; weight =
frac ('source') or 1 ('available').  Grid points are the centres of np.histogram2d's bins on
[0, 2 pi] x [-pi/2, pi/2], point p = i_lon * nlat + j_lat.  Packet q is in point p's ball (sklearn
BallTree haversine ``query_radius`` with radius r_p = smear_radius * cos(phi_p)) iff
    sin(0.5*(phi_p - phi_q))**2 + cos(phi_p)*cos(phi_q)*sin(0.5*(lam_p - lam_q))**2
        <= sin(0.5*r_p)**2,
over ALL X0 packets.  Per point: n_total, n_included, the weight sum over the ball (the smeared
abundance) and the speed (v * R_km on [0, vmax]), altitude ([0, pi/2]) and azimuth ([0, 2 pi])
histograms of the included packets of the ball.  Binning is np.histogram's with ``range=``
(linspace edges, right edge inclusive, values outside dropped); on the device it is
nxc_device.hpp's bin_index, the image's binning.  The HIP kernels (nxc_kernels.hpp, k_smap_*) do
the bucketed walk, the membership test and every histogram; the host only sorts the packets by
grid cell and lists each tile's candidate cells.

Quirks of the reference kept as written:
  * the global speed axis is the largest vmax's; an Output whose speed axis ends where the global
    one does adds speed_dist and speed_dist_map TWICE (LOSResult.py:356-363);
  * every other Output adds its raw speed histograms (on its own axis) once, plus np.interp onto the
    global axis -- and the interp of EVERY grid point's speed histogram goes to EVERY grid point
    (the broadcast in the i, j loop, :364-371).  np.interp is linear in its values, so that sum is
    computed as one interp of the Output's speed map summed over the grid;
  * fraction_observed = n_included / n_total, NaN -> 1 for the division of abundance, then 0;
    abundance NaN -> 0 (:377-385); a point with n_included = 0 < n_total and a non-zero
    abundance_uncor gets an infinite abundance, as in the reference;
  * under ``normalize`` the AXES ``altitude`` and ``azimuth`` are overwritten with normalised values
    while altitude_dist / azimuth_dist stay raw (:432-447); the *_dist_map normalisations divide by
    per-point sums and give NaN where such a sum is 0.

Deviations: Outputs with no X0 packet are skipped (the reference fails on ceil(NaN)); Outputs
whose X0 was not kept (device sampler) raise NotImplementedError; the two speed adds of a
max-vmax Output are one add of twice the value on the device (same value to one rounding); the
LDS sums are not in a fixed order (weighted sums agree to rounding, counts exactly).

Files: ``SourceMap.save(path)`` writes an .npz of plain float64 arrays and strings, ``SourceMap(path)``
reads it back exactly; that file is what ``spatialdist.mapfile`` / ``speeddist.vdistfile`` of an
input file name (source_distribution.py launches packets from it).  The reference's .pkl / .sav
files hold pickled astropy quantities and stay out of scope.

Units (``SourceMap.units``): the arrays are plain float64; with ``normalize`` abundance and
abundance_uncor are in '1/(cm2 s)', speed_dist in '1/(km/s)/s', speed_dist_map in
'1/(cm2 s)/(km/s)', altitude and azimuth in '1/(s rad)', the altitude / azimuth maps in
'1/(cm2 s rad)'; longitude, latitude, altitude and azimuth axes in 'rad' and speed in 'km/s'
before that.  Without ``normalize`` the histograms are unitless, as in the reference.
"""
import math
import os

import numpy as np

DEFAULTS = dict(smear_radius=np.radians(10), nlonbins=180, nlatbins=90, nvelbins=100,
                nazbins=45, naltbins=23, smear_abundance=True)
TILE_LDS_BYTES = 32768            # LDS budget of a tile's histograms (k_smap_points)
MAX_TILE = 16


def centres(edges):
    """math/histogram.py's axis: edges[:-1] + dx/2 with dx = edges[1] - edges[0]."""
    return edges[:-1] + (edges[1] - edges[0])/2


def speed_edges(vmax, nvel):
    return np.linspace(0, vmax, nvel + 1)


class SourceMapGrid:
    """The grid of make_source_map.py:40-49,77-83 with what the kernels need: edges, point
    centres, cos(phi_p) and thresholds per latitude row, and the candidate cells of every tile of
    ``tile`` consecutive longitudes of one latitude row (runs [seg[s, 0], seg[s, 1]] of lat-major
    cells j * nlon + i, tile k's runs seg_off[k] .. seg_off[k + 1] - 1)."""

    def __init__(self, grid_params=None, r_km=1.0):
        p = dict(DEFAULTS)
        p.update(grid_params or {})
        self.params = p
        self.smear_radius = float(p['smear_radius'])
        self.nlon, self.nlat = int(p['nlonbins']), int(p['nlatbins'])
        self.nvel, self.nalt, self.naz = int(p['nvelbins']), int(p['naltbins']), int(p['nazbins'])
        self.smear_abundance = bool(p['smear_abundance'])
        self.r_km = float(r_km)
        self.lon_edges = np.linspace(0, 2*np.pi, self.nlon + 1)
        self.lat_edges = np.linspace(-np.pi/2, np.pi/2, self.nlat + 1)
        self.alt_edges = np.linspace(0, np.pi/2, self.nalt + 1)
        self.az_edges = np.linspace(0, 2*np.pi, self.naz + 1)
        self.lon, self.lat = centres(self.lon_edges), centres(self.lat_edges)
        self.altitude, self.azimuth = centres(self.alt_edges), centres(self.az_edges)
        self.cos_lat = np.cos(self.lat)
        self.radius = self.smear_radius*np.cos(self.lat)          # r_p per latitude row
        self.threshold = np.sin(0.5*self.radius)**2
        stride = self.nvel + self.nalt + self.naz + 3
        self.tile = max(1, min(MAX_TILE, self.nlon, TILE_LDS_BYTES // (8*stride)))
        self._segments()

    @property
    def npoints(self):
        return self.nlon*self.nlat

    def _segments(self):
        nlon, nlat, T = self.nlon, self.nlat, self.tile
        dlon = self.lon_edges[1] - self.lon_edges[0]
        dlat = self.lat_edges[1] - self.lat_edges[0]
        tpr = -(-nlon // T)
        seg, seg_off = [], [0]
        for j in range(nlat):
            phi, r = self.lat[j], abs(self.radius[j])*(1 + 1e-6) + 1e-9
            if r >= np.pi:
                rows, width = range(nlat), None
            else:
                jlo = max(0, int(math.floor((phi - r + np.pi/2)/dlat)) - 1)
                jhi = min(nlat - 1, int(math.floor((phi + r + np.pi/2)/dlat)) + 1)
                rows = range(jlo, jhi + 1)
                # |dlam| bound over the band: cos(phi_p) cos(phi_q) sin^2(dlam/2) <= threshold
                top = min(np.pi/2, max(abs(phi - r), abs(phi + r)))
                cmin = 0.0 if top >= np.pi/2 else math.cos(top)
                den = self.cos_lat[j]*cmin
                ratio = self.threshold[j]*(1 + 1e-6)/den if den > 0 else np.inf
                width = None if ratio >= 1 else 2*math.asin(math.sqrt(ratio))*(1 + 1e-6) + 1e-9
            for k in range(tpr):
                i0, i1 = k*T, min(k*T + T, nlon) - 1
                if width is None:
                    c0, c1 = 0, nlon - 1
                else:
                    c0 = int(math.floor((self.lon[i0] - width)/dlon)) - 1
                    c1 = int(math.floor((self.lon[i1] + width)/dlon)) + 1
                    if c1 - c0 + 1 >= nlon:
                        c0, c1 = 0, nlon - 1
                for jj in rows:
                    base = jj*nlon
                    if c0 >= 0 and c1 < nlon:
                        seg.append((base + c0, base + c1))
                    else:
                        a = c0 % nlon
                        n = c1 - c0 + 1
                        if a + n <= nlon:
                            seg.append((base + a, base + a + n - 1))
                        else:
                            seg.append((base + a, base + nlon - 1))
                            seg.append((base, base + a + n - 1 - nlon))
                seg_off.append(len(seg))
        self.seg = np.asarray(seg, dtype=np.int32).reshape(-1, 2)
        self.seg_off = np.asarray(seg_off, dtype=np.int32)

    def bucket(self, lat, lon):
        """(order, cell_start): the packets stably sorted by lat-major cell (i = floor(mod(lon,
        2 pi) / dlon), j = floor((lat + pi/2) / dlat), clamped to the grid; a packet with a
        non-finite lat or lon goes after the last cell).  The cells only prune the walk: the
        tiles' runs are one cell wider than the balls on every side."""
        dlon = self.lon_edges[1] - self.lon_edges[0]
        dlat = self.lat_edges[1] - self.lat_edges[0]
        ncells = self.npoints
        finite = np.isfinite(lat) & np.isfinite(lon)
        with np.errstate(invalid='ignore'):
            i = np.clip(np.floor(np.mod(lon, 2*np.pi)/dlon), 0, self.nlon - 1)
            j = np.clip(np.floor((lat + np.pi/2)/dlat), 0, self.nlat - 1)
        key = np.where(finite, j*self.nlon + i, ncells).astype(np.int64)
        order = np.argsort(key, kind='stable')
        counts = np.bincount(key, minlength=ncells + 1)
        cell_start = np.concatenate([[0], np.cumsum(counts[:ncells])]).astype(np.int32)
        return order, cell_start


X0_COLUMNS = ('longitude', 'latitude', 'v', 'altitude', 'azimuth', 'frac')


def x0_columns(run):
    """An Output's X0 columns as float64 (Output.upcast), or None when it has no packet."""
    from .Output import Output
    X0 = run.X0
    if len(X0) == 0:
        return None
    missing = [c for c in X0_COLUMNS if c not in X0.columns]
    if missing:
        raise NotImplementedError(
            f'make_source_map needs X0 columns {missing}, which this Output did not keep (the '
            "device sampler drops them): run Input.run with sampler='numpy'")
    X0 = Output.upcast(X0[list(X0_COLUMNS)])
    return {c: np.ascontiguousarray(X0[c].values, dtype=np.float64) for c in X0_COLUMNS}


def output_vmax(cols, r_km):
    """make_source_map.py:56: ceil(max(v) * R_km) over every X0 packet (pandas' max skips NaN)."""
    return float(np.ceil(np.nanmax(cols['v'])*r_km))


def combine_small(pieces, vmaxes, nvel, vmax=None):
    """LOSResult.py:338-371 for the whole-planet histograms of the Outputs, in order: ``pieces``
    hold speed_dist, altitude_dist, azimuth_dist and speed_gridsum (the Output's speed map summed
    over the grid), ``vmaxes`` the Outputs' vmax.  Returns the global speed axis, the summed
    whole-planet histograms, the per-Output speed-map factors (2 or 1) and the vector the interp
    broadcast adds to every grid point's speed histogram.  ``vmax``: the global vmax of a shared
    run (default: the largest of ``vmaxes``)."""
    speeds = [centres(speed_edges(v, nvel)) for v in vmaxes]
    speed = centres(speed_edges(max(vmaxes) if vmax is None else vmax, nvel))
    top = speed.max()
    out = dict(speed=speed, speed_dist=np.zeros(nvel), broadcast=np.zeros(nvel))
    out['altitude_dist'] = np.zeros_like(pieces[0]['altitude_dist'])
    out['azimuth_dist'] = np.zeros_like(pieces[0]['azimuth_dist'])
    factors = []
    for piece, s in zip(pieces, speeds):
        out['altitude_dist'] += piece['altitude_dist']
        out['azimuth_dist'] += piece['azimuth_dist']
        out['speed_dist'] += piece['speed_dist']
        if s.max() == top:
            out['speed_dist'] += piece['speed_dist']
            factors.append(2.0)
        else:
            out['speed_dist'] += np.interp(speed, s, piece['speed_dist'])
            out['broadcast'] += np.interp(speed, s, piece['speed_gridsum'])
            factors.append(1.0)
    return out, factors


def finish(distribution, normalize, sourcerate, r_km):
    """LOSResult.py:373-447: fraction_observed and abundance, then (``normalize``) fluxes per cm^2
    for ``sourcerate`` [1e23 atoms/s] and the normalised distributions.  ``distribution``: the
    summed arrays (abundance_uncor, n_included, n_total [nlon, nlat]; *_dist_map [nlon, nlat, n];
    speed_dist, altitude_dist, azimuth_dist) and axes (longitude, latitude, speed, altitude,
    azimuth).  Changes it in place and returns it."""
    d = distribution
    with np.errstate(divide='ignore', invalid='ignore'):
        d['fraction_observed'] = d['n_included']/d['n_total']
        q = np.isnan(d['fraction_observed'])
        d['fraction_observed'][q] = 1
        d['abundance'] = d['abundance_uncor']/d['fraction_observed']
        d['fraction_observed'][q] = 0
        d['abundance'][np.isnan(d['abundance'])] = 0
        if not normalize:
            return d
        rate = float(sourcerate)*1e23                       # sourcerate.to(1/u.s)
        dx = d['longitude'][1] - d['longitude'][0]
        dy = d['latitude'][1] - d['latitude'][0]
        _, gridlatitude = np.meshgrid(d['longitude'], d['latitude'])
        d_area = np.abs(dx*(np.sin(gridlatitude + dy/2) - np.sin(gridlatitude - dy/2)))
        area = (r_km*1e5)**2*d_area
        d['abundance'] = d['abundance']/d['abundance'].sum()/area.T*rate
        d['abundance_uncor'] = d['abundance_uncor']/d['abundance_uncor'].sum()/area.T*rate
        sr = float(sourcerate)
        dv = d['speed'][1] - d['speed'][0]
        d['speed_dist'] = sr*d['speed_dist']/d['speed_dist'].sum()/dv*1e23
        d['speed_dist_map'] = (d['abundance'][:, :, np.newaxis]*d['speed_dist_map'] /
                               d['speed_dist_map'].sum(axis=2)[:, :, np.newaxis]/dv)
        for axis in ('altitude', 'azimuth'):
            da = d[axis][1] - d[axis][0]
            d[axis] = sr*d[axis]/d[axis].sum()/da*1e23
            key = axis + '_dist_map'
            d[key] = (d['abundance'][:, :, np.newaxis]*d[key] /
                      d[key].sum(axis=2)[:, :, np.newaxis]/da)
    return d


UNITS_NORMALIZED = {'abundance': '1/(cm2 s)', 'abundance_uncor': '1/(cm2 s)',
                    'speed_dist': '1/(km/s)/s', 'speed_dist_map': '1/(cm2 s)/(km/s)',
                    'altitude': '1/(s rad)', 'azimuth': '1/(s rad)',
                    'altitude_dist_map': '1/(cm2 s rad)', 'azimuth_dist_map': '1/(cm2 s rad)',
                    'longitude': 'rad', 'latitude': 'rad', 'speed': 'km/s'}
UNITS_RAW = {'longitude': 'rad', 'latitude': 'rad', 'speed': 'km/s', 'altitude': 'rad',
             'azimuth': 'rad'}


class SourceMap:
    """initial_state/SourceMap.py's attributes (abundance, longitude, latitude, speed, speed_dist,
    azimuth, azimuth_dist, altitude, altitude_dist, fraction_observed, coordinate_system) plus
    abundance_uncor, n_included, n_total and the three *_dist_map arrays; ``units`` names the
    unit of each array.  Built from a dict (load_dict) or from an .npz file written by ``save``."""

    ARRAYS = ('abundance', 'longitude', 'latitude', 'speed', 'speed_dist', 'azimuth',
              'azimuth_dist', 'altitude', 'altitude_dist', 'fraction_observed')

    EXTRA = ('abundance_uncor', 'n_included', 'n_total', 'speed_dist_map', 'altitude_dist_map',
             'azimuth_dist_map')

    def __init__(self, sourcemap=None, normalized=False):
        self.abundance = self.longitude = self.latitude = None
        self.speed = self.speed_dist = None
        self.azimuth = self.azimuth_dist = self.altitude = self.altitude_dist = None
        self.fraction_observed = None
        self.coordinate_system = 'solar-fixed'
        for key in self.EXTRA:
            setattr(self, key, None)
        self.units = dict(UNITS_NORMALIZED if normalized else UNITS_RAW)
        if isinstance(sourcemap, dict):
            self.load_dict(sourcemap)
        elif isinstance(sourcemap, (str, os.PathLike)) and os.fspath(sourcemap).endswith('.npz'):
            self.load_npz(sourcemap)
        elif sourcemap is not None:
            raise NotImplementedError(
                'loading .pkl / .sav source map files (pickled astropy quantities) is not '
                'supported: write the map with SourceMap.save to an .npz file and name that')

    def load_dict(self, sourcemap):
        for key in self.ARRAYS + self.EXTRA:
            setattr(self, key, sourcemap.get(key, None))
        self.coordinate_system = sourcemap.get('coordinate_system', 'solar-fixed')

    def save(self, path):
        """Write every attribute that is not None to ``path`` (.npz): the arrays as float64,
        coordinate_system as a string, ``units`` as two string arrays.  ``SourceMap(path)`` reads
        it back exactly."""
        if not os.fspath(path).endswith('.npz'):
            raise ValueError('SourceMap.save writes .npz files: the path must end in .npz')
        contents = {key: np.asarray(getattr(self, key), dtype=np.float64)
                    for key in self.ARRAYS + self.EXTRA if getattr(self, key) is not None}
        contents['coordinate_system'] = np.array(str(self.coordinate_system))
        contents['units_keys'] = np.array(list(self.units), dtype=str)
        contents['units_values'] = np.array([self.units[k] for k in self.units], dtype=str)
        with open(path, 'wb') as file:          # (np.savez would add a second .npz to a bare name)
            np.savez(file, **contents)

    def load_npz(self, path):
        with np.load(path, allow_pickle=False) as file:
            for key in self.ARRAYS + self.EXTRA:
                setattr(self, key, np.array(file[key]) if key in file.files else None)
            self.coordinate_system = str(file['coordinate_system'])
            self.units = dict(zip((str(k) for k in file['units_keys']),
                                  (str(v) for v in file['units_values'])))
