"""The source-map pass's planted cases and their brute-force reference (no test lives here).

k_smap_points only sees the packets of the cells the host listed for its tile (sourcemap.py:
``SourceMapGrid._segments`` -- a latitude band, a longitude window that wraps at 0 / 2 pi, whole
rows near the poles -- and ``bucket``).  A lost member changes n_total by one in a few points, and
nothing downstream would flag it.  So the packets here are planted where a cull or a ragged tile
would lose them, and the reference has no cull at all.

``memberships(grid, lat, lon)``  every grid point against every packet: the haversine rule of
    sourcemap.py:13-14 in np.longdouble, the thresholds sin(0.5 * smear_radius * cos(phi_p))**2
    from the float64 grid centres also in longdouble.  Returns the (point, packet) pairs and, per
    packet, the smallest relative distance |hav - thr| / thr to any point's threshold.
``arrays(grid, X0, pt, pk, vmax, available, factor, select)``  what the device keeps for one
    Output: the raw accumulator [npoints, nvel + nalt + naz + 3] (speed part times ``factor``),
    hist2d (np.histogram2d), the whole-planet histograms (np.histogram) and the grid-summed speed
    histogram.
``case(name)``  one planted case of ``CASES``, built once: grid, packets, memberships.

Planted per grid: for every latitude row (or the rows a trimmed case names) and every longitude
that is the first or last of a tile, plus 0 and nlon - 1, packets at great-circle distance
r_p * f, f in RIM, along evenly spaced bearings and along the two bearings at which the circle
touches a meridian (the largest |dlam|: cos(bearing) = tan(d) tan(phi_p)), by the destination-point
formula in longdouble, longitudes reduced mod 2 pi, r_p * f >= pi skipped.  Copies of seam packets
with longitude exactly 0, exactly 2 pi, and moved by -2 pi and +2 pi (in balls like their
originals; hist2d keeps the first two and drops the moved ones), packets within 1e-7 rad of both
poles, and a few hundred random ones.

Columns: frac = k / 2**20 with integer k, about a fifth at 0, so that with factors 1 and 2 every
device sum is exact in fp64 whatever its order, and every comparison is np.array_equal.  v,
altitude and azimuth are random with some on the histograms' first and last edges; one packet has
v * r_km on vmax exactly.

The device's fp64 sin / cos need not match NumPy's last bit: for the smallest ball here (some
1e-3 rad against coordinates of order 1, rounded to 1e-16) that is a relative error of order 1e-12
in hav.  A packet whose relative distance to any point's threshold is <= NEAR = 1e-10 is dropped;
the planted rims sit 2e-9 away.  ``Case.dropped`` counts them; the share is capped at
MAX_DROPPED = 1 %."""
import functools
from collections import namedtuple

import numpy as np

from nexoclom_amd import sourcemap as SM
from tests import sourcemap_restatement as R

R_KM = 2439.7
NEAR = 1e-10
MAX_DROPPED = 0.01
RIM = (1 - 1e-9, 1 + 1e-9, 0.5)
SMALL_BINS = dict(nvelbins=7, naltbins=5, nazbins=6)
LD = np.longdouble
PI = LD('3.14159265358979323846264338327950288')

Case = namedtuple('Case', 'name params grid X0 pt pk planted rim dropped seam info')


def small(nlon, nlat, degrees, **more):
    return dict(nlonbins=nlon, nlatbins=nlat, smear_radius=np.radians(degrees), **SMALL_BINS,
                **more)


# name: (grid parameters, what to plant).  Each grid is chosen for what it forces.
CASES = {
    # ragged tile 16 + 8
    '24x13 20deg': (small(24, 13, 20), {}),
    # tiles 16 + 16 + 5, window narrower than a tile
    '37x9 3deg': (small(37, 9, 3), {}),
    # ball smaller than a cell: most candidate cells empty
    '33x17 0.5deg': (small(33, 17, 0.5), {}),
    # tile = nlon < 16, two rows
    '5x2 50deg': (small(5, 2, 50), {}),
    # one point, one tile, one cell
    '1x1 30deg': (small(1, 1, 30), {}),
    # r >= pi/2: the window opens to whole rows
    '40x21 100deg': (small(40, 21, 100), {}),
    # r >= pi on the equatorial rows: every row walked, threshold past its maximum
    '40x21 200deg': (small(40, 21, 200), dict(bearings=24)),
    # tile = 8 from the LDS budget
    '19x7 12deg nvel400': (dict(nlonbins=19, nlatbins=7, smear_radius=np.radians(12),
                                nvelbins=400), dict(bearings=24)),
    # tile = 1, 1550 tiles (more than one k_smap_gridsum stride)
    '50x31 3deg nvel3000': (dict(nlonbins=50, nlatbins=31, smear_radius=np.radians(3),
                                 nvelbins=3000),
                            dict(bearings=16, rows=(0, 1, 8, 15, 22, 29, 30),
                                 lons=(0, 1, 17, 24, 25, 33, 48, 49), random=100)),
}
EXPECTED_TILE = {'24x13 20deg': 16, '37x9 3deg': 16, '33x17 0.5deg': 16, '5x2 50deg': 5,
                 '1x1 30deg': 1, '40x21 100deg': 16, '40x21 200deg': 16, '19x7 12deg nvel400': 8,
                 '50x31 3deg nvel3000': 1}


def tile_longitudes(grid):
    """The longitude indices that are the first or last of a tile, plus 0 and nlon - 1."""
    T, nlon = grid.tile, grid.nlon
    out = {0, nlon - 1}
    for k in range(-(-nlon // T)):
        out.update((k*T, min(k*T + T, nlon) - 1))
    return sorted(out)


def destination(phi, lam, d, bearing):
    """The point at great-circle distance d from (phi, lam) along ``bearing`` (from north), in
    longdouble; longitude in [0, 2 pi)."""
    phi, lam, d, bearing = (np.asarray(a, dtype=LD) for a in (phi, lam, d, bearing))
    s = np.sin(phi)*np.cos(d) + np.cos(phi)*np.sin(d)*np.cos(bearing)
    phi2 = np.arcsin(np.clip(s, -1, 1))
    lam2 = lam + np.arctan2(np.sin(bearing)*np.sin(d)*np.cos(phi), np.cos(d) - np.sin(phi)*s)
    return phi2, np.mod(lam2, 2*PI)


def rim_packets(grid, rows=None, lons=None, bearings=48):
    """(lat, lon) in float64 of the packets planted around the chosen points, and the point
    (i, j) and factor f each was planted for."""
    rows = range(grid.nlat) if rows is None else rows
    lons = tile_longitudes(grid) if lons is None else lons
    even = 2*PI*np.arange(bearings, dtype=LD)/bearings
    lat, lon, owner = [], [], []
    for j in rows:
        phi, r = LD(grid.lat[j]), LD(grid.smear_radius)*np.cos(LD(grid.lat[j]))
        for f in RIM:
            d = r*LD(f)
            if not d < PI:
                continue
            theta = even
            c = np.tan(d)*np.tan(phi)
            if d < PI/2 and abs(c) <= 1:               # the circle touches two meridians
                touch = np.arccos(c)
                theta = np.concatenate([even, [touch, 2*PI - touch]])
            for i in lons:
                p2, l2 = destination(phi, LD(grid.lon[i]), d, theta)
                lat.append(p2.astype(np.float64))
                lon.append(l2.astype(np.float64))
                owner += [(i, j, f)]*len(theta)
    return np.concatenate(lat), np.concatenate(lon), owner


def memberships(grid, lat, lon, chunk=4096):
    """(pt, pk, rel): every (point, packet) pair with hav <= thr, point = i_lon * nlat + j_lat,
    and per packet the smallest |hav - thr| / thr over all points.  All points x all packets in
    longdouble: no band, no window."""
    glon, glat = grid.lon.astype(LD), grid.lat.astype(LD)
    cos_p = np.cos(glat)
    thr = np.sin(LD(0.5)*LD(grid.smear_radius)*cos_p)**2
    pts, pks, rel = [], [], np.full(len(lat), np.inf, dtype=LD)
    for q0 in range(0, len(lat), chunk):
        phi_q, lam_q = lat[q0:q0 + chunk].astype(LD), lon[q0:q0 + chunk].astype(LD)
        cos_q = np.cos(phi_q)
        s_lon = np.sin(LD(0.5)*(glon[:, None] - lam_q[None, :]))**2            # [nlon, n]
        for j in range(grid.nlat):
            a = np.sin(LD(0.5)*(glat[j] - phi_q))**2
            hav = a[None, :] + (cos_p[j]*cos_q)[None, :]*s_lon
            i, k = np.nonzero(hav <= thr[j])
            pts.append(i*grid.nlat + j)
            pks.append(k + q0)
            near = (np.abs(hav - thr[j])/thr[j]).min(axis=0)
            rel[q0:q0 + chunk] = np.minimum(rel[q0:q0 + chunk], near)
    pt = np.concatenate(pts).astype(np.int64) if pts else np.zeros(0, dtype=np.int64)
    pk = np.concatenate(pks).astype(np.int64) if pks else np.zeros(0, dtype=np.int64)
    return pt, pk, rel.astype(np.float64)


def dyadic_frac(rng, n):
    """k / 2**20, k in 1 .. 2**20; about a fifth at 0."""
    frac = rng.integers(1, 2**20 + 1, n)/2.0**20
    frac[rng.random(n) < 0.2] = 0.0
    return frac


def on_vmax(vmax, r_km=R_KM):
    """A v with v * r_km == vmax exactly (one fp64 product, as the device forms the speed)."""
    v = vmax/r_km
    for _ in range(8):
        for cand in (v, np.nextafter(v, 0), np.nextafter(v, 1)):
            if cand*r_km == vmax:
                return cand
        v = np.nextafter(v, 0) if v*r_km > vmax else np.nextafter(v, 1)
    raise AssertionError(f'no v with v * {r_km} == {vmax}')


def columns(rng, n, vmax=4.0, r_km=R_KM):
    """v, altitude, azimuth and frac of n packets (n >= 16): random, the first ones on the first
    and last edges of each histogram; ceil(max(v) * r_km) == vmax and packet 0 sits on it."""
    v = rng.uniform(0, (vmax - 0.25)/r_km, n)
    alt = rng.uniform(0, np.pi/2, n)
    az = rng.uniform(0, 2*np.pi, n)
    frac = dyadic_frac(rng, n)
    v[0], v[1], v[2] = on_vmax(vmax, r_km), 0.0, on_vmax(vmax, r_km)
    alt[3], alt[4], alt[5] = 0.0, np.pi/2, np.pi/2
    az[6], az[7], az[8] = 0.0, 2*np.pi, 2*np.pi
    frac[:9] = np.arange(1, 10)/2.0**20
    frac[2] = 0.0                                      # on an edge, but not included
    where = rng.permutation(n)                         # the edge packets anywhere on the sphere
    return {c: a[where] for c, a in (('v', v), ('altitude', alt), ('azimuth', az),
                                     ('frac', frac))}


def bucketed(grid, X0):
    """(X0 sorted by cell, cell_start): what source_map_accumulate takes."""
    order, cell_start = grid.bucket(X0['latitude'], X0['longitude'])
    return {c: X0[c][order] for c in SM.X0_COLUMNS}, cell_start


def cell_of_packets(grid, lat, lon):
    order, cell_start = grid.bucket(lat, lon)
    cell = np.full(len(lat), grid.npoints, dtype=np.int64)
    cell[order[:cell_start[-1]]] = np.repeat(np.arange(grid.npoints), np.diff(cell_start))
    return cell


def tile_of_point(grid, pt):
    tpr = -(-grid.nlon // grid.tile)
    return (pt % grid.nlat)*tpr + (pt // grid.nlat)//grid.tile


def walked_cells(grid, t):
    """The cells tile t's segment list names, in order (a cell named twice appears twice)."""
    runs = grid.seg[grid.seg_off[t]:grid.seg_off[t + 1]]
    if len(runs) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(a, b + 1) for a, b in runs])


def candidate_total(grid, cell_start, t):
    """The packets tile t walks: k_smap_points' ``total``."""
    runs = grid.seg[grid.seg_off[t]:grid.seg_off[t + 1]]
    return int(sum(cell_start[b + 1] - cell_start[a] for a, b in runs))


def arrays(grid, X0, pt, pk, vmax, available=False, factor=1.0, select=None):
    """One Output's share of what the device keeps.  ``select``: boolean mask of the packets of
    X0 that form the Output (default: all); pt / pk index X0."""
    n = len(X0['frac'])
    sel = np.ones(n, dtype=bool) if select is None else np.asarray(select, dtype=bool)
    lon, lat, v, alt, az, frac = (X0[c] for c in SM.X0_COLUMNS)
    nlon, nlat, nvel, nalt, naz = grid.nlon, grid.nlat, grid.nvel, grid.nalt, grid.naz
    P = grid.npoints
    inc = (frac > 0) & sel
    w = np.ones(n) if available else frac
    speed = v*grid.r_km
    out = {}
    out['hist2d'] = np.histogram2d(lon[inc], lat[inc], bins=(nlon, nlat), weights=w[inc],
                                   range=[[0, 2*np.pi], [-np.pi/2, np.pi/2]])[0].ravel()
    out['speed_dist'] = np.histogram(speed[inc], bins=nvel, range=[0, vmax], weights=w[inc])[0]
    out['altitude_dist'] = np.histogram(alt[inc], bins=nalt, range=[0, np.pi/2],
                                        weights=w[inc])[0]
    out['azimuth_dist'] = np.histogram(az[inc], bins=naz, range=[0, 2*np.pi], weights=w[inc])[0]
    keep = sel[pk]
    pt, pk = pt[keep], pk[keep]
    acc = np.zeros((P, nvel + nalt + naz + 3))
    nb = nvel + nalt + naz
    acc[:, nb] = np.bincount(pt, minlength=P)
    acc[:, nb + 1] = np.bincount(pt, weights=inc[pk].astype(float), minlength=P)
    acc[:, nb + 2] = np.bincount(pt, weights=w[pk], minlength=P)
    keep = inc[pk]
    pt, pk = pt[keep], pk[keep]
    at = 0
    for values, lo, hi, nbin, scale in ((speed, 0, vmax, nvel, factor), (alt, 0, np.pi/2, nalt, 1.0),
                                        (az, 0, 2*np.pi, naz, 1.0)):
        b = R.bins_of(values[pk], lo, hi, nbin)
        ok = b >= 0
        hist = np.bincount(pt[ok]*nbin + b[ok], weights=w[pk][ok], minlength=P*nbin)
        hist = hist.reshape(P, nbin)
        if at == 0:
            out['speed_gridsum'] = hist.sum(axis=0)
        acc[:, at:at + nbin] = scale*hist
        at += nbin
    out['acc'] = acc
    return out


PIECES = ('speed_dist', 'altitude_dist', 'azimuth_dist', 'speed_gridsum')


def build_case(name, params, rows=None, lons=None, bearings=48, random=300, seed=11):
    grid = SM.SourceMapGrid(params, R_KM)
    assert grid.tile == EXPECTED_TILE.get(name, grid.tile), (name, grid.tile)
    rng = np.random.default_rng(seed)
    lat, lon, owner = rim_packets(grid, rows, lons, bearings)
    planted = len(lat)
    # seam copies: packets planted for the first and last longitude, at longitude exactly 0 and
    # exactly 2 pi (same latitude) and moved by -2 pi and +2 pi
    at_seam = np.array([k for k, (i, j, f) in enumerate(owner) if i in (0, grid.nlon - 1)])
    src = at_seam[rng.choice(len(at_seam), min(6, len(at_seam)), replace=False)]
    first = len(lat)
    lat = np.concatenate([lat, lat[src], lat[src], lat[src], lat[src]])
    lon = np.concatenate([lon, np.zeros(len(src)), np.full(len(src), 2*np.pi),
                          lon[src] - 2*np.pi, lon[src] + 2*np.pi])
    seam = dict(source=src, zero=first + np.arange(len(src)),
                two_pi=first + len(src) + np.arange(len(src)),
                minus=first + 2*len(src) + np.arange(len(src)),
                plus=first + 3*len(src) + np.arange(len(src)))
    # both poles
    npole = 8
    pole = (np.pi/2 - 1e-7*rng.random(2*npole))*np.repeat([1.0, -1.0], npole)
    lat = np.concatenate([lat, pole, np.arcsin(rng.uniform(-1, 1, random))])
    lon = np.concatenate([lon, rng.uniform(0, 2*np.pi, 2*npole), rng.uniform(0, 2*np.pi, random)])
    pt, pk, rel = memberships(grid, lat, lon)
    keep = rel > NEAR
    dropped = int((~keep).sum())
    # renumber the kept packets
    new = np.cumsum(keep) - 1
    ok = keep[pk]
    pt, pk = pt[ok], new[pk[ok]]
    seam = {k: np.where(keep[v], new[v], -1) for k, v in seam.items()}
    lat, lon = lat[keep], lon[keep]
    # the kept rim packets come first: rim[k] = (i, j, index into RIM) of packet k's point
    rim = np.array([(i, j, RIM.index(f)) for i, j, f in owner], dtype=np.int64)[keep[:planted]]
    X0 = dict(latitude=lat, longitude=lon, **columns(rng, len(lat)))
    info = dict(packets=len(lat), memberships=len(pt), total=len(keep),
                share=dropped/len(keep), smallest_rel=float(rel[keep].min()),
                vmax=SM.output_vmax(X0, R_KM))
    return Case(name, params, grid, X0, pt, pk, planted, rim, dropped, seam, info)


@functools.lru_cache(maxsize=None)
def case(name):
    params, plant = CASES[name]
    return build_case(name, params, **plant)


def cluster_case(params, cells, counts, seed=3, spread=0.45):
    """Packets in chosen cells only: counts[k] packets inside cell cells[k] = (i, j), within
    ``spread`` of a cell's width around its centre, near-threshold ones replaced.  Returns (grid,
    X0, pt, pk)."""
    grid = SM.SourceMapGrid(params, R_KM)
    rng = np.random.default_rng(seed)
    dlon, dlat = grid.lon_edges[1] - grid.lon_edges[0], grid.lat_edges[1] - grid.lat_edges[0]
    lat, lon = [], []
    for (i, j), n in zip(cells, counts):
        la, lo = np.zeros(0), np.zeros(0)
        while len(la) < n:
            a = grid.lat[j] + dlat*rng.uniform(-spread, spread, n)
            o = grid.lon[i] + dlon*rng.uniform(-spread, spread, n)
            far = memberships(grid, a, o)[2] > NEAR
            la, lo = np.concatenate([la, a[far]])[:n], np.concatenate([lo, o[far]])[:n]
        lat.append(la)
        lon.append(lo)
    lat, lon = np.concatenate(lat), np.concatenate(lon)
    pt, pk, rel = memberships(grid, lat, lon)
    assert (rel > NEAR).all()
    n = len(lat)
    if n >= 16:
        cols = columns(rng, n)
    else:
        cols = dict(v=rng.uniform(0, 3.5/R_KM, n), altitude=rng.uniform(0, np.pi/2, n),
                    azimuth=rng.uniform(0, 2*np.pi, n), frac=np.arange(1, n + 1)/2.0**20)
    return grid, dict(latitude=lat, longitude=lon, **cols), pt, pk
