"""NumPy restatement of make_source_map.py:11-174 (one Output) and LOSResult.py:338-447 (the sum
over Outputs and the normalisation), written from the reference's behaviour for the tests.

Membership is vectorised per latitude row of grid points over the packets of its latitude band
(|phi_q - phi_p| <= r_p, with slack), using the haversine rule of sklearn's BallTree.query_radius;
the interp broadcast of LOSResult.py:364-371 is summed as one interp of the grid-summed speed map
(np.interp is linear in its values; test_sourcemap_cpu checks that against the literal loop)."""
import numpy as np

GRID = dict(smear_radius=np.radians(10), nlonbins=180, nlatbins=90, nvelbins=100, nazbins=45,
            naltbins=23, smear_abundance=True)


def params(grid_params=None):
    p = dict(GRID)
    p.update(grid_params or {})
    return p


def axis(lo, hi, n):
    e = np.linspace(lo, hi, n + 1)
    return e[:-1] + (e[1] - e[0])/2


def haversine(phi_p, lam_p, phi_q, lam_q, cos_p=None, cos_q=None):
    """sklearn's reduced haversine distance, point p (query) against packet q."""
    cos_p = np.cos(phi_p) if cos_p is None else cos_p
    cos_q = np.cos(phi_q) if cos_q is None else cos_q
    s0 = np.sin(0.5*(phi_p - phi_q))
    s1 = np.sin(0.5*(lam_p - lam_q))
    return s0*s0 + cos_p*cos_q*s1*s1


def grid_points(p):
    lon = axis(0, 2*np.pi, p['nlonbins'])
    lat = axis(-np.pi/2, np.pi/2, p['nlatbins'])
    return lon, lat


def members(lat, lon, p):
    """(point index, packet index) of every membership, point = i_lon * nlat + j_lat."""
    glon, glat = grid_points(p)
    nlat = len(glat)
    order = np.argsort(lat, kind='stable')
    slat = lat[order]
    pts, pks = [], []
    cos_q = np.cos(lat)
    for j, phi in enumerate(glat):
        r = p['smear_radius']*np.cos(phi)
        thr = np.sin(0.5*r)**2
        a, b = np.searchsorted(slat, [phi - r*1.001 - 1e-9, phi + r*1.001 + 1e-9])
        q = order[a:b]
        if len(q) == 0:
            continue
        h = haversine(phi, glon[:, None], lat[q][None, :], lon[q][None, :], np.cos(phi),
                      cos_q[q][None, :])
        i, k = np.nonzero(h <= thr)
        pts.append(i*nlat + j)
        pks.append(q[k])
    if not pts:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(pts), np.concatenate(pks)


def bins_of(values, lo, hi, n):
    """np.histogram's bin (with range=) of every value; -1 outside."""
    edges = np.linspace(lo, hi, n + 1)
    k = np.searchsorted(edges, values, side='right') - 1
    k[values == edges[-1]] = n - 1
    k[~((values >= edges[0]) & (values <= edges[-1]))] = -1
    return k


def one_output(X0, r_km, grid_params=None, todo='source'):
    """make_source_map.py for one Output's X0 columns (dict of float64 arrays)."""
    p = params(grid_params)
    lon, lat, v, alt, az, frac = (np.asarray(X0[c], dtype=np.float64) for c in
                                  ('longitude', 'latitude', 'v', 'altitude', 'azimuth', 'frac'))
    nlon, nlat, nvel = p['nlonbins'], p['nlatbins'], p['nvelbins']
    nalt, naz = p['naltbins'], p['nazbins']
    vmax = np.ceil(np.nanmax(v)*r_km)
    inc = frac > 0
    w = frac if todo == 'source' else np.ones_like(frac)
    hist2d, _, _ = np.histogram2d(lon[inc], lat[inc], bins=(nlon, nlat), weights=w[inc],
                                  range=[[0, 2*np.pi], [-np.pi/2, np.pi/2]])
    glon, glat = grid_points(p)
    d = dict(longitude=glon, latitude=glat, abundance_uncor=hist2d)
    d['speed_dist'] = np.histogram(v[inc]*r_km, bins=nvel, range=[0, vmax], weights=w[inc])[0]
    d['speed'] = axis(0, vmax, nvel)
    d['altitude_dist'] = np.histogram(alt[inc], bins=nalt, range=[0, np.pi/2], weights=w[inc])[0]
    d['altitude'] = axis(0, np.pi/2, nalt)
    d['azimuth_dist'] = np.histogram(az[inc], bins=naz, range=[0, 2*np.pi], weights=w[inc])[0]
    d['azimuth'] = axis(0, 2*np.pi, naz)
    P = nlon*nlat
    pt, pk = members(lat, lon, p)
    d['n_total'] = np.bincount(pt, minlength=P).astype(float).reshape(nlon, nlat)
    d['n_included'] = np.bincount(pt, weights=inc[pk].astype(float),
                                  minlength=P).reshape(nlon, nlat)
    if p['smear_abundance']:
        d['abundance_uncor'] = np.bincount(pt, weights=w[pk], minlength=P).reshape(nlon, nlat)
    keep = inc[pk]
    pt, pk = pt[keep], pk[keep]
    for key, values, lo, hi, n in (('speed_dist_map', v*r_km, 0, vmax, nvel),
                                   ('altitude_dist_map', alt, 0, np.pi/2, nalt),
                                   ('azimuth_dist_map', az, 0, 2*np.pi, naz)):
        b = bins_of(values[pk], lo, hi, n)
        ok = b >= 0
        flat = np.bincount(pt[ok]*n + b[ok], weights=w[pk][ok], minlength=P*n)
        d[key] = flat.reshape(nlon, nlat, n)
    return d


def combine(sources):
    """LOSResult.py:338-376 over per-Output dicts (the broadcast as one grid-summed interp)."""
    dist = {k: np.zeros_like(v) for k, v in sources[0].items()}
    vmaxes = [s['speed'].max() for s in sources]
    vmax = max(vmaxes)
    dist['speed'] = sources[int(np.where(np.array(vmaxes) == vmax)[0][0])]['speed']
    for s in sources:
        for key in ('abundance_uncor', 'n_included', 'n_total', 'altitude_dist',
                    'altitude_dist_map', 'azimuth_dist', 'azimuth_dist_map', 'speed_dist',
                    'speed_dist_map'):
            dist[key] = dist[key] + s[key]
        if s['speed'].max() == vmax:
            dist['speed_dist'] = dist['speed_dist'] + s['speed_dist']
            dist['speed_dist_map'] = dist['speed_dist_map'] + s['speed_dist_map']
        else:
            dist['speed_dist'] = dist['speed_dist'] + np.interp(dist['speed'], s['speed'],
                                                                s['speed_dist'])
            summed = s['speed_dist_map'].sum(axis=(0, 1))
            dist['speed_dist_map'] = dist['speed_dist_map'] + np.interp(dist['speed'], s['speed'],
                                                                        summed)
    for key in ('longitude', 'latitude', 'azimuth', 'altitude'):
        dist[key] = sources[0][key]
    return dist


def normalise(dist, normalize, sourcerate, r_km):
    """LOSResult.py:373-447: sourcerate in 1e23 atoms/s, area in cm^2."""
    d = dict(dist)
    with np.errstate(divide='ignore', invalid='ignore'):
        fo = d['n_included']/d['n_total']
        nan = np.isnan(fo)
        fo[nan] = 1
        ab = d['abundance_uncor']/fo
        fo[nan] = 0
        ab[np.isnan(ab)] = 0
        d['fraction_observed'], d['abundance'] = fo, ab
        if not normalize:
            return d
        rate = sourcerate*1e23
        dx = d['longitude'][1] - d['longitude'][0]
        dy = d['latitude'][1] - d['latitude'][0]
        lat2 = np.broadcast_to(d['latitude'][None, :], (len(d['longitude']), len(d['latitude'])))
        area = (r_km*1e5)**2*np.abs(dx*(np.sin(lat2 + dy/2) - np.sin(lat2 - dy/2)))
        d['abundance'] = ab/ab.sum()/area*rate
        d['abundance_uncor'] = d['abundance_uncor']/d['abundance_uncor'].sum()/area*rate
        dv = d['speed'][1] - d['speed'][0]
        d['speed_dist'] = sourcerate*d['speed_dist']/d['speed_dist'].sum()/dv*1e23
        a3 = d['abundance'][:, :, None]
        d['speed_dist_map'] = a3*d['speed_dist_map']/d['speed_dist_map'].sum(axis=2)[:, :, None]/dv
        for name in ('altitude', 'azimuth'):
            step = d[name][1] - d[name][0]
            d[name] = sourcerate*d[name]/d[name].sum()/step*1e23
            m = d[name + '_dist_map']
            d[name + '_dist_map'] = a3*m/m.sum(axis=2)[:, :, None]/step
    return d


def source_map(outputs_x0, r_km, grid_params=None, todo='source', normalize=True,
               sourcerate=1.0):
    """The whole restated make_source_map for a list of X0 column dicts (empty ones skipped)."""
    sources = [one_output(X0, r_km, grid_params, todo) for X0 in outputs_x0
               if len(X0['v'])]
    return normalise(combine(sources), normalize, sourcerate, r_km)
