"""NumPy restatement of the device's launch from a source map's per-point laws (k_sample's
NXC_LAW_NODES instantiation: speed_type 4, angular_type 2), the maps the tests use, and the
analytic law the draws are held to.

TEST INFRASTRUCTURE.  The uniforms are the kernels' own counter-based ones
(oracle.np_oracle.philox_uniform_pairs): blocks 0-2 as for every source, block 16 -> (u_cell, u_x),
block 17 -> (u_y, u_corner).  The launch point is tests/sourcemap_launch_restatement.py's; the
corner choice and the per-node inversion restate map_corner and interp_node operation for
operation.

The law: the joint density of launch point and per-point draw is sum_c w_c A_c p_c over the four
corner nodes of the point's cell (w bilinear hat weights in (longitude, sin latitude), A the
node's abundance, p its tabulated law).  Integrated over the map, node n is drawn with probability
A_n m_n / sum A m, m_n the number of cells touching n (each hat integrates to a quarter cell per
cell), and a per-point quantity has the mixture cdf sum_n P(n) cdf_n -- piecewise linear on the
shared grid, like every cdf_n.
"""
import numpy as np

from oracle.np_oracle import philox_uniform_pairs

from . import sourcemap_launch_restatement as S

STREAM_SOURCE, MAP_BLOCK = S.STREAM_SOURCE, S.MAP_BLOCK


# ---- the device's draw --------------------------------------------------------------------------------
def map_points(nodes, cdf, limits, u_cell, u_x, u_y):
    """S.map_points with what map_point additionally returns: (lon, lat, i, j, tx, ty)."""
    nlon, nlat = nodes.shape
    lon0, lon1, s0, s1 = limits
    dlon, ds = (lon1 - lon0)/float(nlon - 1), (s1 - s0)/float(nlat - 1)
    cell = np.searchsorted(cdf, u_cell, side='right')
    i, j = cell//(nlat - 1), cell % (nlat - 1)
    a, b, c, d = nodes[i, j], nodes[i, j + 1], nodes[i + 1, j], nodes[i + 1, j + 1]
    tx = S.linear_inverse_cdf(a + b, c + d, u_x)
    f0, f1 = (1.0 - tx)*a + tx*c, (1.0 - tx)*b + tx*d
    ty = S.linear_inverse_cdf(f0, f1, u_y)
    lon = lon0 + (i + tx)*dlon
    s = s0 + (j + ty)*ds
    return lon, np.arcsin(np.where(s < s1, s, s1)), i, j, tx, ty


def map_corner(nodes, i, j, tx, ty, u):
    """Node index i_lon * nlat + j_lat of the corner each packet draws from (nxc_kernels.hpp,
    map_corner), branch by branch."""
    a, b, c, d = nodes[i, j], nodes[i, j + 1], nodes[i + 1, j], nodes[i + 1, j + 1]
    w0, w1 = (1.0 - tx)*(1.0 - ty)*a, (1.0 - tx)*ty*b
    w2, w3 = tx*(1.0 - ty)*c, tx*ty*d
    r1 = w0 + w1
    r2 = r1 + w2
    total = r2 + w3
    target = u*total
    leftover = np.where(w3 > 0, 3, np.where(w2 > 0, 2, np.where(w1 > 0, 1, 0)))
    k = np.where(w0 > target, 0, np.where(r1 > target, 1, np.where(r2 > target, 2,
                 np.where(total > target, 3, leftover))))
    best, largest = a.copy(), np.zeros(len(a), dtype=np.int64)
    for corner, value in ((1, b), (2, c), (3, d)):
        largest = np.where(value > best, corner, largest)
        best = np.where(value > best, value, best)
    k = np.where(total > 0.0, k, largest)
    return (i + (k >> 1))*nodes.shape[1] + (j + (k & 1))


def interp_node(cdf_table, grid, node, u):
    """np.interp(u, cdf_table[node], grid) for each packet (interp_node = interp_global on the
    node's row; np.interp is what interp_global restates)."""
    out = np.empty(len(u))
    order = np.argsort(node, kind='stable')
    ranked = node[order]
    starts = np.flatnonzero(np.r_[True, ranked[1:] != ranked[:-1]])
    for first, last in zip(starts, np.r_[starts[1:], len(u)]):
        rows = order[first:last]
        out[rows] = np.interp(u[rows], cdf_table[ranked[first]], grid)
    return out


def draw(n, seed, first_index=0, *, endtime, exobase, unit_km, random_time, angular_type,
         is_planet, speed_type, map_nodes, map_cdf, map_lon0, map_lon1, map_s0, map_s1,
         spatial_type=2, vprob=0.0, vwidth=0.0, sinalt0=0.0, sinalt1=1.0, az0=0.0, az1=2*np.pi,
         speed_table=None, node_speed_table=None, node_altitude_table=None,
         node_azimuth_table=None, **unused):
    """Everything k_sample<NXC_LAW_NODES> forms for packets first_index .. first_index + n - 1:
    X (n, 8) and lon, lat, node, speed [km/s], altitude, azimuth."""
    assert spatial_type == 2
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    ut, _ = philox_uniform_pairs(idx, 0, STREAM_SOURCE, seed)
    _, uspd = philox_uniform_pairs(idx, 1, STREAM_SOURCE, seed)
    ualt, uaz = philox_uniform_pairs(idx, 2, STREAM_SOURCE, seed)
    u_cell, u_x = philox_uniform_pairs(idx, MAP_BLOCK, STREAM_SOURCE, seed)
    u_y, u_corner = philox_uniform_pairs(idx, MAP_BLOCK + 1, STREAM_SOURCE, seed)
    nodes = np.asarray(map_nodes, dtype=float)
    lon, lat, i, j, tx, ty = map_points(nodes, np.asarray(map_cdf, dtype=float),
                                        (map_lon0, map_lon1, map_s0, map_s1), u_cell, u_x, u_y)
    node = map_corner(nodes, i, j, tx, ty, u_corner)
    time = ut*endtime if random_time else np.zeros(n) + endtime
    sign = 1.0 if is_planet else -1.0
    x0 = sign*exobase*np.sin(lon)*np.cos(lat)
    y0 = -exobase*np.cos(lon)*np.cos(lat)
    z0 = exobase*np.sin(lat)
    if speed_type == 0:
        speed = uspd*2*vwidth + vprob - vwidth
    elif speed_type == 2:
        speed = np.interp(uspd, speed_table[0], speed_table[1])
    else:
        assert speed_type == 4
        speed = interp_node(node_speed_table[0], node_speed_table[1], node, uspd)
    v = speed/unit_km
    if angular_type == 2:
        alt = interp_node(node_altitude_table[0], node_altitude_table[1], node, ualt)
        az = interp_node(node_azimuth_table[0], node_azimuth_table[1], node, uaz)
    elif angular_type == 0:
        alt, az = np.zeros(n) + np.pi/2, np.zeros(n)
    else:
        alt = np.arcsin(ualt*(sinalt1 - sinalt0) + sinalt0)
        az = az0 + (az1 - az0)*uaz
    v_rad, v_t0, v_t1 = np.sin(alt), np.cos(alt)*np.cos(az), np.cos(alt)*np.sin(az)
    rn = np.sqrt((x0*x0 + y0*y0) + z0*z0)
    en = np.sqrt(y0*y0 + x0*x0)
    n0, n1, n2 = -z0*x0, -z0*y0, x0*x0 + y0*y0
    nn = np.sqrt((n0*n0 + n1*n1) + n2*n2)
    X = np.zeros((n, 8))
    X[:, 0] = time
    X[:, 1], X[:, 2], X[:, 3] = x0, y0, z0
    X[:, 4] = ((v_t0*(n0/nn) + v_t1*(y0/en)) + v_rad*(x0/rn))*v
    X[:, 5] = ((v_t0*(n1/nn) + v_t1*(-x0/en)) + v_rad*(y0/rn))*v
    X[:, 6] = ((v_t0*(n2/nn) + v_t1*0.0) + v_rad*(z0/rn))*v
    X[:, 7] = 1.0
    return dict(X=X, lon=lon, lat=lat, node=node, speed=speed, altitude=alt, azimuth=az)


def launch_angles(X):
    """(speed, altitude, azimuth) of states given as rows (time, x, y, z, vx, vy, vz, frac): the
    inverse of the local frame k_sample launches in (radial, east, north of the launch point)."""
    x, y, z = X[1], X[2], X[3]
    vel = X[4:7]
    radial = np.array([x, y, z])/np.sqrt(x*x + y*y + z*z)
    east = np.array([y, -x, np.zeros_like(z)])/np.sqrt(x*x + y*y)
    north = np.array([-z*x, -z*y, x*x + y*y])
    north = north/np.sqrt((north**2).sum(axis=0))
    speed = np.sqrt((vel**2).sum(axis=0))
    up, to_e, to_n = (radial*vel).sum(axis=0), (east*vel).sum(axis=0), (north*vel).sum(axis=0)
    altitude = np.arcsin(np.clip(up/speed, -1, 1))
    return speed, altitude, np.arctan2(to_e, to_n) % (2*np.pi)


# ---- the maps ----------------------------------------------------------------------------------------
NV, NA, NZ = 7, 3, 4


def angle_centres(top, n):
    edges = np.linspace(0, top, n + 1)
    return edges[:-1] + (edges[1] - edges[0])/2


def coded_map():
    """5 x 4 nodes whose laws decode the node.  A law that sits in bin k >= 1 alone puts its
    deviates into (grid[k - 1], grid[k]) -- density_cdf drops bin 0 -- so nv = 7, na = 3, nz = 4
    give 6, 2 and 3 distinguishable laws: fewer than nodes for any one of them, 36 for the triple,
    and each of the 17 nodes with abundance gets a triple of its own (its speed bin alone cannot
    decode 17 nodes; the triple also shows that one corner serves all three draws).  Rows therefore
    have leading and trailing zeros.  Nodes (3, 3), (4, 2), (4, 3) have no abundance, which leaves
    cell (3, 2) with mass at the single corner (3, 2); (3, 3) and (4, 3) carry NaN rows, (4, 2)
    ordinary ones that must never be used."""
    longitude = np.linspace(0, 2*np.pi, 5)
    latitude = np.linspace(-np.pi/2, np.pi/2, 4)
    abundance = 0.5 + np.arange(20, dtype=float).reshape(5, 4) % 7
    abundance[3, 3] = abundance[4, 2] = abundance[4, 3] = 0.0
    speed_map, alt_map, az_map = np.zeros((5, 4, NV)), np.zeros((5, 4, NA)), np.zeros((5, 4, NZ))
    code = {}
    for n in range(20):
        i, j = divmod(n, 4)
        ks, ka, kz = 1 + n % 6, 1 + (n//6) % 2, 1 + (n//12 + n) % 3
        speed_map[i, j, ks], alt_map[i, j, ka], az_map[i, j, kz] = 2.0, 0.5, 3.0
        if abundance[i, j] > 0:
            assert (ks, ka, kz) not in code
            code[ks, ka, kz] = n
    for i, j in ((3, 3), (4, 3)):
        speed_map[i, j] = alt_map[i, j] = az_map[i, j] = np.nan
    content = dict(longitude=longitude, latitude=latitude, abundance=abundance,
                   speed=np.linspace(0.25, 3.25, NV), speed_dist_map=speed_map,
                   altitude_dist_map=alt_map, azimuth_dist_map=az_map)
    return content, code


def decode_nodes(code, speed_grid, alt_grid, az_grid, speed, altitude, azimuth):
    """The node each packet of the coded map drew from, -1 for a triple no node with abundance
    has."""
    ks = np.searchsorted(speed_grid, speed, side='left')
    ka = np.searchsorted(alt_grid, altitude, side='left')
    kz = np.searchsorted(az_grid, azimuth, side='left')
    table = -np.ones((NV + 1, NA + 1, NZ + 1), dtype=np.int64)
    for (a, b, c), n in code.items():
        table[a, b, c] = n
    return table[ks, ka, kz]


def smooth_map():
    """181 x 91 nodes, abundance > 0 everywhere, laws that change across the map: speeds hotter
    towards longitude 0, altitudes more vertical towards the poles, azimuths peaked away from the
    node's longitude."""
    longitude = np.linspace(0, 2*np.pi, 181)
    latitude = np.linspace(-np.pi/2, np.pi/2, 91)
    lon, lat = np.meshgrid(longitude, latitude, indexing='ij')
    abundance = 1.0 + 0.8*np.cos(lon)*np.cos(lat)
    speed = np.linspace(0.1, 4.7, 24)
    vth2 = (1.0 + 0.9*np.cos(lon)*np.cos(lat))[:, :, None] + 0.3
    speed_map = speed**3*np.exp(-speed**2/vth2)
    alt = angle_centres(np.pi/2, 9)
    alt_map = np.cos(alt)*np.sin(alt)**(1.0 + 2.0*np.abs(np.sin(lat)))[:, :, None]
    az = angle_centres(2*np.pi, 12)
    az_map = 1.0 + 0.6*np.cos(az - lon[:, :, None])
    return dict(longitude=longitude, latitude=latitude, abundance=abundance, speed=speed,
                speed_dist_map=speed_map, altitude_dist_map=alt_map, azimuth_dist_map=az_map)


# ---- the law, analytically -----------------------------------------------------------------------------
def node_probabilities(abundance):
    """P(node) = A m / sum A m, flat in node order; m = cells touching the node (1, 2 or 4)."""
    a = np.asarray(abundance, dtype=float)
    m = np.ones(a.shape)
    m[1:-1, :] *= 2
    m[:, 1:-1] *= 2
    return (a*m/(a*m).sum()).ravel()


def node_goodness_of_fit(node, abundance):
    """p-value of the chi-square goodness of fit of the node counts against node_probabilities,
    over all nodes (those expecting fewer than 5 packets pooled, as in S.cell_goodness_of_fit);
    0 when a node without abundance (or no node at all, index < 0) was drawn."""
    from scipy import stats
    prob = node_probabilities(abundance)
    if np.any(node < 0):
        return 0.0
    counts = np.bincount(node, minlength=len(prob)).astype(float)
    if np.any(counts[prob == 0] > 0):
        return 0.0
    expected = prob*len(node)
    small = expected < 5                   # pooled into one bin, so that nothing is left out
    obs, exp = list(counts[~small]), list(expected[~small])
    if expected[small].sum() > 0:
        obs.append(counts[small].sum())
        exp.append(expected[small].sum())
    obs, exp = np.array(obs), np.array(exp)
    chi2 = np.sum((obs - exp)**2/exp)
    return float(stats.chi2.sf(chi2, len(obs) - 1))


def mixture_cdf(abundance, table):
    """The cdf of a per-point quantity over the whole map as a function of x: sum_n P(n) cdf_n,
    piecewise linear on the table's grid."""
    cdf_table, grid = table
    mixed = node_probabilities(abundance) @ cdf_table
    return lambda x: np.interp(x, grid, mixed)
