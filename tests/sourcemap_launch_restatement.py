"""NumPy restatement of the device's launch from a source map (k_sample, spatial_type 2 and 3),
and the analytic law it is held to.

TEST INFRASTRUCTURE.  The uniforms are the kernels' own counter-based ones
(oracle.np_oracle.philox_uniform_pairs: blocks 0-2 as for every source, block 16 -> (u_cell, u_x),
block 17 -> (u_y, -) for the 2-D map); the arithmetic is the kernel's, operation for operation, so
the two agree to the last bits of libm's asin / sin / cos.  The cell a packet lands in cannot
differ: both sides compare the same fp64 cdf with the same uniform.

The law (what math/randomdeviates.py's random_deviates_2d accepts against): on
[lon.min, lon.max] x [s.min, s.max], s = sin(latitude), a density proportional to the bilinear
interpolant of abundance[nlon, nlat] on the even node grid linspace x linspace.
"""
import numpy as np

from oracle.np_oracle import philox_uniform_pairs

STREAM_SOURCE = 0x5a0
MAP_BLOCK = 16


def linear_inverse_cdf(f0, f1, u):
    """t in [0, 1] with CDF(t) = u for the density f0 + (f1 - f0) t (nxc_kernels.hpp,
    linear_inverse_cdf): u (f0+f1) / (f0 + sqrt(f0^2 + u (f0+f1) (f1-f0))); 0 for u = 0; u where
    both ends are zero."""
    s = f0 + f1
    with np.errstate(divide='ignore', invalid='ignore'):
        t = u*s/(f0 + np.sqrt(f0*f0 + u*s*(f1 - f0)))
    t = np.where(t < 1.0, t, 1.0)
    t = np.where(s > 0.0, t, u)
    return np.where(u > 0.0, t, 0.0)


def map_points(nodes, cdf, limits, u_cell, u_x, u_y):
    """(lon, lat, cell) of the 2-D map source for the three uniforms (nxc_kernels.hpp, map_point)."""
    nlon, nlat = nodes.shape
    lon0, lon1, s0, s1 = limits
    dlon, ds = (lon1 - lon0)/float(nlon - 1), (s1 - s0)/float(nlat - 1)
    cell = np.searchsorted(cdf, u_cell, side='right')        # first cell with cdf > u
    i, j = cell//(nlat - 1), cell % (nlat - 1)
    a, b, c, d = nodes[i, j], nodes[i, j + 1], nodes[i + 1, j], nodes[i + 1, j + 1]
    tx = linear_inverse_cdf(a + b, c + d, u_x)
    f0, f1 = (1.0 - tx)*a + tx*c, (1.0 - tx)*b + tx*d
    ty = linear_inverse_cdf(f0, f1, u_y)
    lon = lon0 + (i + tx)*dlon
    s = s0 + (j + ty)*ds
    return lon, np.arcsin(np.where(s < s1, s, s1)), cell


def launch_points(n, seed, first_index=0, *, spatial_type, map_nodes, map_cdf, map_lon0=0.0,
                  map_lon1=0.0, map_s0=0.0, map_s1=0.0, **unused):
    """(lon, lat) of packets first_index .. first_index + n - 1."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    if spatial_type == 3:
        ulon, _ = philox_uniform_pairs(idx, 1, STREAM_SOURCE, seed)
        return np.interp(ulon, map_cdf, map_nodes), np.zeros(n)
    assert spatial_type == 2
    u_cell, u_x = philox_uniform_pairs(idx, MAP_BLOCK, STREAM_SOURCE, seed)
    u_y, _ = philox_uniform_pairs(idx, MAP_BLOCK + 1, STREAM_SOURCE, seed)
    lon, lat, _ = map_points(np.asarray(map_nodes, dtype=float), np.asarray(map_cdf, dtype=float),
                             (map_lon0, map_lon1, map_s0, map_s1), u_cell, u_x, u_y)
    return lon, lat


def sample_x0(n, seed, first_index=0, *, endtime, exobase, unit_km, random_time, angular_type,
              is_planet, speed_type, vprob=0.0, vwidth=0.0, sinalt0=0.0, sinalt1=1.0, az0=0.0,
              az1=2*np.pi, speed_table=None, **source):
    """X0 (n, 8) of a map source: `launch_points` and then k_sample's speed and direction, as
    oracle.np_oracle.sample_x0_philox states them for the other sources (flat and tabulated
    speeds)."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    ut, _ = philox_uniform_pairs(idx, 0, STREAM_SOURCE, seed)
    _, uspd = philox_uniform_pairs(idx, 1, STREAM_SOURCE, seed)
    ualt, uaz = philox_uniform_pairs(idx, 2, STREAM_SOURCE, seed)
    time = ut*endtime if random_time else np.zeros(n) + endtime
    lon, lat = launch_points(n, seed, first_index, **source)
    sign = 1.0 if is_planet else -1.0
    x0 = sign*exobase*np.sin(lon)*np.cos(lat)
    y0 = -exobase*np.cos(lon)*np.cos(lat)
    z0 = exobase*np.sin(lat)
    if speed_type == 0:
        v = uspd*2*vwidth + vprob - vwidth
    else:
        assert speed_type == 2
        v = np.interp(uspd, speed_table[0], speed_table[1])
    v = v/unit_km
    if angular_type == 0:
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
    return X


# ---- the law, analytically --------------------------------------------------------------------------
def cell_probabilities(abundance):
    """Probability of each cell of the node grid, [nlon - 1, nlat - 1]: the integral of a bilinear
    function over a cell is the cell's area (equal for all) times the mean of its corners."""
    a = np.asarray(abundance, dtype=float)
    mass = a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:]
    return mass/mass.sum()


def cell_of(lon, s, limits, shape):
    """Lon-major index pair of the grid cell each (lon, s) lies in."""
    lon0, lon1, s0, s1 = limits
    nlon, nlat = shape
    i = np.clip(np.floor((lon - lon0)/((lon1 - lon0)/(nlon - 1))).astype(np.int64), 0, nlon - 2)
    j = np.clip(np.floor((s - s0)/((s1 - s0)/(nlat - 1))).astype(np.int64), 0, nlat - 2)
    return i, j


def cell_goodness_of_fit(lon, s, abundance, limits):
    """p-value of the chi-square goodness of fit of the points' cell counts against
    `cell_probabilities`, over all cells: those expecting fewer than 5 points are pooled into one
    bin, so nothing is left out.  A point in a cell of probability zero gives p = 0."""
    from scipy import stats
    prob = cell_probabilities(abundance)
    i, j = cell_of(lon, s, limits, np.shape(abundance))
    counts = np.zeros(prob.shape)
    np.add.at(counts, (i, j), 1.0)
    if np.any(counts[prob == 0] > 0):
        return 0.0
    expected = prob*len(lon)
    small = expected < 5
    obs, exp = list(counts[~small]), list(expected[~small])
    if expected[small].sum() > 0:
        obs.append(counts[small].sum())
        exp.append(expected[small].sum())
    obs, exp = np.array(obs), np.array(exp)
    chi2 = np.sum((obs - exp)**2/exp)
    return float(stats.chi2.sf(chi2, len(obs) - 1))
