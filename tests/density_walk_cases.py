"""The density kernels' cell cull and candidate walk restated with NumPy, a point index with a
caller-chosen cell edge, and the planted cases that drive both (no test lives here).

k_density, k_density_moments and k_density_spectrum find the query points within ``dr`` of a row
the same way (nxc_kernels.hpp: density_cells, then the (cy, cz) range walk of density_walk, which
k_density_moments carries written out).  ``DensityIndex(points, dr)`` starts from the edge
h = dr (1 + 2^-20), where r_cell = dr / h + 1e-6 > 1 and every row visits all 27 cells around
it; the cull only decides anything on a grid of edge h > dr, which the product builds once the
grid would pass ``MAX_CELLS``.  Two ways lead there at test sizes:

``grid_index(points, dr, h, origin, pad)``  the layout documented on ``DensityIndex`` restated for
    any edge h >= dr (1 + 2^-20), any origin at or below the points and extra empty cells;
``product_index(points, dr, max_cells, monkeypatch)``  the product's own class, growth loop
    included, with the module's ``MAX_CELLS`` lowered.

``restated_walk`` follows the kernel step by step and takes the narrowing mutations of
``MUTATIONS``, which tests/test_density_walk_cpu.py uses to show that the cases are sharp.

Every case is a ``Case``: ``points`` (Q, 3) and ``rows`` (P, 3) in float64 (rows planted in
float32 are given widened), ``dr`` = 2^-4 and grid origins that are dyadic, so that distances
planted along an axis are exact; ``grid`` says how its index is built (``build_index``);
``hits`` / ``misses`` are the planted (point, row) pairs that are meant to be within ``dr`` or
not; ``ordinary`` masks the rows a KD-tree can take (all but the planted non-finite ones)."""
import functools
import importlib
import itertools
from collections import namedtuple

import numpy as np

CELL_SLACK = 1.0 + 2.0**-20
DR = 2.0**-4
ORIGIN = np.array([-17., 9., -33.])/32       # dyadic; no face of the grids below lies at 0

MUTATIONS = ('r_cell halved', 'band [0, n)', 'upper neighbour late', 'lower neighbour late',
             'last cy skipped', 'last cz skipped', 'last x cell dropped', 'y and z swapped',
             'lower clamp at 1')

Grid = namedtuple('Grid', 'h max_cells origin pad', defaults=(None, None, None, (0, 0, 0)))
Case = namedtuple('Case', 'points dr grid rows hits misses name family ordinary info')
Walk = namedtuple('Walk', 'counts cells widths')


class GridIndex:
    """What ``DensityIndex`` holds, for a caller-chosen edge: ``points`` sorted by cell,
    ``cell_start`` (int32, ncells + 1), ``origin``, ``h``, ``dr``, ``dims``, ``order`` and
    ``scatter``; ``args`` are the arguments of ``ctx.density_set``."""

    def __init__(self, points, dr, h, origin=None, pad=(0, 0, 0)):
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        assert len(points) and np.isfinite(points).all()
        assert h >= dr*CELL_SLACK
        origin = points.min(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
        assert origin.shape == (3,) and (origin <= points.min(axis=0)).all()
        cell = np.floor((points - origin) * (1.0 / h)).astype(np.int64)
        dims = tuple(int(v) + int(p) for v, p in zip(cell.max(axis=0) + 1, pad))
        ncells = dims[0]*dims[1]*dims[2]
        assert ncells <= 1 << 24
        linear = (cell[:, 2]*dims[1] + cell[:, 1])*dims[0] + cell[:, 0]
        order = np.argsort(linear, kind='stable')
        counts = np.bincount(linear, minlength=ncells)
        self.dr, self.h, self.origin, self.dims = float(dr), float(h), origin, dims
        self.order = order
        self.points = np.ascontiguousarray(points[order])
        self.cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        assert len(self.cell_start) == ncells + 1 and self.cell_start[-1] == len(points)

    @property
    def args(self):
        return self.points, self.cell_start, self.origin, self.h, self.dr, self.dims

    def scatter(self, values, size):
        out = np.zeros(size)
        out[self.order] = values
        return out


def grid_index(points, dr, h, origin=None, pad=(0, 0, 0)):
    return GridIndex(points, dr, h, origin, pad)


def product_index(points, dr, max_cells, monkeypatch):
    """``DensityIndex(points, dr)`` with the module's ``MAX_CELLS`` set to ``max_cells``."""
    module = importlib.import_module('nexoclom_amd.ModelDensity')
    with monkeypatch.context() as patch:
        patch.setattr(module, 'MAX_CELLS', max_cells)
        return module.DensityIndex(points, dr)


def build_index(case, monkeypatch):
    if case.grid.max_cells is not None:
        return product_index(case.points, case.dr, case.grid.max_cells, monkeypatch)
    return grid_index(case.points, case.dr, case.grid.h, case.grid.origin, case.grid.pad)


def index_args(index):
    """(points, cell_start, origin, h, dr, dims) of an index object, or the tuple itself."""
    if hasattr(index, 'cell_start'):
        return index.points, index.cell_start, index.origin, index.h, index.dr, index.dims
    return index


def candidate_cells(index, p):
    """The cells k_density visits for a row at p (restated from nxc_kernels.hpp density_cells):
    per axis the row's cell and the neighbour on each side it is within dr/h (+ 1e-6) of."""
    r_cell = index.dr / index.h + 1e-6
    ranges = []
    for a in range(3):
        t = (p[a] - index.origin[a]) * (1.0 / index.h)
        if not (-1.0 <= t < index.dims[a] + 1.0):
            return []
        c = np.floor(t)
        f = t - c
        lo = int(c) - 1 if f <= r_cell else int(c)
        hi = int(c) + 1 if f >= 1.0 - r_cell else int(c)
        ranges.append(range(max(lo, 0), min(hi, index.dims[a] - 1) + 1))
    nx, ny, _ = index.dims
    return [(cz*ny + cy)*nx + cx for cz in ranges[2] for cy in ranges[1] for cx in ranges[0]]


def restated_cells(index, rows, mutate=None):
    """density_cells for every row: (live (P,), lo (P, 3), hi (P, 3))."""
    _, _, origin, h, dr, dims = index_args(index)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(dims, dtype=np.float64)
    inv_h = 1.0 / h
    r_cell = dr / h + 1e-6
    if mutate == 'r_cell halved':
        r_cell = 0.5*r_cell
    with np.errstate(invalid='ignore', over='ignore'):
        t = (rows - np.asarray(origin, dtype=np.float64)) * inv_h
        if mutate == 'band [0, n)':
            inside = (t >= 0.0) & (t < n)
        else:
            inside = (t >= -1.0) & (t < n + 1.0)
    live = inside.all(axis=1)
    t = np.where(live[:, None], t, 0.0)
    c = np.floor(t)
    f = t - c
    ci = c.astype(np.int64)
    lower = f < r_cell - 1e-3 if mutate == 'lower neighbour late' else f <= r_cell
    upper = f > 1.0 - r_cell + 1e-3 if mutate == 'upper neighbour late' else f >= 1.0 - r_cell
    lo = np.where(lower, ci - 1, ci)
    hi = np.where(upper, ci + 1, ci)
    lo = np.maximum(lo, 1 if mutate == 'lower clamp at 1' else 0)
    hi = np.minimum(hi, np.asarray(dims, dtype=np.int64) - 1)
    live &= (lo <= hi).all(axis=1)
    return live, lo, hi


def restated_walk(index, rows, mutate=None, max_pairs=4_000_000):
    """The walk of the density kernels in NumPy: density_cells, then per (cy, cz) of a row's
    cells the candidates cell_start[row + lo0] .. cell_start[row + hi0 + 1] with row =
    (cz ny + cy) nx, and the membership (dx*dx + dy*dy) + dz*dz <= dr*dr with d = q - p.
    ``Walk``: hits per indexed point (the index's order), the number of cells each row visits
    (0 for a culled row) and the cells per axis (P, 3).  ``mutate``: one of ``MUTATIONS``; they
    only leave cells out (or permute them), so nothing reads out of range."""
    assert mutate is None or mutate in MUTATIONS
    points, cell_start, _, _, dr, dims = index_args(index)
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cs = np.asarray(cell_start, dtype=np.int64)
    nx, ny, nz = (int(v) for v in dims)
    assert len(cs) == nx*ny*nz + 1
    live, lo, hi = restated_cells(index, rows, mutate)
    widths = np.where(live[:, None], hi - lo + 1, 0)
    cells = widths.prod(axis=1)
    hi1 = hi[:, 1] - (mutate == 'last cy skipped')
    hi2 = hi[:, 2] - (mutate == 'last cz skipped')
    dr2 = dr*dr
    counts = np.zeros(len(points), dtype=np.int64)
    for dz, dy in itertools.product(range(3), range(3)):
        cz, cy = lo[:, 2] + dz, lo[:, 1] + dy
        at = np.flatnonzero(live & (cz <= hi2) & (cy <= hi1))
        if len(at) == 0:
            continue
        cz, cy = cz[at], cy[at]
        base = (cy*nz + cz)*nx if mutate == 'y and z swapped' else (cz*ny + cy)*nx
        j = cs[base + lo[at, 0]]
        e = cs[base + hi[at, 0] + (0 if mutate == 'last x cell dropped' else 1)]
        length = np.maximum(e - j, 0)
        step = max(1, max_pairs // max(1, int(length.max())))
        for a in range(0, len(at), step):
            ln = length[a:a + step]
            total = int(ln.sum())
            if total == 0:
                continue
            lane = np.repeat(np.arange(len(ln)), ln)
            q = np.arange(total) - np.repeat(np.cumsum(ln) - ln, ln) + j[a:a + step][lane]
            d = points[q] - rows[at[a:a + step]][lane]
            with np.errstate(invalid='ignore', over='ignore'):
                hit = (d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2] <= dr2
            counts += np.bincount(q[hit], minlength=len(points))
    return Walk(counts, cells, widths)


def brute_counts(points, dr, rows):
    """Hits per point by the kernel's expression over every row."""
    rows = np.asarray(rows, dtype=np.float64)
    counts = np.zeros(len(points), dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for k, q in enumerate(np.asarray(points, dtype=np.float64)):
            d = q - rows
            counts[k] = np.count_nonzero((d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2]
                                         <= dr*dr)
    return counts


def pair_hits(case, pairs):
    """The membership expression for planted (point, row) pairs."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    d = case.points[pairs[:, 0]] - case.rows[pairs[:, 1]]
    return (d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1]) + d[:, 2]*d[:, 2] <= case.dr*case.dr


def coord_at(o, inv_h, target, dtype=np.float64):
    """The smallest number p of ``dtype`` whose cell coordinate (p - o) * inv_h, formed in fp64
    as the kernel forms it, is >= target: p lies on the face, the number below p under it."""
    def t(p):
        return (np.float64(p) - o) * inv_h
    up = dtype(np.inf)
    p = dtype(o + target/inv_h)
    for _ in range(4096):              # p - o rounds: many p share one cell coordinate
        if t(p) < target:
            p = np.nextafter(p, up)
        elif t(np.nextafter(p, -up)) >= target:
            p = np.nextafter(p, -up)
        else:
            return p
    raise AssertionError('no face near o + target / inv_h')


def narrowed(a):
    """float64 values that float32 holds."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def make_case(name, points, grid, rows, hits=(), misses=(), family=None, ordinary=None, **info):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    ordinary = np.ones(len(rows), dtype=bool) if ordinary is None else np.asarray(ordinary)
    return Case(np.asarray(points, dtype=np.float64).reshape(-1, 3), DR, grid, rows,
                np.asarray(hits, dtype=np.int64).reshape(-1, 2),
                np.asarray(misses, dtype=np.int64).reshape(-1, 2), name, family or name,
                ordinary, info)


# -- coarse ----------------------------------------------------------------------------------
COARSE_EDGES = (CELL_SLACK, 1.25, 1.5, 1.999, 2.0, 3.7, 16.0)
COARSE_CAPS = (4096, 64, 8, 1)


@functools.lru_cache(maxsize=None)
def coarse_sets():
    rng = np.random.default_rng(41)
    return rng.uniform(-1, 1, (600, 3)), rng.uniform(-1.2, 1.2, (60_000, 3))


def coarse(ratio=None, max_cells=None):
    """600 random points in [-1, 1]^3 against 60 000 rows in [-1.2, 1.2]^3, on a grid of edge
    ``ratio`` dr (grid_index) or on the product's grid under ``max_cells``."""
    points, rows = coarse_sets()
    if max_cells is not None:
        return make_case(f'coarse cap={max_cells}', points, Grid(max_cells=max_cells), rows,
                         family='coarse')
    name = 'coarse h/dr=1+2^-20' if ratio == CELL_SLACK else f'coarse h/dr={ratio:g}'
    return make_case(name, points, Grid(h=ratio*DR), rows, family='coarse')


# -- faces -----------------------------------------------------------------------------------
def faces(ratio, dtype=np.float64):
    """Per axis: a point on the face between cells 1 and 2 (the smallest number of cell 2, f = 0)
    with rows below the face, and the number under it (in cell 1) with rows above the face.  The
    rows lie at dr from their point along the axis, at dr (1 +- 2^-30), and one number of
    ``dtype`` further from and nearer to it than the first.  Meant to hit: the row at
    dr (1 - 2^-30), meant to miss: the one at dr (1 + 2^-30); planted in float32, where those two
    round to the first, the nearer and the further number.  (One number of float64 is less than
    the rounding of q - p where the row is the smaller of the two, so it decides nothing.)"""
    h = ratio*DR
    inv_h = 1.0/h
    points, rows, hits, misses = [], [], [], []
    for a, side in itertools.product(range(3), (-1, 1)):
        b, c = (a + 1) % 3, (a + 2) % 3
        face = float(coord_at(ORIGIN[a], inv_h, 2.0))
        q = np.empty(3)
        q[a] = face if side < 0 else np.nextafter(face, -np.inf)
        q[b] = narrowed(ORIGIN[b] + (3*len(points) + 1.5)*h)
        q[c] = narrowed(ORIGIN[c] + 1.5*h)
        assert np.floor((q[a] - ORIGIN[a])*inv_h) == (2 if side < 0 else 1)
        first = dtype(q[a] + side*DR)
        along = [first, dtype(q[a] + side*DR*(1 + 2.0**-30)), dtype(q[a] + side*DR*(1 - 2.0**-30)),
                 np.nextafter(first, dtype(side*np.inf)), np.nextafter(first, dtype(-side*np.inf))]
        for n, v in enumerate(along):
            row = q.copy()
            row[a] = float(v)
            assert np.floor((row[a] - ORIGIN[a])*inv_h) != np.floor((q[a] - ORIGIN[a])*inv_h)
            if n == (1 if dtype is np.float64 else 3):
                misses.append((len(points), len(rows)))
            if n == (2 if dtype is np.float64 else 4):
                hits.append((len(points), len(rows)))
            rows.append(row)
        points.append(q)
    return make_case(f'faces h/dr={ratio:g} {np.dtype(dtype).name}', points,
                     Grid(h=h, origin=ORIGIN), rows, hits, misses)


# -- corners ---------------------------------------------------------------------------------
CORNER_DIMS = (5, 3, 2)


def corners(ratio, dtype=np.float64):
    """Grid 5 x 3 x 2 with 0 to 3 filler points per cell.  For each of the 26 directions s a point
    0.05 h inside the neighbouring cell across the face, edge or corner towards s, and two rows
    in the home cell on the line through it along s: 0.999 dr from it (a hit) and 1.001 dr (a
    miss)."""
    h = ratio*DR
    rng = np.random.default_rng(43)
    points, rows, hits, misses = [], [], [], []
    for cell in range(30):
        at = np.array([cell % 5, (cell // 5) % 3, cell // 15])
        for _ in range(cell % 4):
            points.append(ORIGIN + (at + rng.uniform(0.2, 0.8, 3))*h)
    for n, s in enumerate(itertools.product((-1, 0, 1), repeat=3)):
        if s == (0, 0, 0):
            continue
        s = np.array(s)
        u = s/np.linalg.norm(s)
        home = np.array([1 + n % 3, 1, 0 if s[2] > 0 else 1 if s[2] < 0 else n % 2])
        q = ORIGIN + (home + 0.5)*h
        for a in np.flatnonzero(s):
            q[a] = ORIGIN[a] + (home[a] + (s[a] > 0))*h + s[a]*0.05*h
        assert np.array_equal(np.floor((q - ORIGIN)/h), home + s)
        for scale, bucket in ((0.999, hits), (1.001, misses)):
            row = (q - scale*DR*u).astype(dtype).astype(np.float64)
            assert np.array_equal(np.floor((row - ORIGIN)/h), home)
            bucket.append((len(points), len(rows)))
            rows.append(row)
        points.append(q)
    box = np.array(CORNER_DIMS)*h
    rows += list(narrowed(ORIGIN - h + rng.uniform(0, 1, (300, 3))*(box + 2*h)))
    return make_case(f'corners h/dr={ratio:g} {np.dtype(dtype).name}', points,
                     Grid(h=h, origin=ORIGIN), rows, hits, misses)


# -- grid edges ------------------------------------------------------------------------------
def edge_case(name, points, ratio, origin=None, pad=(0, 0, 0), dtype=np.float64):
    """Rows along each axis through each point (its other two coordinates kept, so the planted
    distance is the one along the axis; points and rows are numbers float32 holds): at t = -1 and the number under it, in [-1, 0), at
    t = n and in [n, n + 1), under t = n + 1 and at it; and 200 random rows about the grid.
    ``info['outside']``: planted hits by (axis, side) of rows outside the grid."""
    h = ratio*DR
    inv_h = 1.0/h
    points = narrowed(points).reshape(-1, 3)
    index = grid_index(points, DR, h, origin, pad)
    o, dims = index.origin, index.dims
    rows, hits, misses, outside = [], [], [], {}
    down = dtype(-np.inf)
    for a in range(3):
        n = dims[a]
        low, top, past = (coord_at(o[a], inv_h, v, dtype) for v in (-1.0, float(n), n + 1.0))
        along = [low, np.nextafter(low, down), top, np.nextafter(top, down), past,
                 np.nextafter(past, down)]
        along += [dtype(o[a] + t*h) for t in (-0.75, -0.3, -2.0**-30, n + 2.0**-30, n + 0.3, n + 0.75)]
        for k, q in enumerate(points[:16]):
            for v in along:
                row = q.copy()
                row[a] = float(v)
                t = (row[a] - o[a])*inv_h
                apart = abs(row[a] - q[a])
                if apart < 0.99*DR:
                    hits.append((k, len(rows)))
                    if t < 0 or t >= n:
                        side = (a, -1 if t < 0 else 1)
                        outside[side] = outside.get(side, 0) + 1
                elif apart > 1.01*DR:
                    misses.append((k, len(rows)))
                rows.append(row)
    for k, q in enumerate(points[:16]):                    # and one row half a radius from each point
        hits.append((k, len(rows)))
        rows.append(narrowed(q + [0.5*DR, 0., 0.]))
    rng = np.random.default_rng(47)
    box = np.array(dims)*h
    rows += list(np.asarray(o - 1.5*h + rng.uniform(0, 1, (200, 3))*(box + 3*h), dtype=dtype))
    return make_case(f'edges {name} h/dr={"1+2^-20" if ratio == CELL_SLACK else f"{ratio:g}"} '
                     f'{np.dtype(dtype).name}', points,
                     Grid(h=h, origin=None if origin is None else o, pad=pad), rows, hits, misses,
                     outside=outside, dims=dims)


def box_points(h, dims=(4, 3, 2), origin=ORIGIN):
    """A point 0.1 h inside each of the grid's eight corners, and three more inside."""
    ends = [(0.1, n - 0.1) for n in dims]
    t = [list(v) for v in itertools.product(*ends)] + [[1.5, 1.2, 0.7], [2.4, 0.5, 1.5], [0.6, 2.5, 1.1]]
    return origin + np.array(t)*h


EDGE_NAMES = ('box 1+2^-20', 'box 1.5', 'box 2', 'collinear 1+2^-20', 'collinear 2', 'coplanar 1.5',
              'single 1+2^-20', 'single 2', 'duplicates 2', 'padded 1.5', 'padded 2')


def grid_edges(which, dtype=np.float64):
    name, ratio = which.split()
    ratio = CELL_SLACK if ratio == '1+2^-20' else float(ratio)
    h = ratio*DR
    if name == 'box':
        return edge_case(name, box_points(h), ratio, ORIGIN, dtype=dtype)
    if name == 'collinear':                                          # dims n x 1 x 1
        pts = ORIGIN + np.array([[0.1 + 0.7*i, 0.5, 0.5] for i in range(6)])*h
        return edge_case(name, pts, ratio, ORIGIN, dtype=dtype)
    if name == 'coplanar':                                           # dims n x m x 1
        pts = ORIGIN + np.array([[0.1 + 0.8*i, 0.9 + 0.6*j, 0.5] for i in range(4) for j in range(3)])*h
        return edge_case(name, pts, ratio, ORIGIN, dtype=dtype)
    if name == 'single':                      # dims 1 x 1 x 1; the grid's origin is the point (f = 0)
        return edge_case(name, ORIGIN + np.array([[0.3, 0.3, 0.3]]), ratio, dtype=dtype)
    if name == 'duplicates':                  # dims 1 x 1 x 1, f = 0.9
        pts = np.repeat(ORIGIN + np.array([[0.9, 0.9, 0.9]])*h, 5, axis=0)
        return edge_case(name, pts, ratio, ORIGIN, dtype=dtype)
    assert name == 'padded'                   # empty first cells (a lower origin) and last cells (pad)
    return edge_case(name, box_points(h), ratio, ORIGIN - np.array([2, 1, 3])*h, pad=(2, 1, 3),
                     dtype=dtype)


# -- ragged ----------------------------------------------------------------------------------
RAGGED_NAMES = ('lane 0', 'lane 31', 'lane 63', 'corners 3x3x3', 'corners 2x2x2', 'one point')


def ragged(which):
    """One wave of 64 rows whose lanes walk candidate lists of very different lengths."""
    rng = np.random.default_rng(53)
    if which.startswith('lane'):
        # h = 2 dr, dims 6 x 4 x 3: 3000 points in cell (1, 1, 1); lane k sits at its centre
        # (f = 0.5: 27 cells) and the others near three sparse points, among empty cells, or
        # outside the grid
        k, h = int(which.split()[1]), 2*DR
        centre = ORIGIN + 1.5*h
        dense = centre + rng.uniform(-0.45, 0.45, (3000, 3))*h
        sparse = ORIGIN + (np.array([4, 2, 1]) + rng.uniform(0.3, 0.7, (3, 3)))*h
        points = np.concatenate([dense, sparse, [ORIGIN + (np.array([5, 3, 2]) + 0.5)*h]])
        rows, hits = [], []
        for lane in range(64):
            if lane == k:
                rows.append(centre)
            elif lane % 3 == 0:
                hits.append((3000 + lane % 2, lane))
                rows.append(sparse[lane % 2] + rng.normal(0, 0.1*DR, 3))
            elif lane % 3 == 1:
                rows.append(ORIGIN + (np.array([3, 0, 0]) + 0.5)*h)
            else:
                rows.append(ORIGIN - 3*h + rng.uniform(0, 1e-3, 3))
        return make_case(f'ragged {which}', points, Grid(h=h, origin=ORIGIN), rows, hits, lane=k)
    if which.startswith('corners'):
        # a row whose block of cells holds points only in corner cells, none of them in the
        # block's last (cy, cz) range: advance() crosses empty ranges between full ones and ends
        # on an empty one.  Odd lanes sit in a block without any point.
        wide = which.endswith('3x3x3')
        h, f, home = (1.5*DR, 0.35, np.array([2, 2, 2])) if wide else (2*DR, 0.2, np.array([2, 2, 2]))
        steps = (-1, 1) if wide else (-1, 0)
        points = []
        for n, s in enumerate(itertools.product(steps, repeat=3)):
            if s[1] == steps[1] and s[2] == steps[1]:
                continue                                        # the last (cy, cz) range stays empty
            if not wide and s[1:] == (steps[1], steps[0]):
                continue                                        # and so does the second
            cell = home + np.array(s)
            if s == (-1, -1, -1):                               # 0.02 h inside its far corner: a hit
                points.append(ORIGIN + (cell + 0.98)*h)
            else:
                points += list(ORIGIN + (cell + rng.uniform(0.1, 0.9, (2 + n % 4, 3)))*h)
        rows, hits = [], []
        for lane in range(64):
            if lane % 2 == 0:
                rows.append(ORIGIN + (home + f + lane*1e-5)*h)
                hits.append((0, lane))
            else:
                rows.append(ORIGIN + (np.array([6, 2, 2]) + 0.5)*h)
        # (2x2x2: no point has the home cell's cy, so one padded cell along y as well)
        return make_case(f'ragged {which}', points,
                         Grid(h=h, origin=ORIGIN, pad=(4, 0 if wide else 1, 0)), rows, hits,
                         block=3 if wide else 2)
    assert which == 'one point'
    point = ORIGIN + 0.3
    rows = point + rng.normal(0, 0.2*DR, (64, 3))
    return make_case('ragged one point', [point], Grid(h=2*DR), rows, [(0, k) for k in range(64)])


# -- non-finite rows -------------------------------------------------------------------------
def nonfinite(ratio):
    """NaN, +inf, -inf and +-1e300 in each position column of a row that would otherwise hit its
    point, mixed into a wave of ordinary rows."""
    rng = np.random.default_rng(59)
    points = rng.uniform(-0.5, 0.5, (40, 3))
    near = rng.integers(0, 40, 113)
    rows = points[near] + rng.normal(0, 0.4*DR, (113, 3))
    ordinary = np.ones(128, dtype=bool)
    bad = np.arange(15)*8 + 3                                   # spread over both waves
    ordinary[bad] = False
    out = np.empty((128, 3))
    out[ordinary] = rows
    values = (np.nan, np.inf, -np.inf, 1e300, -1e300)
    for n, at in enumerate(bad):
        out[at] = points[n]
        out[at, n // 5] = values[n % 5]
    name = f'nonfinite h/dr={"1+2^-20" if ratio == CELL_SLACK else f"{ratio:g}"}'
    return make_case(name, points, Grid(h=ratio*DR), out, ordinary=ordinary)


# -- the registry ----------------------------------------------------------------------------
def _registry():
    reg = {}

    def add(case_name, builder, *args):
        reg[case_name] = (builder, args)
    for ratio in COARSE_EDGES:
        add(coarse(ratio).name, coarse, ratio)
    for cap in COARSE_CAPS:
        add(f'coarse cap={cap}', coarse, None, cap)
    for ratio in (2.0, 3.7):
        add(f'faces h/dr={ratio:g}', faces, ratio)
    for ratio in (1.5, 2.0, 3.7):
        add(f'corners h/dr={ratio:g}', corners, ratio)
    for which in EDGE_NAMES:
        add(f'edges {which}', grid_edges, which)
    for which in RAGGED_NAMES:
        add(f'ragged {which}', ragged, which)
    for ratio in (CELL_SLACK, 2.0):
        add(nonfinite(ratio).name, nonfinite, ratio)
    return reg


REGISTRY = _registry()
CASE_NAMES = tuple(REGISTRY)
FLOAT32_NAMES = tuple(n for n in CASE_NAMES if n.split()[0] in ('faces', 'corners', 'edges'))


@functools.lru_cache(maxsize=None)
def case(name, dtype=np.float64):
    """The case of that name (``CASE_NAMES``); ``dtype``: what its rows are planted in (the
    ``FLOAT32_NAMES`` take float32)."""
    builder, args = REGISTRY[name]
    if dtype is np.float64:
        return builder(*args)
    assert name in FLOAT32_NAMES
    return builder(*args, dtype=dtype)
