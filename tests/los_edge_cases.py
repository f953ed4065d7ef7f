"""Constructed inputs of the line-of-sight edge tests (tests/test_gpu_los_edges.py; their layouts are
also what tests/test_los_blocks_cpu.py checks the restated block formation on).  NumPy only.

LAYOUTS: index columns by name, as lists of packet lengths.
cloud(): the rows of a layout as a compact ball of samples outside the planet's shadow (y < 0).
lines_of_sight(): spacecraft around that ball; "hot" ones look at it, "cold" ones away from it."""
import functools

import numpy as np

ONE_PACKET = (1, 7, 8, 9, 255, 256, 257, 511, 512, 513)
B2B = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)


def _mixed():
    # packets of 1 to 40 rows, 769 rows = three regions and one row
    lens = np.random.default_rng(40).integers(1, 41, 80).tolist()
    out = []
    while sum(out) < 769:
        out.append(lens[len(out)])
    out[-1] -= sum(out) - 769
    return out


def _region_tail():
    # 20-row packets that start at positions 247, 248 and 255 of regions 0, 1 and 2: the region's
    # end cuts them after 9 rows (more than a block: a fresh group), 8 rows (exactly a block: none)
    # and 1 row.  Packets of three rows in between, so that no block before them ends on a group's
    # last slot -- there a fresh group would take the very next slot anyway.
    def fill(n):
        return [3]*(n//3) + ([n % 3] if n % 3 else [])
    return fill(247) + [20] + fill(256 + 248 - 267) + [20] + fill(512 + 255 - 524) + [20]


LAYOUTS = {f'one-{p}': [p] for p in ONE_PACKET}
LAYOUTS.update({
    'b2b': list(B2B),                       # packets straddle the region edges at 256, 512, ...
    'b2b-rev': list(B2B[::-1]),
    'singles': [1]*300,                     # a slot per row: 256 slots a region, the densest stream
    'nines': [9]*170 + [7],                 # every packet opens a group: the most padding
    # packet starts on each of a lane's four rows, short packets and long; several starts in one
    # lane's rows; a run of 8 after an odd number of blocks
    'lane-starts': [5, 5, 5, 5, 1, 2, 1, 3, 9, 10, 11, 13, 1, 1, 1, 1, 8, 8, 12, 2, 17, 3, 16, 4, 33]*2,
    'region-tail': _region_tail(),
    'mixed': _mixed(),
})
# layouts of three regions and one row whose packets straddle every region edge: with slabs of 256
# rows the last slab has one row
SLAB_LAYOUTS = {'one-513': 513, 'b2b': 1537, 'b2b-rev': 1537, 'nines': 1537, 'mixed': 769}


def layout_ids(name, rows=None):
    """The index column of a layout (int64), cut to its first `rows` rows."""
    lens = LAYOUTS[name]
    return np.repeat(np.arange(len(lens), dtype=np.int64), lens)[:rows]


CENTRE = np.array([0.0, -3.0, 0.0])     # of the ball of samples: foot points with y < 0 are lit
BALL = 0.22                             # packets start inside this radius ...
WIGGLE = 0.03                           # ... and stay within sqrt(3) x this of their start
DISTANCE = 5.0                          # spacecraft from the ball's centre
DPHI = np.radians(5.0)                  # the ball (0.272 at 5: 3.1 degrees) fits a cone aimed 1 degree off
OUTEREDGE = 25.0


def cloud(ids, seed=0):
    """Rows of an index column as samples: dict(x, y, z, vy, frac) of float64 columns.  A packet is
    a short smooth curve inside the ball; the rows' frac are all different, so that a row taken
    for another changes the radiance."""
    ids = np.asarray(ids)
    P = len(ids)
    rng = np.random.default_rng(1000 + seed)
    npk = int(ids.max()) + 1
    d = rng.normal(size=(npk, 3))
    start = d/np.linalg.norm(d, axis=1)[:, None]*(BALL*rng.uniform(0, 1, npk)**(1/3))[:, None]
    phase = rng.uniform(0, 2*np.pi, npk)
    first = np.r_[0, np.nonzero(ids[1:] != ids[:-1])[0] + 1]
    k = np.arange(P) - np.repeat(first, np.diff(np.r_[first, P]))
    ph = phase[ids]
    pts = CENTRE + start[ids] + WIGGLE*np.stack([np.sin(0.2*k + ph), np.cos(0.17*k + ph),
                                                 np.sin(0.31*k + 2*ph)], 1)
    frac = (rng.permutation(P) + 1.0)/(P + 1.0)
    vy = rng.normal(0, 2e-3, P)
    return dict(x=np.ascontiguousarray(pts[:, 0]), y=np.ascontiguousarray(pts[:, 1]),
                z=np.ascontiguousarray(pts[:, 2]), vy=vy, frac=frac)


def lines_of_sight(S, hot, seed=0):
    """S spacecraft at DISTANCE from the ball's centre, none of them nearer the planet's centre in
    y than the ball (the planet is never between them and the ball).  Those listed in `hot` look
    at the ball: the first of them and every second one after it at most 1 degree off its centre
    (the whole ball is inside the cone), the others 4 degrees off (they see a part of it).  The
    rest look away from it.  Returns (pos (S, 3), look (S, 3)), unit boresights."""
    rng = np.random.default_rng(2000 + seed)
    u = rng.normal(size=(S, 3))
    u[:, 1] = -np.abs(u[:, 1])
    u /= np.linalg.norm(u, axis=1)[:, None]
    pos = CENTRE + DISTANCE*u
    look = u + 0.5*rng.normal(size=(S, 3))                  # cold: away, within a wide scatter
    look[np.sum(look*u, axis=1) < 0.2] = u[np.sum(look*u, axis=1) < 0.2]
    for n, i in enumerate(hot):
        t = rng.normal(size=3)
        t -= np.dot(t, u[i])*u[i]
        t /= np.linalg.norm(t)
        off = np.radians(rng.uniform(0, 1.0) if n % 2 == 0 else 4.0)
        look[i] = -np.cos(off)*u[i] + np.sin(off)*t
    look /= np.linalg.norm(look, axis=1)[:, None]
    return pos, look


@functools.lru_cache(maxsize=None)
def forces():
    from tests import helpers as H
    return H.mercury_forces('Na', 1.3)


@functools.lru_cache(maxsize=None)
def g_tables(lines):
    from tests import helpers as H
    f = forces()
    return H.g_tables('Na', f.aplanet, f.R_km, lines)
