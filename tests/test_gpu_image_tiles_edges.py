"""The tiled stored-sample image (k_image_bin + k_image_tiles) at its chunk, trip, producer and slab
edges, on a few thousand samples and images of a few hundred pixels.

Every expectation is constructed: the samples sit at pixel centres, so the test knows how many land
in which pixel.  Column images take weights k/1024 (1 <= k <= 1024): every partial sum of at most
2^13 of them is a double (and each term a float), so the weight image equals the exact sum bit for
bit in whatever order the device adds -- one lost, doubled or stale entry shows.  Radiance images
are compared with the NumPy oracle (rtol 1e-12: at most 4096 samples per pixel, so the order of the
additions stays below 4095 x 2^-53 = 4.6e-13) and with the atomic path.

Every case first asserts, from the restated plan (tests/tile_plan_restatement.py, tied to the C++
by tests/test_tile_plan_cpu.py), the structure it means to hit: producers, chunks per (producer,
tile) list, the fill of the last chunk, slabs."""
import functools

import numpy as np
import pytest

from oracle import np_oracle as O
from tests import helpers as H
from tests import tile_plan_restatement as TP

pytestmark = pytest.mark.gpu

# nxc_tile_plan.hpp, nxc_tile_per_trip: NXC_TILE_BIN_BLOCK (1024 threads) x nxc_tile_unroll (4
# float32 samples, 2 of 64 bits) -- what a producer takes between two pairs of barriers
PER_TRIP = {4: 4096, 8: 2048}
# nxc_tile_plan.hpp, tile_plan: cap = min(256, NXC_TILE_STAGE >> lg), lg the smallest with
# ceil(nx / 2^lg) <= tile_pixels / nz.  (nx, nz, tile_pixels) that reach each chunk size with one
# image row per tile:
GEO = {256: (32, 8, 8), 128: (64, 8, 8), 64: (128, 8, 8)}
# nxc_tile_plan.hpp, tile_slabs: a producer owns samples [k span, (k + 1) span) of a slab, and
# span = per_trip as long as the slab holds at most per_trip x (workgroups the chip holds); the
# cases here need four producers at most, and a chip holds one per CU at least
MAX_PRODUCERS = 4
# sizeof(LdsHeader) rounded to 32 (NXC_HEADER_BYTES, nxc_device.hpp): the image tables staged by
# the stored-sample kernels are this header + [g-value tables | edges]
LDS_HEADER = 4224

# The four <T, DEFER> forms of k_image_bin (image_run, nxc_api.hip: defer = float32 values &&
# nxc_tile_room(img_bytes)), and the set-up that reaches each:
#   f64          <double, non-DEFER>  float64 columns, no down-cast
#   f32          <float, DEFER>       float32 columns
#   f64_cast     <double, DEFER>      float64 columns holding float32 values, downcast_f32
#   f32_lines4   <float, DEFER> with pass 2 forming radiances: the four emission lines (3303, 5891,
#                5897, 5891) are 53 200 bytes of tables (the 3303 table has 49 points), which DO
#                leave room for a tile beside them
#   f32_no_room  <float, non-DEFER>   four tables of 389 points (5891, 5897, 5891, 5897): 66 560
#                bytes, beyond the 65 536 that nxc_tile_room leaves whatever the header
ROUTES = {
    'f64': dict(bytes=8, dtype=np.float64, quantity='column', downcast=False, lines=()),
    'f32': dict(bytes=4, dtype=np.float32, quantity='column', downcast=False, lines=()),
    'f64_cast': dict(bytes=8, dtype=np.float64, quantity='column', downcast=True, lines=()),
    'f32_lines4': dict(bytes=4, dtype=np.float32, quantity='radiance', downcast=False,
                       lines=(3303, 5891, 5897, 5891)),
    'f32_no_room': dict(bytes=4, dtype=np.float32, quantity='radiance', downcast=False,
                        lines=(5891, 5897, 5891, 5897)),
}
COLUMN_ROUTES = ['f64', 'f32', 'f64_cast']
ALL_ROUTES = list(ROUTES)
RADIANCE_CAP = 4096           # samples per pixel at most where the oracle's sum is the reference


@pytest.fixture
def tiles(ctx):
    """Leaves the context in its default mode whatever the test did."""
    yield ctx
    ctx.image_mode('auto')


@functools.lru_cache(maxsize=None)
def _forces():
    return H.mercury_forces('Na', 1.3)


@functools.lru_cache(maxsize=None)
def _radiance_view(nx, nz, lines, sublon, sublat):
    """An image whose pixel (ix, iz) is the unit square at (ix, iz) of the observer's plane."""
    return H.image_setup(_forces(), 'radiance', dims=(nx, nz), center=(nx/2, nz/2),
                         width=(float(nx), float(nz)), sublon=sublon, sublat=sublat,
                         wavelengths=lines)


def deferred(route, nx, nz):
    """image_run's `defer` for this route and image size, from its own expression."""
    r = ROUTES[route]
    part = 0 if not r['lines'] else TP.image_part_bytes(_radiance_view(nx, nz, r['lines'], 0.0,
                                                                       np.pi/2)['g_tables'], nx, nz)
    part = part or (nx + nz + 2)*8
    f32_values = r['bytes'] == 4 or r['downcast']
    return f32_values and TP.room(LDS_HEADER + part)


def set_view(ctx, route, nx, nz, rotation=(0.0, np.pi/2)):
    """nxc_set_image for a route; returns what the sample builder and the oracle need."""
    r = ROUTES[route]
    if r['quantity'] == 'column':
        xe, ze = np.arange(nx + 1.0), np.arange(nz + 1.0)
        ctx.set_image(np.eye(3), 0.0, 1.0, 'column', xe, ze, [], downcast_f32=r['downcast'])
        return dict(M=np.eye(3), dims=(nx, nz), route=route)
    f = _forces()
    im = _radiance_view(nx, nz, r['lines'], *rotation)
    assert np.array_equal(im['xedges'], np.arange(nx + 1.0))
    assert np.array_equal(im['zedges'], np.arange(nz + 1.0))
    ctx.set_image(im['M'], f.vrplanet, im['apix'], 'radiance', im['xedges'], im['zedges'],
                  im['g_tables'])
    return dict(M=im['M'], dims=(nx, nz), route=route, im=im)


def scene(ix, iz, k=None, yo=-1.0, seed=1):
    """Samples by pixel: sample j sits at the centre of pixel (ix[j], iz[j]) at depth yo[j] of the
    observer's frame with frac = k[j] / 1024.  ix = -1 / -2: left / right of the frame; iz = -1:
    below it.  xyz_bad / frac_bad / vy_nan: overwrite the coordinates / frac with that value (0:
    leave), vy with a NaN."""
    ix = np.array(ix, dtype=np.int64)
    n = len(ix)
    rng = np.random.default_rng(seed)
    return dict(ix=ix, iz=np.zeros(n, dtype=np.int64) + np.asarray(iz, dtype=np.int64),
                k=rng.integers(1, 1025, n) if k is None else np.zeros(n, dtype=np.int64) + k,
                yo=np.zeros(n) + yo, xyz_bad=np.zeros(n), frac_bad=np.zeros(n),
                vy_nan=np.zeros(n, dtype=bool), seed=seed)


def take(s, order):
    """The same samples in another order."""
    return {key: (v[order] if isinstance(v, np.ndarray) else v) for key, v in s.items()}


def join(*scenes):
    return {key: (np.concatenate([s[key] for s in scenes]) if isinstance(v, np.ndarray) else v)
            for key, v in scenes[0].items()}


def columns(view, s):
    """The five columns the device gets, in the route's width."""
    r = ROUTES[view['route']]
    nx, nz = view['dims']
    n = len(s['ix'])
    xo = np.where(s['ix'] >= 0, s['ix'] + 0.5, np.where(s['ix'] == -1, -2.5, nx + 1.5))
    zo = np.where(s['iz'] >= 0, s['iz'] + 0.5, -2.5)
    x, y, z = (np.stack([xo, s['yo'], zo], axis=1) @ view['M']).T    # M^T obs: M is a rotation
    frac = s['k']/1024.0
    vy = np.zeros(n)
    if r['quantity'] == 'radiance':
        vy = np.random.default_rng(s['seed'] + 77).normal(size=n)*3.0/_forces().R_km
    bad = s['xyz_bad'] != 0
    x, y, z = (np.where(bad, s['xyz_bad'], c) for c in (x, y, z))
    frac = np.where(s['frac_bad'] != 0, s['frac_bad'], frac)
    vy = np.where(s['vy_nan'], np.nan, vy)
    with np.errstate(over='ignore'):
        cols = [np.ascontiguousarray(c, dtype=r['dtype']) for c in (x, y, z, vy, frac)]
    if r['downcast']:
        assert all(np.array_equal(c, c.astype(np.float32).astype(np.float64), equal_nan=True)
                   for c in cols)
    return cols


def expected(view, s):
    """Constructed counts, exact column weights, the three counters, and the image row under which
    pass 1 files each sample (-1: it is not filed)."""
    nx, nz = view['dims']
    ix, iz = s['ix'], s['iz']
    inframe = (ix >= 0) & (iz >= 0) & (s['xyz_bad'] == 0)
    finite = (s['frac_bad'] == 0) & ~s['vy_nan']
    binned = inframe & finite
    counts = np.zeros((nx, nz), dtype=np.uint64)
    np.add.at(counts, (ix[binned], iz[binned]), 1)
    hidden = ((ix + 0.5)**2 + (iz + 0.5)**2 <= 1.0) & (s['yo'] >= 0)      # behind the planet
    lit = binned & ~hidden
    weights = np.zeros((nx, nz))
    np.add.at(weights, (ix[lit], iz[lit]), s['k'][lit]/1024.0)
    assert counts.max(initial=0) <= 8192                                  # 2^13 terms: exact sums
    ctr = dict(samples=len(ix), samples_binned=int(binned.sum()), nonfinite=int((~finite).sum()))
    # (the deferred forms file every sample inside the frame; pass 2 finds the non-finite weights)
    filed = np.where(inframe if deferred(view['route'], nx, nz) else binned, ix, -1)
    return counts, weights, ctr, filed


def structure(route, geo, s, slab=0):
    """(geometry, plan, entries[slab, producer, tile]) of a call, from the restated plan."""
    nx, nz, tile_pixels = geo
    g = TP.geometry(nx, nz, tile_pixels)
    plan = TP.slabs(g, len(s['ix']), slab, MAX_PRODUCERS, ROUTES[route]['bytes'])
    assert plan['per_trip'] == PER_TRIP[ROUTES[route]['bytes']] == plan['span']
    assert plan == TP.slabs(g, len(s['ix']), slab, TP.SLOTS, ROUTES[route]['bytes'])
    view = dict(dims=(nx, nz), route=route)
    return g, plan, TP.lists(g, plan, expected(view, s)[3])


def run(ctx, route, geo, s, slab=0, rotation=(0.0, np.pi/2), calls=1):
    """set_image, `calls` tiled passes over the samples, and every check; returns what came back."""
    nx, nz, tile_pixels = geo
    view = set_view(ctx, route, nx, nz, rotation)
    cols = columns(view, s)
    counts, weights, ctr, _ = expected(view, s)
    ctx.image_mode('tiles', tile_pixels, slab)
    for _ in range(calls):
        ctx.image_accumulate(*cols)
    image, got_counts = ctx.image_download()
    got_ctr = ctx.counters()
    assert {key: got_ctr[key] for key in ctr} == ctr            # (of the last call)
    assert np.array_equal(got_counts, counts*np.uint64(calls))
    if ROUTES[route]['quantity'] == 'column':
        assert np.array_equal(image, weights*calls)
        return image, got_counts
    # radiance: the oracle over the finite samples, and the atomic path over all of them
    assert counts.max(initial=0) <= RADIANCE_CAP
    f, im = _forces(), view['im']
    c64 = [c.astype(np.float64) for c in cols]
    ok = np.isfinite(c64[0]) & np.isfinite(c64[3]) & np.isfinite(c64[4])
    ref_img, ref_cnt, _, _ = O.create_image(*(c[ok] for c in c64), f.vrplanet, im['M'], 'radiance',
                                            im['g_tables'], im['dims'], im['xrange'], im['zrange'],
                                            im['apix'], matmul=False)
    assert np.array_equal(counts, ref_cnt.astype(np.uint64))
    np.testing.assert_allclose(image, ref_img*calls, rtol=1e-12, atol=0)
    ctx.image_clear()
    ctx.image_mode('atomics')
    ctx.image_accumulate(*cols)
    image1, counts1 = ctx.image_download()
    assert got_ctr == ctx.counters()
    assert np.array_equal(counts, counts1)
    np.testing.assert_allclose(image, image1*calls, rtol=1e-12, atol=0)
    return image, got_counts


def test_each_route_reaches_its_form_of_the_binning_kernel():
    """image_run's own expression, restated: which routes leave the weight to pass 2."""
    for nx, nz, _ in GEO.values():
        assert [deferred(r, nx, nz) for r in ALL_ROUTES] == [False, True, True, True, False]
        gt = _radiance_view(nx, nz, ROUTES['f32_no_room']['lines'], 0.0, np.pi/2)['g_tables']
        assert TP.image_part_bytes(gt, nx, nz) > 64*1024                # whatever the header
        # ... and the image is not refused: pass 1's tables and staging blocks fit the LDS
        assert TP.geometry(nx, nz, 8, LDS_HEADER + TP.image_part_bytes(gt, nx, nz)) is not None


# ---- the fill ladder ----------------------------------------------------------------------------
def ladder_calls(cap, nb, nz, budget, by_tile, one_pixel, seed):
    """Calls of one producer in which tile b receives LADDER[(b + call) % 8] samples as long as
    the call's budget lasts (the tiles after that stay empty)."""
    ladder = [0, 1, cap - 1, cap, cap + 1, 2*cap - 1, 2*cap, 2*cap + 1]
    rng = np.random.default_rng(seed)
    out = []
    for call in range(8):
        ix, iz, left = [], [], budget
        for b in range(nb):
            m = ladder[(b + call) % 8]
            if m > left:
                continue
            left -= m
            ix += [b]*m
            iz += [(b + call) % nz]*m if one_pixel else [j % nz for j in range(m)]
        s = scene(ix, iz, seed=seed + call)
        out.append(s if by_tile else take(s, rng.permutation(len(ix))))
    return ladder, out


@pytest.mark.parametrize('layout', ['shuffled-spread', 'by_tile-spread', 'shuffled-one_pixel',
                                    'by_tile-one_pixel'])
@pytest.mark.parametrize('cap', [256, 128, 64])
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_fill_ladder(tiles, route, cap, layout):
    """One producer; a tile's list holds 0, 1, cap - 1, cap, cap + 1, 2 cap - 1, 2 cap or 2 cap + 1
    entries: no chunk, a partial one, exactly full ones (the nlist word's zero fill), and a full
    one followed by one entry.  In seeded random order, and sorted by tile (all lanes of a wave ask
    for the same staging block); a tile's samples in one pixel, and spread over its pixels."""
    order, spread = layout.split('-')
    geo = GEO[cap]
    g = TP.geometry(*geo)
    assert (g['cap'], g['nb'], g['tile_used']) == (cap, geo[0], geo[1])
    ladder, calls = ladder_calls(cap, g['nb'], g['nz'], PER_TRIP[ROUTES[route]['bytes']],
                                 order == 'by_tile', spread == 'one_pixel', 40 + cap)
    seen = set()
    for s in calls:
        _, plan, n = structure(route, geo, s)
        assert n.shape[:2] == (1, 1) and len(s['ix']) <= plan['per_trip']        # one producer
        seen |= set(zip(TP.chunks(n[0, 0], cap).tolist(), TP.last_fill(n[0, 0], cap).tolist()))
        if order == 'by_tile':
            assert np.all(np.diff(s['ix']) >= 0)
    assert seen == {(0, 0), (1, 1), (1, cap - 1), (1, cap), (2, 1), (2, cap - 1), (2, cap), (3, 1)}
    for s in calls:
        _, counts = run(tiles, route, geo, s)
        if spread == 'one_pixel':
            assert np.all(np.count_nonzero(counts, axis=1) <= 1)


# ---- a whole trip into one tile -----------------------------------------------------------------
@pytest.mark.parametrize('cap', [256, 128, 64])
@pytest.mark.parametrize('route', COLUMN_ROUTES)
def test_a_whole_trip_into_one_tile(tiles, route, cap):
    """p = per_trip, every sample in one image row: the row's staging block overflows and is
    emptied per_trip / cap - 1 times inside the one trip (64 retry rounds with 64-entry chunks and
    float32 samples); the list ends on a full chunk."""
    geo = GEO[cap]
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    row = geo[0] - 3
    s = scene([row]*per_trip, np.arange(per_trip) % geo[1], seed=cap)
    _, _, n = structure(route, geo, s)
    assert n.shape[:2] == (1, 1) and np.count_nonzero(n) == 1
    assert TP.chunks(n[0, 0, row], cap) == per_trip//cap and TP.last_fill(n[0, 0, row], cap) == cap
    run(tiles, route, geo, s)


# ---- ragged trips and producers -----------------------------------------------------------------
def scattered(nx, nz, p, seed, outside=0.25):
    """p samples over the pixels of the image and, a quarter of them, around it."""
    rng = np.random.default_rng(seed)
    ix = rng.integers(0, nx, p)
    iz = rng.integers(0, nz, p)
    out = rng.random(p) < outside
    ix = np.where(out, rng.choice([-1, -2, 0], p), ix)
    iz = np.where(out & (ix == 0), -1, iz)
    return scene(ix, iz, seed=seed)


def ragged_sizes(per_trip):
    return [1, 63, 64, 65, 1023, 1025, per_trip - 1, per_trip, per_trip + 1, 2*per_trip + 1]


@pytest.mark.parametrize('which', range(10))
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_ragged_trips_and_producers(tiles, route, which):
    """p = 1, 63, 64, 65, 1023, 1025, per_trip - 1, per_trip, per_trip + 1, 2 per_trip + 1 (the last
    producer then holds one sample) into 100 x 8 pixels in 128 tiles of 64-entry chunks, of which
    tiles 100..127 never receive a sample."""
    geo = (100, 8, 8)
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    p = ragged_sizes(per_trip)[which]
    s = scattered(100, 8, p, 500 + which)
    s['ix'][-1], s['iz'][-1] = 99, 7                      # the last sample is binned
    g, plan, n = structure(route, geo, s)
    assert (g['nb'], g['cap']) == (128, 64) and np.all(n[:, :, 100:] == 0)
    assert n.shape[:2] == (1, (p + per_trip - 1)//per_trip) and plan['prod'] == n.shape[1]
    if p == 2*per_trip + 1:
        assert n.shape[1] == 3 and n[0, 2].sum() == 1
    run(tiles, route, geo, s)


@pytest.mark.parametrize('route', ALL_ROUTES)
def test_a_producer_whose_whole_span_is_outside_the_image(tiles, route):
    """Three producers; every sample of the middle one falls outside the frame: its lists are all
    empty (nlist words of no chunks), between two producers with full lists."""
    geo = GEO[128]
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    s = scattered(64, 8, 2*per_trip + 1, 77)
    s['ix'][per_trip:2*per_trip] = -2
    _, _, n = structure(route, geo, s)
    assert n.shape[:2] == (1, 3) and n[0, 1].sum() == 0 and n[0, 0].sum() > per_trip//2
    run(tiles, route, geo, s)


# ---- the small images ---------------------------------------------------------------------------
@pytest.mark.parametrize('geo', [(1, 1, 0), (5, 3, 0), (37, 1, 1)])
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_small_images(tiles, route, geo):
    """1 x 1 and 5 x 3 pixels in one tile; 37 x 1 pixels in tiles of one pixel (cap as the plan
    gives it: 64 tiles, 128-entry chunks); two producers and one sample."""
    nx, nz, _ = geo
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    s = scattered(nx, nz, per_trip + 1, 900 + nx, outside=0.6 if nx == 1 else 0.25)
    g, plan, n = structure(route, geo, s)
    assert (g['nb'], g['cap'], g['tile_used']) == {1: (1, 256, 1), 5: (1, 256, 15),
                                                   37: (64, 128, 1)}[nx]
    assert n.shape[:2] == (1, 2)
    run(tiles, route, geo, s)


# ---- slabs --------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['five_of_one', 'trip_plus_one', 'trip'])
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_slabs(tiles, route, case):
    """Slabs of one sample; slabs just above and exactly at a trip.  The answers are those of one
    slab: the scratch is reused slab after slab and nothing of the last one may be read again."""
    geo = GEO[128]
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    p, slab = {'five_of_one': (5, 1), 'trip_plus_one': (3*per_trip + 5, per_trip + 1),
               'trip': (3*per_trip + 5, per_trip)}[case]
    s = scattered(64, 8, p, 1200 + len(case), outside=0.1)
    if case == 'five_of_one':
        s['ix'][:], s['iz'][:] = [3, 3, -1, 63, 3], [0, 0, 0, 7, 1]
    _, plan, n = structure(route, geo, s, slab)
    if case == 'five_of_one':
        assert plan['slab'] == 1 and n.shape[:2] == (5, 1)
        assert n.sum(axis=(1, 2)).tolist() == [1, 1, 0, 1, 1]
    else:
        # four equal slabs (the fourth a little shorter), one producer each
        assert n.shape[0] == 4 and plan['slab'] == (p + 3)//4 <= slab
        assert n.shape[1] == plan['prod'] == 1
        assert p - 3*plan['slab'] >= 1
    run(tiles, route, geo, s, slab=slab)


def test_two_producers_per_slab(tiles):
    """Slabs of per_trip + 1 samples that are not evened out: 2 (per_trip + 1) samples make two
    slabs of two producers, the second producer holding one sample."""
    geo, route = GEO[64], 'f32'
    per_trip = PER_TRIP[4]
    s = scattered(128, 8, 2*(per_trip + 1), 31, outside=0.0)
    _, plan, n = structure(route, geo, s, per_trip + 1)
    assert n.shape[:2] == (2, 2) and plan['slab'] == per_trip + 1
    assert n[:, 1].sum(axis=1).tolist() == [1, 1]
    run(tiles, route, geo, s, slab=per_trip + 1)


# ---- nothing binned -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['outside', 'nonfinite_coordinates', 'nonfinite_weights'])
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_nothing_binned(tiles, route, case):
    """All samples outside the frame; all coordinates NaN or infinite; non-finite frac or vy inside
    the frame: a zero image, zero counts, and the constructed number of non-finite samples."""
    geo = GEO[256]
    p = PER_TRIP[ROUTES[route]['bytes']] + 37
    rng = np.random.default_rng(5)
    if case == 'outside':
        s = scene(rng.choice([-1, -2], p), rng.integers(-1, 8, p))
        s['frac_bad'][::97] = np.inf                       # ... some of them not finite either
        s['vy_nan'][5::101] = True
    elif case == 'nonfinite_coordinates':
        s = scene(rng.integers(0, 32, p), rng.integers(0, 8, p))
        s['xyz_bad'][:] = rng.choice([np.nan, np.inf, -np.inf], p)
        s['frac_bad'][::89] = np.nan
    else:
        s = scene(rng.integers(0, 32, p), rng.integers(0, 8, p))
        s['frac_bad'][:] = rng.choice([np.nan, np.inf, -np.inf], p)
        s['frac_bad'][::3] = 0
        s['vy_nan'][::3] = True
    view = dict(dims=geo[:2], route=route)
    counts, weights, ctr, filed = expected(view, s)
    assert counts.sum() == 0 and weights.sum() == 0 and ctr['samples_binned'] == 0
    assert ctr['nonfinite'] == {'outside': len(s['ix'][::97]) + len(s['ix'][5::101]) -
                                len(set(range(0, p, 97)) & set(range(5, p, 101))),
                                'nonfinite_coordinates': len(s['ix'][::89]),
                                'nonfinite_weights': p}[case]
    # only the deferred forms file anything: the samples whose weight pass 2 finds non-finite
    assert (filed >= 0).sum() == (p if case == 'nonfinite_weights' and deferred(route, 32, 8) else 0)
    image, _ = run(tiles, route, geo, s)
    assert not image.any()


# ---- zero weights -------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_zero_weights_are_counted(tiles, route):
    """Samples behind the planet (x^2 + z^2 <= 1 and y >= 0 in the observer's frame: pixel (0, 0))
    and samples of frac = 0 are counted and add nothing: a pixel with only such samples stays at
    exactly 0.0 and one that also receives positive samples holds exactly their sum."""
    geo = GEO[256]
    rng = np.random.default_rng(8)
    behind = scene([0]*300, 0, yo=rng.choice([0.0, 0.5, 2.0], 300), seed=2)
    front = scene([0]*200, 0, yo=-1.0, seed=3)
    zeros_only = scene([5]*70 + [31]*3, [2]*70 + [7]*3, k=0, seed=4)
    mixed = scene([9]*400, 4, seed=5)
    mixed['k'][::2] = 0
    others = scattered(32, 8, 1000, 6)
    others['ix'][np.isin(others['ix'], [0, 5, 9, 31])] = 17
    s = join(behind, front, zeros_only, mixed, others)
    s = take(s, np.random.default_rng(9).permutation(len(s['ix'])))
    counts, weights, _, _ = expected(dict(dims=geo[:2], route=route), s)
    assert counts[0, 0] == 500 and counts[5, 2] == 70 and counts[31, 7] == 3 and counts[9, 4] == 400
    assert weights[5, 2] == 0 and weights[31, 7] == 0
    assert weights[0, 0] == front['k'].sum()/1024.0 and weights[9, 4] == mixed['k'].sum()/1024.0
    image, _ = run(tiles, route, geo, s)
    assert image[5, 2] == 0.0 and image[31, 7] == 0.0


# ---- the hand-over ------------------------------------------------------------------------------
def handover_places(case, tile_used):
    """Places of a tile (lane = place % 64 in k_image_tiles' hand-over loop) that receive samples."""
    place = np.arange(tile_used)
    lane = place % 64
    if case == 'lower':
        return place[lane < 32]
    if case == 'upper':
        return place[lane >= 32]
    if case == 'partners':                     # lanes l and l + 32 of the first and the last wave
        return np.concatenate([place[:64], place[-64:]])
    if case == 'one_pixel':
        return place[[tile_used//3]]
    if case == 'alternating':
        return place[::2]
    assert case == 'gap' and tile_used >= 192  # a wave with nothing to hand over between two with some
    return np.concatenate([place[3:64:5], place[128:192:3]])


@pytest.mark.parametrize('case', ['lower', 'upper', 'partners', 'one_pixel', 'alternating', 'gap'])
@pytest.mark.parametrize('geo', [(16, 16, 0), (64, 16, 512)])
@pytest.mark.parametrize('route', COLUMN_ROUTES)
def test_hand_over_shapes(tiles, route, geo, case):
    """The touched pixels of a tile arranged so that only the lower half-waves, only the upper,
    both partners, a single pixel, alternating pixels and a gap of 64 untouched pixels occur in
    the hand-over; most pixels hold one sample, two hold thousands (a lower and an upper lane: the
    whole count crosses the half-wave swap)."""
    nx, nz, _ = geo
    g = TP.geometry(*geo)
    assert (g['nb'], g['tile_used']) == {16: (1, 256), 64: (2, 512)}[nx]
    places = handover_places(case, g['tile_used'])
    lanes = places % 64
    assert {'lower': lanes.max() < 32, 'upper': lanes.min() >= 32,
            'partners': set(lanes) == set(range(64)), 'one_pixel': len(places) == 1,
            'alternating': set(lanes) == set(range(0, 64, 2)),
            'gap': not np.any((places >= 64) & (places < 128))}[case]
    b = g['nb'] - 1                                            # the touched tile
    pix = np.array([TP.pixel(int(loc), b, g) for loc in places])
    big = [pix[0]] if len(pix) == 1 else [pix[0], pix[32]] if case == 'partners' else [pix[0], pix[-1]]
    many = [2900, 2500][:len(big)]
    pix = np.concatenate([pix] + [[q]*(m - 1) for q, m in zip(big, many)])
    s = scene(pix//nz, pix % nz, seed=len(case))
    s = take(s, np.random.default_rng(3).permutation(len(pix)))
    assert len(pix) <= 3*PER_TRIP[ROUTES[route]['bytes']] + 5
    _, _, n = structure(route, geo, s)
    assert n[..., :b].sum() == 0 and n.sum() == len(pix)
    _, counts = run(tiles, route, geo, s)
    assert np.count_nonzero(counts) == len(places) and counts.max() == max(many)


# ---- the scratch is reused ----------------------------------------------------------------------
def reuse_calls(route):
    per_trip = PER_TRIP[ROUTES[route]['bytes']]
    return {'large': ((128, 8, 8), scattered(128, 8, 3*per_trip, 61, outside=0.05)),
            'small': ((5, 3, 0), scattered(5, 3, 65, 62)),
            'other_cap': ((64, 8, 8), scattered(64, 8, per_trip + 1, 63))}


@pytest.mark.parametrize('order', ['large-small-other_cap', 'other_cap-small-large',
                                   'small-large-small'])
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_scratch_reuse_between_calls(tiles, route, order):
    """On one context: 3 per_trip samples into 128 tiles, then 65 samples into one tile of another
    image, then a call in another chunk size -- and the other way round.  Each gives the
    constructed answer wherever it stands: no list or nlist word of an earlier layout is read."""
    calls = reuse_calls(route)
    shapes = {}
    for name, (geo, s) in calls.items():
        g, plan, n = structure(route, geo, s)
        shapes[name] = (g['nb'], g['cap'], n.shape[1], plan['bytes'])
    assert [v[:3] for v in shapes.values()] == [(128, 64, 3), (1, 256, 1), (64, 128, 2)]
    assert shapes['large'][3] > shapes['other_cap'][3] > shapes['small'][3]
    got = {}
    for name in order.split('-'):
        geo, s = calls[name]
        image, counts = run(tiles, route, geo, s)
        if name in got:
            assert np.array_equal(got[name][0], image) and np.array_equal(got[name][1], counts)
        got[name] = (image, counts)


# ---- calls add, clear clears --------------------------------------------------------------------
@pytest.mark.parametrize('route', ALL_ROUTES)
def test_two_calls_add_and_clear_clears(tiles, route):
    geo = GEO[64]
    s = scattered(128, 8, PER_TRIP[ROUTES[route]['bytes']] + 65, 71)
    one, counts1 = run(tiles, route, geo, s)
    two, counts2 = run(tiles, route, geo, s, calls=2)
    assert np.array_equal(counts2, 2*counts1) and counts1.sum() > 1000
    if ROUTES[route]['quantity'] == 'column':
        assert np.array_equal(two, 2*one)
    tiles.image_clear()
    image, counts = tiles.image_download()
    assert not image.any() and not counts.any()


# ---- a general rotation -------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['f32_lines4', 'f32_no_room'])
def test_general_rotation(tiles, route):
    """sublon = 0.4, sublat = 1.1: image_locate_core_xz forms all three observer coordinates from
    all three of the sample (the column cases, under the identity, take its x_is_x branch)."""
    geo = GEO[128]
    rotation = (0.4, 1.1)
    M = _radiance_view(64, 8, ROUTES[route]['lines'], *rotation)['M']
    assert np.count_nonzero(M) == 9
    s = scattered(64, 8, 2*PER_TRIP[4] + 1, 81)
    s['yo'][:] = np.random.default_rng(82).uniform(-3, 3, len(s['ix']))
    _, _, n = structure(route, geo, s)
    assert n.shape[:2] == (1, 3)
    _, counts = run(tiles, route, geo, s, rotation=rotation)
    assert counts.sum() > 4000
