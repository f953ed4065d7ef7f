"""The source-map kernels (k_smap_prep, k_smap_points, k_smap_gridsum) against the brute-force
longdouble reference of tests/sourcemap_cases.py, straight through Context.source_map_set /
source_map_accumulate / source_map_download: the raw accumulator, hist2d and the returned small
histograms are compared before any host arithmetic.

The packets are planted on the rims of the balls of the points at every tile's first and last
longitude, across the 0 / 2 pi seam and over the poles; the weights are dyadic and the factors 1
and 2, so every device sum is exact in fp64 whatever its order and every comparison here is
np.array_equal.  Packets within 1e-10 (relative) of a threshold are not in the cases
(sourcemap_cases.NEAR; the share is asserted in test_sourcemap_cases_cpu)."""
import numpy as np
import pytest

from nexoclom_amd import sourcemap as SM
from nexoclom_amd.hip_api import HipError
from tests import sourcemap_cases as C

pytestmark = pytest.mark.gpu
NXC_ERR_ARG = -2
NARROW = C.CASES['37x9 3deg'][0]          # tiles 16 + 16 + 5, window narrower than a tile


def accumulate(ctx, grid, X0, vmax, available, factor=1.0):
    cols, cell_start = C.bucketed(grid, X0)
    return ctx.source_map_accumulate(cols['latitude'], cols['longitude'], cols['v'],
                                     cols['altitude'], cols['azimuth'], cols['frac'], cell_start,
                                     SM.speed_edges(vmax, grid.nvel), available, factor), cell_start


def same_pieces(got, want):
    for key in C.PIECES:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key


def same_map(ctx, want_acc, want_hist2d):
    acc, hist2d = ctx.source_map_download()
    assert acc.shape == want_acc.shape and hist2d.shape == want_hist2d.shape
    bad = np.argwhere(acc != want_acc)
    assert len(bad) == 0, (len(bad), bad[:8].tolist(), acc[acc != want_acc][:8],
                           want_acc[acc != want_acc][:8])
    assert np.array_equal(hist2d, want_hist2d)
    return acc, hist2d


@pytest.mark.parametrize('available', [False, True], ids=['source', 'available'])
@pytest.mark.parametrize('name', list(C.CASES))
def test_planted_case_equals_the_brute_force_reference(ctx, name, available):
    c = C.case(name)
    want = C.arrays(c.grid, c.X0, c.pt, c.pk, c.info['vmax'], available)
    ctx.source_map_set(c.grid)
    pieces, _ = accumulate(ctx, c.grid, c.X0, c.info['vmax'], available)
    same_pieces(pieces, want)
    acc, _ = same_map(ctx, want['acc'], want['hist2d'])
    nb = c.grid.nvel + c.grid.nalt + c.grid.naz
    assert acc[:, nb].sum() == len(c.pt) > 0 and (acc[:, nb + 1] < acc[:, nb]).any()


def outputs_of(c, rng):
    """The case's packets dealt to three Outputs with vmax 5, 5 and 3 (factors 2, 2 and 1), each
    with speeds of its own and one packet on its vmax."""
    n = len(c.X0['frac'])
    deal = rng.integers(0, 3, n)
    X0 = {k: v.copy() for k, v in c.X0.items()}
    outs = []
    for k, (vmax, factor) in enumerate(((5.0, 2.0), (5.0, 2.0), (3.0, 1.0))):
        mask = deal == k
        idx = np.flatnonzero(mask)
        X0['v'][idx] = rng.uniform(0, (vmax - 0.25)/C.R_KM, len(idx))
        X0['v'][idx[0]] = C.on_vmax(vmax)
        X0['frac'][idx[0]] = 0.5
        outs.append((mask, vmax, factor))
    for mask, vmax, _ in outs:
        assert SM.output_vmax({'v': X0['v'][mask]}, C.R_KM) == vmax
    return X0, outs


@pytest.mark.parametrize('available', [False, True], ids=['source', 'available'])
def test_several_outputs_into_one_resident_map(ctx, available):
    """Two Outputs that share the largest vmax (factor 2 each) and a smaller one (factor 1), each
    with its own speed edges: the speed part of the map carries the factor, nothing else does.
    Then a call without packets, and one whose every frac is 0."""
    c = C.case('24x13 20deg')
    g = c.grid
    X0, outs = outputs_of(c, np.random.default_rng(5))
    ctx.source_map_set(g)
    acc, hist2d = np.zeros((g.npoints, g.nvel + g.nalt + g.naz + 3)), np.zeros(g.npoints)
    for mask, vmax, factor in outs:
        want = C.arrays(g, X0, c.pt, c.pk, vmax, available, factor, select=mask)
        plain = C.arrays(g, X0, c.pt, c.pk, vmax, available, 1.0, select=mask)
        assert np.array_equal(want['acc'][:, :g.nvel], factor*plain['acc'][:, :g.nvel])
        assert np.array_equal(want['acc'][:, g.nvel:], plain['acc'][:, g.nvel:])
        pieces, _ = accumulate(ctx, g, {k: v[mask] for k, v in X0.items()}, vmax, available,
                               factor)
        same_pieces(pieces, plain)                   # the returned histograms are unscaled
        acc += want['acc']
        hist2d += want['hist2d']
        same_map(ctx, acc, hist2d)
    assert acc[:, :g.nvel].sum() > 0
    # no packet at all
    empty = {k: np.zeros(0) for k in X0}
    pieces, _ = accumulate(ctx, g, empty, 1.0, available, 2.0)
    assert all(not pieces[key].any() for key in C.PIECES)
    same_map(ctx, acc, hist2d)
    # every frac 0: the packets count in n_total (and weigh 1 each when 'available'), no more
    mask = outs[2][0]
    none = dict(X0, frac=np.zeros_like(X0['frac']))
    want = C.arrays(g, none, c.pt, c.pk, 3.0, available, 1.0, select=mask)
    nb = g.nvel + g.nalt + g.naz
    grows = [nb, nb + 2] if available else [nb]
    assert want['acc'][:, nb].sum() > 0 and not np.delete(want['acc'], grows, axis=1).any()
    assert not want['hist2d'].any()
    pieces, _ = accumulate(ctx, g, {k: v[mask] for k, v in none.items()}, 3.0, available, 1.0)
    assert all(not pieces[key].any() for key in C.PIECES)
    same_map(ctx, acc + want['acc'], hist2d)


@pytest.mark.parametrize('count', [0, 1, 255, 256, 257])
def test_candidate_total_of_one_tile(ctx, count):
    """``count`` packets in cell (2, 4), 40 in cell (30, 7), which no tile walks together with
    the first: the tile of points 0..15 of row 4 walks exactly ``count`` candidates -- none, one,
    one short of a workgroup, a workgroup, one more -- and most tiles walk none."""
    grid, X0, pt, pk = C.cluster_case(NARROW, [(2, 4), (30, 7)], [count, 40], seed=count)
    for available in (False, True):
        ctx.source_map_set(grid)
        pieces, cell_start = accumulate(ctx, grid, X0, 4.0, available)
        totals = [C.candidate_total(grid, cell_start, t) for t in range(len(grid.seg_off) - 1)]
        assert totals[4*3 + 0] == count and set(totals) == {0, count, 40}
        want = C.arrays(grid, X0, pt, pk, 4.0, available)
        same_pieces(pieces, want)
        same_map(ctx, want['acc'], want['hist2d'])


def test_all_packets_in_one_cell(ctx):
    grid, X0, pt, pk = C.cluster_case(NARROW, [(36, 0)], [300])        # last longitude, first row
    assert len(pt) > 0
    for available in (False, True):
        ctx.source_map_set(grid)
        pieces, cell_start = accumulate(ctx, grid, X0, 4.0, available)
        assert np.count_nonzero(np.diff(cell_start)) == 1
        want = C.arrays(grid, X0, pt, pk, 4.0, available)
        same_pieces(pieces, want)
        same_map(ctx, want['acc'], want['hist2d'])


def test_a_second_set_leaves_nothing_of_the_first_map(ctx):
    a, b = C.case('24x13 20deg'), C.case('5x2 50deg')
    ctx.source_map_set(a.grid)
    accumulate(ctx, a.grid, a.X0, 4.0, False, 2.0)
    ctx.source_map_set(b.grid)
    acc, hist2d = ctx.source_map_download()
    assert acc.shape == (10, 7 + 5 + 6 + 3) and not acc.any() and not hist2d.any()
    pieces, _ = accumulate(ctx, b.grid, b.X0, 4.0, True)
    want = C.arrays(b.grid, b.X0, b.pt, b.pk, 4.0, True)
    same_pieces(pieces, want)
    same_map(ctx, want['acc'], want['hist2d'])
    # and back: the larger map starts from zero again, with its own tiles and segments
    ctx.source_map_set(a.grid)
    pieces, _ = accumulate(ctx, a.grid, a.X0, 4.0, False)
    want = C.arrays(a.grid, a.X0, a.pt, a.pk, 4.0, False)
    same_pieces(pieces, want)
    same_map(ctx, want['acc'], want['hist2d'])


def test_a_grid_k_smap_prep_cannot_stage_is_refused_at_set(ctx):
    """The default grid with nvelbins = 4000: the tile shrinks to 1, which k_smap_points can hold,
    but k_smap_prep would stage 67 288 bytes of edges and histograms.  source_map_set refuses it
    (nothing is launched); the resident map of before stays, and the handle builds a small map
    afterwards."""
    c = C.case('1x1 30deg')
    want = C.arrays(c.grid, c.X0, c.pt, c.pk, 4.0, False)
    ctx.source_map_set(c.grid)
    accumulate(ctx, c.grid, c.X0, 4.0, False)
    big = SM.SourceMapGrid(dict(nvelbins=4000), C.R_KM)
    assert big.tile == 1
    with pytest.raises(HipError, match='need 67288 bytes, more than the 64 KiB of LDS') as err:
        ctx.source_map_set(big)
    assert err.value.code == NXC_ERR_ARG
    same_map(ctx, want['acc'], want['hist2d'])
    d = C.case('5x2 50deg')
    ctx.source_map_set(d.grid)
    pieces, _ = accumulate(ctx, d.grid, d.X0, 4.0, True)
    want = C.arrays(d.grid, d.X0, d.pt, d.pk, 4.0, True)
    same_pieces(pieces, want)
    same_map(ctx, want['acc'], want['hist2d'])
