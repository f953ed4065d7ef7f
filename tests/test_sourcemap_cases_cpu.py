"""The planted source-map cases (tests/sourcemap_cases.py) without a GPU: every membership of the
brute-force reference lies in a cell its point's tile walks (SourceMapGrid.bucket against seg /
seg_off), no tile names a cell twice, the near-threshold rule drops at most 1 % of a case, the
cases hold what they were planted for, the brute-force reference agrees with the restatement that
is pinned to BallTree, and nxc_source_map_set's host-only check as a stand-alone program, plain
and under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from nexoclom_amd import sourcemap as SM
from tests import sourcemap_cases as C
from tests import sourcemap_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = list(C.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_every_membership_lies_in_a_walked_cell(name):
    c = C.case(name)
    g = c.grid
    assert len(c.pt) > 0
    cell = C.cell_of_packets(g, c.X0['latitude'], c.X0['longitude'])
    assert (cell < g.npoints).all()
    tile = C.tile_of_point(g, c.pt)
    ntiles = -(-g.nlon // g.tile)*g.nlat
    assert len(g.seg_off) == ntiles + 1
    missed = 0
    for t in np.unique(tile):
        walked = np.zeros(g.npoints + 1, dtype=bool)
        walked[C.walked_cells(g, t)] = True
        missed += int((~walked[cell[c.pk[tile == t]]]).sum())
    assert missed == 0


@pytest.mark.parametrize('name', NAMES)
def test_no_tile_names_a_cell_twice(name):
    g = C.case(name).grid
    assert (g.seg[:, 0] >= 0).all() and (g.seg[:, 0] <= g.seg[:, 1]).all()
    assert (g.seg[:, 1] < g.npoints).all()
    for t in range(len(g.seg_off) - 1):
        cells = C.walked_cells(g, t)
        assert len(cells) == len(np.unique(cells)), t


@pytest.mark.parametrize('name', NAMES)
def test_dropped_share_and_what_the_case_holds(name):
    c = C.case(name)
    g, X0 = c.grid, c.X0
    print(f'{name}: {c.dropped} of {c.info["total"]} packets dropped '
          f'({100*c.info["share"]:.2f} %), smallest kept distance {c.info["smallest_rel"]:.2e}')
    assert c.info['share'] <= C.MAX_DROPPED
    assert c.info['smallest_rel'] > C.NEAR
    assert g.tile == C.EXPECTED_TILE[name]
    assert c.info['packets'] <= 20000
    # the rims: the kept packets planted inside a ball are in it, those outside are not
    rim, n = c.rim, len(X0['frac'])
    own = rim[:, 0]*g.nlat + rim[:, 1]
    inside = np.isin(own*n + np.arange(len(rim)), c.pt*n + c.pk)
    # a ball with r > pi/2 planted at r (1 + 1e-9) still lies outside; one with r >= pi is skipped
    assert inside[rim[:, 2] == 0].all() and inside[rim[:, 2] == 2].all()
    assert not inside[rim[:, 2] == 1].any()
    assert (rim[:, 2] == 0).sum() > 0 and (rim[:, 2] == 1).sum() > 0
    # columns: dyadic weights, a fifth or so at 0, the histograms' outer edges, v r_km on vmax
    k = X0['frac']*2.0**20
    assert np.array_equal(k, np.round(k)) and 0.1 < (X0['frac'] == 0).mean() < 0.3
    assert c.info['vmax'] == 4.0 and (X0['v']*C.R_KM == 4.0).sum() == 2
    inc = X0['frac'] > 0
    for col, top in (('altitude', np.pi/2), ('azimuth', 2*np.pi)):
        assert (X0[col][inc] == 0).any() and (X0[col][inc] == top).any()
    assert (X0['v'][inc] == 0).any()
    # poles and the seam
    assert (np.pi/2 - np.abs(X0['latitude']) < 1e-7).sum() >= 16
    lon = X0['longitude']
    assert (lon == 0).any() and (lon == 2*np.pi).any() and (lon < 0).any() and (lon > 2*np.pi).any()


@pytest.mark.parametrize('name', [n for n in NAMES if not n.startswith('1x1')])
def test_seam_copies_are_in_balls_like_their_originals(name):
    c = C.case(name)
    seam, checked = c.seam, 0
    wanted = np.concatenate(list(seam.values()))
    of = np.isin(c.pk, wanted[wanted >= 0])
    balls = {}
    for p, k in zip(c.pt[of].tolist(), c.pk[of].tolist()):
        balls.setdefault(k, set()).add(p)
    for m in range(len(seam['source'])):
        src, zero, two_pi, minus, plus = (int(seam[key][m]) for key in
                                          ('source', 'zero', 'two_pi', 'minus', 'plus'))
        if min(src, minus, plus) >= 0:
            assert balls.get(src, set()) == balls.get(minus, set()) == balls.get(plus, set())
            checked += 1
        if min(zero, two_pi) >= 0:
            assert balls.get(zero, set()) == balls.get(two_pi, set())
    assert checked > 0
    # hist2d keeps longitude 0 and 2 pi (the latter in the last bin) and drops the moved copies
    g, X0 = c.grid, c.X0
    ref = C.arrays(g, X0, c.pt, c.pk, c.info['vmax'], available=True)
    lon = X0['longitude']
    inside = (X0['frac'] > 0) & (lon >= 0) & (lon <= 2*np.pi)
    assert ref['hist2d'].sum() == inside.sum() < (X0['frac'] > 0).sum()
    at_two_pi = (X0['frac'] > 0) & (lon == 2*np.pi)
    if at_two_pi.any():
        last = ref['hist2d'].reshape(g.nlon, g.nlat)[-1].sum()
        assert last >= at_two_pi.sum()


@pytest.mark.parametrize('name', ['24x13 20deg', '37x9 3deg'])
def test_brute_force_agrees_with_the_pinned_restatement(name):
    """sourcemap_restatement.members (float64, with its own latitude band) is pinned to sklearn's
    BallTree by test_sourcemap_cpu; away from the thresholds the longdouble reference without a
    band must find the same pairs, and the per-point arrays built from them must be
    one_output's."""
    c = C.case(name)
    X0, g = c.X0, c.grid
    pt, pk = R.members(X0['latitude'], X0['longitude'], R.params(c.params))
    assert np.array_equal(np.unique(pt*len(X0['frac']) + pk),
                          np.unique(c.pt*len(X0['frac']) + c.pk))
    nvel, nalt, naz = g.nvel, g.nalt, g.naz
    nb = nvel + nalt + naz
    shape = (g.nlon, g.nlat)
    for available in (False, True):
        want = R.one_output(X0, C.R_KM, c.params, 'available' if available else 'source')
        got = C.arrays(g, X0, c.pt, c.pk, c.info['vmax'], available)
        acc = got['acc']
        assert np.array_equal(acc[:, nb].reshape(shape), want['n_total'])
        assert np.array_equal(acc[:, nb + 1].reshape(shape), want['n_included'])
        assert np.array_equal(acc[:, nb + 2].reshape(shape), want['abundance_uncor'])
        assert np.array_equal(acc[:, :nvel].reshape(shape + (nvel,)), want['speed_dist_map'])
        assert np.array_equal(acc[:, nvel:nvel + nalt].reshape(shape + (nalt,)),
                              want['altitude_dist_map'])
        assert np.array_equal(acc[:, nvel + nalt:nb].reshape(shape + (naz,)),
                              want['azimuth_dist_map'])
        for key in ('speed_dist', 'altitude_dist', 'azimuth_dist'):
            assert np.array_equal(got[key], want[key])
        assert np.array_equal(got['speed_gridsum'], want['speed_dist_map'].sum(axis=(0, 1)))
        flat = R.one_output(X0, C.R_KM, dict(c.params, smear_abundance=False),
                            'available' if available else 'source')['abundance_uncor']
        assert np.array_equal(got['hist2d'].reshape(shape), flat)


def test_outputs_add_up_and_the_factor_reaches_the_speed_part_only():
    c = C.case('5x2 50deg')
    g, X0 = c.grid, c.X0
    n = len(X0['frac'])
    first = np.arange(n) < n//2
    whole = C.arrays(g, X0, c.pt, c.pk, 4.0)
    a = C.arrays(g, X0, c.pt, c.pk, 4.0, select=first)
    b = C.arrays(g, X0, c.pt, c.pk, 4.0, select=~first)
    for key in ('acc', 'hist2d') + C.PIECES:
        assert np.array_equal(a[key] + b[key], whole[key]), key
    twice = C.arrays(g, X0, c.pt, c.pk, 4.0, factor=2.0)
    assert np.array_equal(twice['acc'][:, :g.nvel], 2*whole['acc'][:, :g.nvel])
    assert np.array_equal(twice['acc'][:, g.nvel:], whole['acc'][:, g.nvel:])
    assert np.array_equal(twice['speed_gridsum'], whole['speed_gridsum'])
    assert whole['acc'][:, :g.nvel].sum() > 0


def test_cluster_case_fills_its_cells_only():
    params = C.CASES['37x9 3deg'][0]
    grid, X0, pt, pk = C.cluster_case(params, [(2, 4), (30, 7)], [257, 40])
    cell = C.cell_of_packets(grid, X0['latitude'], X0['longitude'])
    assert np.array_equal(np.bincount(cell, minlength=grid.npoints)[[4*37 + 2, 7*37 + 30]],
                          [257, 40]) and len(cell) == 297
    assert 0 < len(np.unique(pk)) < 297                  # some in a ball, some in none
    _, cell_start = C.bucketed(grid, X0)
    totals = {C.candidate_total(grid, cell_start, t) for t in range(len(grid.seg_off) - 1)}
    assert totals == {0, 40, 257}                        # no tile walks both cells


# ---- the C side's refusals, as a host program ---------------------------------------------------
@pytest.mark.parametrize('flags', [['-O1'], ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitizers'])
def test_descriptor_check_as_a_host_program(tmp_path, flags):
    """nxc_source_map_set's refusals and the LDS of k_smap_points and k_smap_prep are host-only
    code (nxc_source_map_check.hpp); tests/tools/source_map_check.cpp feeds it good descriptions,
    one bad one per refusal and both LDS requests below, at and past 64 KiB.  Built plainly and
    with the host sanitizers; both runs must pass."""
    exe = tmp_path / 'source_map_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags,
                           os.path.join(HERE, 'tools', 'source_map_check.cpp'), '-o', str(exe)])
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert '0 unexpected' in done.stdout and 'UNEXPECTED' not in done.stdout
    assert not done.stderr.strip()
    lines = done.stdout.splitlines()
    refused = [line for line in lines if ' refused: ' in line]
    assert len(refused) >= 40 and sum(line.endswith(' accepted') for line in lines) >= 9
    for word in ('null argument', 'bad nxc_source_map_desc grid', 'edges must be finite',
                 'null table', 'do not span the segments', 'are not sorted',
                 'segment outside the grid', "a tile's histograms and segment table need",
                 'edges and whole-planet histograms need 67288 bytes', '64 KiB'):
        assert any(word in line for line in refused), word
    assert any(line.startswith('prep LDS of 64 KiB exactly accepted') for line in lines)
    assert any(line.startswith('prep LDS of 64 KiB + 16 refused') for line in lines)
    assert any(line.startswith('points LDS of 64 KiB exactly accepted') for line in lines)
    assert any(line.startswith('points LDS of 64 KiB + 8 (one more run) refused') for line in lines)
    assert any(line.startswith('4000 speed bins on the default grid, tile 1 refused')
               for line in lines)


def test_the_grid_that_overflowed_is_the_default_one_with_4000_speed_bins():
    """What nxc_source_map_set now refuses: the default grid with nvelbins = 4000 shrinks its tile
    to 1 (32.6 KB for k_smap_points), while k_smap_prep would stage 8 * (ne + nh) = 67 288 bytes."""
    g = SM.SourceMapGrid(dict(nvelbins=4000), C.R_KM)
    assert g.tile == 1
    ne = g.nvel + g.nalt + g.naz + g.nlon + g.nlat + 5
    assert 8*(ne + g.nvel + g.nalt + g.naz) == 67288 > 64*1024
    nseg_max = int(np.diff(g.seg_off).max())
    assert 8*g.tile*(g.nvel + g.nalt + g.naz + 3) + 8*(nseg_max + 1) < 64*1024
