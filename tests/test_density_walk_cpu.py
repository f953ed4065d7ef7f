"""The cases of tests/density_walk_cases.py before any GPU sees them: on every case the restated
walk, scipy's KDTree and a brute-force count by the kernel's expression agree; the cases reach
the regimes they are built for (stated as conditions on the grids, not measured from the product);
and each narrowing mutation of the walk is caught by at least one case."""
import numpy as np
import pytest
from scipy.spatial import KDTree

from tests import density_walk_cases as cases
from tests.density_walk_cases import (CASE_NAMES, CELL_SLACK, COARSE_CAPS, COARSE_EDGES, CORNER_DIMS,
                                      FLOAT32_NAMES, MUTATIONS, build_index, candidate_cells,
                                      pair_hits, restated_cells, restated_walk)
from tests.test_gpu_density_moments import WAVE_CASES, wave_case

EVERY_CASE = [(name, np.float64) for name in CASE_NAMES] + [(name, np.float32) for name in FLOAT32_NAMES]
IDS = [f'{name} {np.dtype(dtype).name}' for name, dtype in EVERY_CASE]
_references = {}


def references(case):
    """(KDTree's counts, the brute-force counts) per point, once per family of cases."""
    if case.family not in _references:
        rows = case.rows[case.ordinary]
        kd = KDTree(rows).query_ball_point(case.points, case.dr, return_length=True)
        _references[case.family] = (np.asarray(kd, dtype=np.int64),
                                    cases.brute_counts(case.points, case.dr, case.rows))
    return _references[case.family]


def walk_counts(case, index, mutate=None):
    walk = restated_walk(index, case.rows, mutate)
    return index.scatter(walk.counts, len(case.points)).astype(np.int64), walk


@pytest.mark.parametrize('name, dtype', EVERY_CASE, ids=IDS)
def test_references_agree(name, dtype, monkeypatch):
    case = cases.case(name, dtype)
    index = build_index(case, monkeypatch)
    kd, brute = references(case)
    got, walk = walk_counts(case, index)
    assert np.array_equal(kd, brute)
    assert np.array_equal(got, kd)
    assert kd.sum() >= 1
    # what is planted to hit hits, what is planted to miss misses
    assert pair_hits(case, case.hits).all() and not pair_hits(case, case.misses).any()
    assert len(case.hits) or name.split()[0] in ('coarse', 'nonfinite')
    if dtype is np.float32:
        assert np.array_equal(case.rows, cases.narrowed(case.rows))
    # the vectorised cull is candidate_cells' (the scalar restatement test_density_cpu.py uses)
    some = np.linspace(0, len(case.rows) - 1, 40).astype(int)
    live, lo, hi = restated_cells(index, case.rows[some])
    for k, p in enumerate(case.rows[some]):
        want = candidate_cells(index, p) if np.isfinite(p).all() else []
        assert walk.cells[some[k]] == len(want) and bool(live[k]) == bool(want)


@pytest.mark.parametrize('name', WAVE_CASES)
@pytest.mark.parametrize('coarse', [False, True])
def test_references_agree_on_the_wave_shapes(name, coarse):
    from nexoclom_amd.ModelDensity import DensityIndex
    pts, dr, calls = wave_case(name, np.random.default_rng(WAVE_CASES.index(name)))
    rows = np.concatenate([np.stack(c[:3], axis=1) for c in calls])
    index = cases.grid_index(pts, dr, 2*dr) if coarse else DensityIndex(pts, dr)
    kd = KDTree(rows).query_ball_point(pts, dr, return_length=True)
    assert np.array_equal(cases.brute_counts(pts, dr, rows), kd)
    assert np.array_equal(index.scatter(restated_walk(index, rows).counts, len(pts)), kd)
    assert kd.sum() >= 1


def inside(index, rows):
    t = (rows - index.origin) * (1.0 / index.h)
    return ((t >= 0) & (t < np.array(index.dims))).all(axis=1)


@pytest.mark.parametrize('name', [n for n in CASE_NAMES if n.startswith('coarse')])
def test_coarse_grids_reach_their_regimes(name, monkeypatch):
    case = cases.case(name)
    index = build_index(case, monkeypatch)
    ratio = index.h / case.dr
    walk = restated_walk(index, case.rows)
    within = inside(index, case.rows)
    assert within.sum() > 10_000 and (~within).sum() > 10_000
    widths = walk.widths[within]
    if case.grid.max_cells is not None:
        assert int(np.prod(index.dims)) <= case.grid.max_cells and ratio >= 2
    if ratio >= 2:
        # r_cell <= 1/2 + 1e-6: a row sees at most one neighbour per axis, but for the sliver
        # |f - 1/2| <= 1e-6 that h = 2 dr leaves (2e-6 of the rows per axis)
        if ratio > 2*(1 + 1e-5):
            assert set(np.unique(walk.cells[within])) <= {1, 2, 4, 8}
        else:
            assert (widths == 3).any(axis=1).mean() < 1e-4
        if min(index.dims) >= 2:
            assert set(np.unique(walk.cells[within])) >= {1, 2, 4, 8}
        else:
            assert index.dims == (1, 1, 1) and set(np.unique(walk.cells[within])) == {1}
    elif ratio > CELL_SLACK:
        # 1/2 < r_cell < 1: both neighbours near the middle of a cell, one cell at the grid's ends
        assert set(np.unique(widths)) == {1, 2, 3}
        assert (widths == 3).any(axis=0).all() and (widths == 1).any(axis=0).all()
    else:
        # the default edge: r_cell > 1, all 27 cells away from the grid's ends
        assert walk.cells[within].max() == 27
        assert np.all((widths == 3) | (widths == 2))


def test_the_coarse_sets_and_grids():
    assert COARSE_EDGES == (1 + 2.0**-20, 1.25, 1.5, 1.999, 2.0, 3.7, 16.0)
    assert COARSE_CAPS == (4096, 64, 8, 1)
    points, rows = cases.coarse_sets()
    assert len(points) == 600 and len(rows) == 60_000
    assert cases.DR == 2.0**-4


def test_planted_cases_reach_their_regimes(monkeypatch):
    for ratio in (1.5, 2.0, 3.7):
        for dtype in (np.float64, np.float32):
            case = cases.case(f'corners h/dr={ratio:g}', dtype)
            index = build_index(case, monkeypatch)
            assert index.dims == CORNER_DIMS and len(case.hits) == len(case.misses) == 26
            assert len(set(np.diff(index.cell_start))) >= 4       # populations differ
    for ratio in (2.0, 3.7):
        case = cases.case(f'faces h/dr={ratio:g}')
        assert len(case.hits) == len(case.misses) == 6
    for which in cases.EDGE_NAMES:
        case = cases.case(f'edges {which}')
        index = build_index(case, monkeypatch)
        assert index.dims == case.info['dims']
        ones = sum(n == 1 for n in index.dims)
        want = {'box': 0, 'padded': 0, 'coplanar': 1, 'collinear': 2, 'single': 3, 'duplicates': 3}
        assert ones == want[which.split()[0]]
        if which.startswith('box') or which.split()[0] in ('single', 'duplicates'):
            # rows outside the grid hit on every axis (box: and on either side)
            sides = case.info['outside']
            assert {a for a, _ in sides} == {0, 1, 2}
            assert not which.startswith('box') or len(sides) == 6
        if which.startswith('padded'):
            cs = index.cell_start
            nx, ny, nz = index.dims
            assert cs[nx*ny] == 0 and cs[-1] == cs[len(cs) - 1 - nx*ny]   # first and last slabs empty
        # rows at the band's ends: one on each end is culled, its neighbour is not
        live, _, _ = restated_cells(index, case.rows)
        t = (case.rows - index.origin) * (1.0 / index.h)
        n = np.array(index.dims)
        assert (t == -1.0).any(axis=0).all() and (t == n).any(axis=0).all()
        assert not live[(t < -1.0).any(axis=1) | (t >= n + 1.0).any(axis=1)].any()
        assert ((t < -1.0).sum(axis=0) >= 1).all() and ((t >= n + 1.0).sum(axis=0) >= 1).all()
    for k in (0, 31, 63):
        case = cases.case(f'ragged lane {k}')
        index = build_index(case, monkeypatch)
        walk = restated_walk(index, case.rows)
        assert len(case.rows) == 64 and walk.cells[k] == 27
        candidates = [sum(index.cell_start[c + 1] - index.cell_start[c] for c in
                          candidate_cells(index, p)) for p in case.rows]
        assert candidates[k] >= 3000 and max(candidates[:k] + candidates[k + 1:]) <= 4
        assert 0 in candidates and (walk.cells == 0).any()
    for which, block in (('corners 3x3x3', 3), ('corners 2x2x2', 2)):
        case = cases.case(f'ragged {which}')
        index = build_index(case, monkeypatch)
        _, lo, hi = restated_cells(index, case.rows[:1])
        assert np.array_equal(hi[0] - lo[0] + 1, [block]*3)
        nx, ny, _ = index.dims
        cs = index.cell_start
        filled = [[int(cs[(cz*ny + cy)*nx + hi[0, 0] + 1] - cs[(cz*ny + cy)*nx + lo[0, 0]]) > 0
                   for cy in range(lo[0, 1], hi[0, 1] + 1)] for cz in range(lo[0, 2], hi[0, 2] + 1)]
        ranges = [f for per_cz in filled for f in per_cz]
        assert ranges[0] and not ranges[1] and not ranges[-1] and sum(ranges) >= 2
        assert len(case.rows) == 64 and restated_walk(index, case.rows).cells[1] == block**3
    case = cases.case('ragged one point')
    assert np.array_equal(references(case)[0], [64])
    for name in ('nonfinite h/dr=1+2^-20', 'nonfinite h/dr=2'):
        case = cases.case(name)
        bad = case.rows[~case.ordinary]
        assert len(bad) == 15 and (~np.isfinite(bad) | (np.abs(bad) == 1e300)).any(axis=1).all()
        assert all(np.isnan(bad[:, a]).sum() == 1 and np.isposinf(bad[:, a]).sum() == 1 and
                   np.isneginf(bad[:, a]).sum() == 1 and (np.abs(bad[:, a]) == 1e300).sum() == 2
                   for a in range(3))
        index = build_index(case, monkeypatch)
        assert not restated_walk(index, case.rows).cells[~case.ordinary].any()


def sharp_cases():
    """Every case but the largest coarse grids, whose regimes the smaller ones share."""
    skip = ('coarse h/dr=16', 'coarse cap=8', 'coarse cap=1')
    return [n for n in CASE_NAMES if n not in skip]


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_each_mutation_is_caught(mutation, monkeypatch):
    caught = []
    for name in sharp_cases():
        case = cases.case(name)
        index = build_index(case, monkeypatch)
        got, _ = walk_counts(case, index, mutation)
        if not np.array_equal(got, references(case)[0]):
            caught.append(name)
    print(f'{mutation}: caught by {len(caught)} cases: {", ".join(caught)}')
    assert caught
