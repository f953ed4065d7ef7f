"""Surface re-emission on the CPU: np_oracle.bounce_packets against the rows the reference's own
bouncepackets() produced (tests/golden/g12_bounce.npz, made by tests/tools/make_bounce_golden.py),
bit for bit, and the sensitivity of those rows to the last bit of every libm result, which sets
the tolerance of the single-impact GPU tests (tests/test_gpu_bounce.py)."""
import numpy as np
import pytest

from oracle import np_oracle as O
from tests import bounce_cases as B


@pytest.fixture(scope='module')
def golden():
    return np.load(B.GOLDEN, allow_pickle=False)


def test_golden_covers_what_it_should(golden):
    g = golden
    assert list(g['edge_names'][:2]) == ['random', 'terminator pi/2']
    for name in B.CASES:
        X, hit, edge = g[f'{name}_X'], g[f'{name}_hit'], g[f'{name}_edge']
        assert 300 < len(X) < 2000 and 0 < (~hit).sum() < 50
        assert set(range(1, len(g['edge_names']))) <= set(edge.tolist())
        ids = g[f'{name}_ids']
        assert np.array_equal(ids, ids[0] + np.arange(len(ids), dtype=np.uint64))
        assert g[f'{name}_nb'].min() == 0 and g[f'{name}_nb'].max() == 40
        assert (g[f'{name}_nb'] == 0).sum() > 300
        rnd = hit & (edge == 0)
        depth = 1 - g[f'{name}_r0'][rnd]
        speed = np.linalg.norm(X[rnd, 4:7], axis=1)*float(g['unit_km'])
        assert depth.min() < 1e-6 and depth.max() > 2e-2 and speed.min() < 0.4 and speed.max() > 3.9
        outward = np.sum(X[rnd, 1:4]*X[rnd, 4:7], axis=1) > 0
        assert 0.2 < outward.mean() < 0.8
    firsts = [int(g[f'{n}_ids'][0]) for n in B.CASES]
    assert firsts == [0, 2**32 - 100, 2**33 + 5, 2**32]      # one case straddles the high word
    assert [tuple(g[f'{n}_scalars'][1:]) for n in B.CASES] == \
        [(0.5, 0., 0.3), (0.2, 1., 0.), (0., 0., 0.), (0., 0., 0.4)]


@pytest.mark.parametrize('name', list(B.CASES))
def test_restatement_equals_the_reference_bouncepackets_bit_for_bit(golden, name):
    g = golden
    cfg = B.golden_config(g, name)
    ids, nb = g[f'{name}_ids'], g[f'{name}_nb']
    # the stored uniforms are the ones the restatement draws for (id, bounce number)
    assert np.array_equal(B.uniforms(ids, nb, int(g['seed'])), g[f'{name}_u'])
    X = g[f'{name}_X'].copy()
    nb_after = nb.astype(np.int64).copy()
    O.bounce_packets(X, g[f'{name}_r0'], g[f'{name}_hit'], cfg, ids, nb_after)
    want = g[f'{name}_out']
    differs = np.nonzero(np.any(X != want, axis=1))[0]
    assert len(differs) == 0, (differs[:10], g[f'{name}_edge'][differs[:10]],
                               np.abs(X[differs[:10]]/want[differs[:10]] - 1))
    assert np.array_equal(nb_after, nb + g[f'{name}_hit'])
    # packets above the surface are untouched
    assert np.array_equal(want[~g[f'{name}_hit']], g[f'{name}_X'][~g[f'{name}_hit']])


def test_libm_sensitivity_is_what_the_gpu_tolerance_was_derived_from(golden):
    """The figures in test_gpu_bounce's docstring: the largest change of the restatement's rows
    when every libm result in it is moved by one ulp up or down (all up, all down, and random
    signs per call and row), relative to the column's scale (1 for positions, the speed for
    velocities, frac for frac)."""
    from tests.test_gpu_bounce import LIBM_SPREAD, libm_spread
    worst = np.zeros(3)
    for name in B.CASES:
        worst = np.maximum(worst, libm_spread(golden, name))
    # the recorded figures bound what is measured here, and are not padded by more than 2x
    assert np.all(worst <= LIBM_SPREAD) and np.all(worst >= 0.5*np.array(LIBM_SPREAD)), worst
