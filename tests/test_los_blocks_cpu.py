"""The restated block formation of the line-of-sight pass (tests/los_blocks_restatement.py), without
a GPU: the properties k_los relies on, on the constructed layouts of the GPU edge tests and on
seeded random index columns.  (The GPU tests tie the restatement to the device: with culling off
the sphere-test counter is a function of the slot layout alone.)"""
import numpy as np
import pytest

from tests import los_blocks_restatement as LB
from tests import los_edge_cases as LC


def check_layout(n_rows, index, slab_rows=1 << 24):
    """Every property of the list in one walk; returns the slabs."""
    slabs = LB.layouts(n_rows, index, slab_rows)
    seen = np.zeros(n_rows, dtype=np.int64)
    slab = max(LB.FORM, min(n_rows, slab_rows))
    assert len(slabs) == (n_rows + slab - 1)//slab
    for k, s in enumerate(slabs):
        rows_here = min(slab, n_rows - k*slab)
        assert len(s['regions']) == (rows_here + LB.FORM - 1)//LB.FORM
        for r, slots in enumerate(s['regions']):
            lo = k*slab + r*LB.FORM
            hi = min(lo + LB.FORM, k*slab + rows_here)
            # a whole number of groups, within slot_desc[][NXC_LOS_FORM + 8] of the kernel
            assert len(slots) % 8 == 0 and 8 <= len(slots) <= LB.FORM + 8
            assert any(b is not None for b in slots[-8:])          # no group of padding alone
            for pos, b in enumerate(slots):
                if b is None:
                    continue
                first, n = b
                assert 1 <= n <= LB.BLOCK and lo <= first and first + n <= hi
                seen[first:first + n] += 1
                if index is not None:
                    assert (index[first:first + n] == index[first]).all()
                # the first block of its packet inside this region?
                starts = first == lo or (index is not None and index[first - 1] != index[first])
                if starts:
                    run = 1
                    while first + run < hi and (index is None or index[first + run] == index[first]):
                        run += 1
                    if run > LB.BLOCK:
                        assert pos % 8 == 0, (first, run, pos)
                    assert n == min(run, LB.BLOCK)
                else:
                    # a later block of a packet follows the one before it, and that one is full
                    assert slots[pos - 1] == (first - LB.BLOCK, LB.BLOCK)
        assert s['slots'] == sum(len(r) for r in s['regions'])
        # the host's max_slots: a slot per row at most, and 7 empty ones per region at most
        assert s['slots'] <= rows_here + 8*len(s['regions'])
        assert s['T'] == -(-s['slots']//64)
        blocks = sum(b is not None for r in s['regions'] for b in r)
        assert -(-blocks//8) <= s['G'] <= s['slots']//8 and s['G'] <= s['H'] <= 2*s['G']
        assert -(-blocks//4) <= s['H']
    assert (seen == 1).all()
    return slabs


@pytest.mark.parametrize('name', list(LC.LAYOUTS))
def test_constructed_layouts(name):
    """The layouts of test_gpu_los_edges.py: every row in exactly one block, blocks within 8 rows,
    one packet and one region, long packets on fresh groups, whole groups per region, the stream
    within the host's bound -- as one slab and as slabs of one region each."""
    ids = LC.layout_ids(name)
    P = len(ids)
    assert P == sum(LC.LAYOUTS[name])
    for slab_rows in (1 << 24, 256):
        check_layout(P, ids, slab_rows)
        if len(LC.LAYOUTS[name]) == 1:
            check_layout(P, None, slab_rows)
    if name in LC.SLAB_LAYOUTS:
        rows = LC.SLAB_LAYOUTS[name]
        ids = ids[:rows]
        assert len(ids) == rows and rows % 256 == 1 and rows >= 513
        edges = np.arange(256, rows, 256)
        assert (ids[edges - 1] == ids[edges]).all()        # a packet straddles every slab edge
        slabs = check_layout(rows, ids, 256)
        assert len(slabs) == rows//256 + 1 and slabs[-1]['regions'] == [[(rows - 1, 1)] + [None]*7]


def test_the_layouts_reach_the_edges_they_are_named_for():
    """What each constructed layout is there for, read from the restated stream."""
    one = {p: LB.slab_layout(p, None) for p in LC.ONE_PACKET}
    assert [one[p]['slots'] for p in LC.ONE_PACKET] == [8, 8, 8, 8, 32, 32, 40, 64, 64, 72]
    assert one[9]['regions'] == [[(0, 8), (8, 1)] + [None]*6]
    assert one[257]['regions'][1] == [(256, 1)] + [None]*7
    # a slot per row: the densest stream, 256 slots a region
    s = LB.slab_layout(300, LC.layout_ids('singles'))
    assert [len(r) for r in s['regions']] == [256, 48] and s['G'] == 32 + 6 and s['H'] == 64 + 11
    # packets of 9 rows: two blocks and six empty slots each -- except where a region's edge cuts
    # a packet into pieces of at most 8 rows, which fill up the group before them
    s = LB.slab_layout(1537, LC.layout_ids('nines'))
    assert s['regions'][0][:16] == [(0, 8), (8, 1)] + [None]*6 + [(9, 8), (17, 1)] + [None]*6
    assert len(s['regions'][0]) == 28*8 and s['regions'][0][-8:-5] == [(243, 8), (251, 1), (252, 4)]
    assert s['regions'][1][:9] == [(256, 5)] + [None]*7 + [(261, 8)]
    assert max(len(r) for r in s['regions']) == 29*8
    # packet starts on every one of a lane's four rows, for packets within a block and beyond
    lens = np.array(LC.LAYOUTS['lane-starts'])
    starts = np.cumsum(lens) - lens
    for long in (False, True):
        assert set(starts[(lens > 8) == long] % 4) == {0, 1, 2, 3}
    # the 20-row packets at 247, 248 and 255: 9 rows left in the region open a group (slot 83 ->
    # 88), 8 rows and 1 row do not
    s = LB.slab_layout(787, LC.layout_ids('region-tail'))
    r0, r1, r2, r3 = s['regions']
    assert r0[82:] == [(246, 1)] + [None]*5 + [(247, 8), (255, 1)] + [None]*6
    assert r1[:2] == [(256, 8), (264, 3)] and r1[80:] == [(501, 3), (504, 8)] + [None]*6
    assert r2[:2] == [(512, 8), (520, 4)] and r2[82:] == [(764, 3), (767, 1)] + [None]*4
    assert r3 == [(768, 8), (776, 8), (784, 3)] + [None]*5
    # back to back: an 8-row packet after the blocks of the 1- and 7-row packets stays where it is
    s = LB.slab_layout(1546, LC.layout_ids('b2b'))
    assert s['regions'][0][:10] == [(0, 1), (1, 7), (8, 8)] + [None]*5 + [(16, 8), (24, 1)]


@pytest.mark.parametrize('seed', range(6))
def test_random_index_columns(seed):
    """50 index columns a seed: packets of 1..top rows for several `top`, ids in no order, ragged
    sizes, one slab and several."""
    rng = np.random.default_rng(seed)
    for _ in range(50):
        top = int(rng.choice([1, 2, 3, 9, 17, 40, 300, 700]))
        P = int(rng.integers(1, 1400))
        lens = rng.integers(1, top + 1, P)
        ids = np.repeat(rng.permutation(len(lens)), lens)[:P].astype(np.int64)
        if rng.random() < 0.15:
            ids = rng.integers(0, 5, P)                     # every row may start a packet
        check_layout(P, ids, int(rng.choice([1 << 24, 256, 300, 512, 1000])))


def test_counter_formula_of_a_small_case():
    """sphere_tests_without_culling on a stream worked out by hand: 9 rows of one packet = two
    blocks in one group, one half, one trip: S (8 + 2 + 4) tests."""
    assert LB.sphere_tests_without_culling(LB.layouts(9), 3) == 3*14
    # 257 rows: 32 blocks in four groups, and one more group for the second region: 40 slots
    assert LB.sphere_tests_without_culling(LB.layouts(257), 1) == 8*1 + 2*5 + 4*9
    # as slabs of one region: a trip each
    assert LB.sphere_tests_without_culling(LB.layouts(257, None, 256), 1) == 8*2 + 2*5 + 4*9
