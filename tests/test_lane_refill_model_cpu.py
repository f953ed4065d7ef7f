"""tests/lane_refill_model.py against schedules worked out by hand from the rules (64 lanes,
chunks of 32, a packet holds its lane for steps + 1 trips, the loop ends at the first trip start
without a packet in any lane).  The GPU tests judge k_const_fused's wave_trips by this model, so
nothing here comes from the kernel."""
import numpy as np
import pytest

from tests import lane_refill_model as M


def run(steps, order=None):
    steps = np.asarray(steps)
    order = np.arange(len(steps)) if order is None else np.asarray(order)
    return M.schedule(order, steps, len(steps))


def test_three_packets_of_two_zero_and_one_step_make_three_trips():
    # trip 1: the chunk holds 3 packets, lanes 0, 1, 2 take them; the next claim (position 32)
    #         lies beyond n = 3: drained.  Packet 1 (0 steps) ends in this trip.
    # trip 2: packets 0 and 2 take their first step; packet 2 (1 step) ends.
    # trip 3: packet 0 takes its second step and ends.
    # trip 4 would start with no packet in any lane: 3 trips.
    trips, lane, served = run([2, 0, 1])
    assert trips == 3
    assert list(lane) == [0, 1, 2] and list(served) == [1, 1, 1]


def test_sixty_five_packets_of_one_step_make_four_trips():
    # trip 1: 64 lanes ask; chunk 0..31 goes to lanes 0..31, chunk 32..63 to lanes 32..63.
    # trip 2: all 64 take their step and end.
    # trip 3: 64 lanes ask; the chunk at 64 is min(32, 65 - 64) = 1 long: lane 0 takes packet
    #         64; 63 lanes still ask, the claim at 96 is beyond 65: drained.
    # trip 4: packet 64 takes its step and ends.  4 trips.
    trips, lane, served = run([1]*65)
    assert trips == 4
    assert list(lane[:64]) == list(range(64)) and lane[64] == 0
    assert list(served[:64]) == [1]*64 and served[64] == 3


def test_a_ballot_that_crosses_a_chunk_boundary():
    # n = 128.  Queue positions 0..39 take 0 steps, 40..63 take 3, 64..127 take 0.
    # trip 1: chunks 0 and 1 fill lanes 0..63; lanes 0..39 end at once, lanes 40..63 hold their
    #         packets through trips 1..4.
    # trip 2: 40 lanes ask (want = 40).  Chunk 64..95 has room for 32: lanes 0..31.  want > room:
    #         chunk 96..127 is loaded in the same refill and lanes 32..39 take 96..103; it keeps
    #         24.  All 40 end in this trip.
    # trip 3: lanes 0..39 ask again; the chunk has 24 left: 104..127 go to lanes 0..23; 16 lanes
    #         still ask, the claim at 128 is not below n: drained.
    # trip 4: only lanes 40..63 work (their third step).  4 trips.
    steps = [0]*40 + [3]*24 + [0]*64
    trips, lane, served = run(steps)
    assert trips == 4
    assert list(lane[64:104]) == list(range(40)) and list(served[64:104]) == [2]*40
    assert list(lane[104:128]) == list(range(24)) and list(served[104:128]) == [3]*24


def test_the_short_last_chunk():
    # n = 70.  Positions 0..63 take 1 step, 64..69 take 2.
    # trips 1, 2: the first 64 packets, as in the 65-packet case.
    # trip 3: 64 lanes ask; the chunk at 64 is 70 - 64 = 6 long: lanes 0..5; the claim at 96 is
    #         beyond n: drained.
    # trips 4, 5: their two steps.  5 trips.
    trips, lane, served = run([1]*64 + [2]*6)
    assert trips == 5
    assert list(lane[64:]) == [0, 1, 2, 3, 4, 5] and list(served[64:]) == [3]*6


def test_two_hundred_packets_dead_at_the_start():
    # every packet holds its lane for one trip: 64 per trip in trips 1, 2, 3 (positions 0..191,
    # six whole chunks), and in trip 4 the chunk at 192 is 8 long: lanes 0..7, then drained.
    trips, lane, served = run([0]*200)
    assert trips == 4
    assert list(served) == [1]*64 + [2]*64 + [3]*64 + [4]*8
    assert list(lane) == list(range(64))*3 + list(range(8))


def test_fewer_packets_than_a_chunk():
    # n = 5: the first chunk is 5 long, lanes 0..4; the 59 other lanes ask, the claim at 32 is
    # beyond n: drained in trip 1.  The longest packet (3 steps) holds lane 0 for trips 1..4.
    trips, lane, served = run([3, 1, 0, 2, 1])
    assert trips == 4
    assert list(lane) == [0, 1, 2, 3, 4] and list(served) == [1]*5


def test_the_queue_order_decides_who_goes_first():
    # 65 packets, packet 0 last in the queue: it is the one that waits for trip 3 (as packet 64
    # does in the 65-packet case) and takes its 5 steps in trips 4..8.
    order = list(range(1, 65)) + [0]
    trips, lane, served = run([5] + [1]*64, order)
    assert trips == 8 and served[0] == 3 and lane[0] == 0
    assert list(lane[1:]) == list(range(64)) and list(served[1:]) == [1]*64


@pytest.mark.parametrize('seed', range(40))
def test_invariants_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 500))
    steps = rng.integers(0, int(rng.integers(1, 70)), n)
    if seed % 4 == 0:
        steps[rng.random(n) < 0.5] = 0
    order = rng.permutation(n)
    trips, lane, served = M.schedule(order, steps, n)
    assert trips >= -(-int(np.sum(steps + 1))//64)          # 64 lanes, one trip of a packet each
    assert trips >= steps.max() + 1                         # a packet's trips follow one another
    # every packet handed out exactly once ...
    assert np.all((lane >= 0) & (lane < 64)) and np.all(served >= 1)
    # ... in queue order: by trip, within a trip by lane
    assert np.array_equal(np.lexsort((lane, served)), order)
    # no lane holds two packets at once, and the last packet's end is the last trip
    for l in range(64):
        mine = order[lane[order] == l]
        ends = served[mine] + steps[mine]                   # last trip of each
        assert np.all(served[mine][1:] > ends[:-1])
    assert (served + steps).max() == trips


def test_queue_orders_as_the_ordering_kernels_bin_them():
    # |v|^2 = 4, 16, 1, 9: bins int(v2 * 4095 / 16) = 1023, 4095, 255, 2303, fastest first
    X0 = np.zeros((4, 8))
    X0[:, 4] = [2., 4., 1., 3.]
    order, bins = M.speed_order(X0)
    assert list(bins) == [1023, 4095, 255, 2303] and list(order) == [1, 3, 0, 2]
    assert list(M.speed_order(X0[:1])[0]) == [0]
    # steps 0, 16, 3, 16 of n_iter 16: bins 0, 4095, 767, 4095; the tie keeps its members together
    order = M.steps_order([0, 16, 3, 16], 16)
    assert sorted(order[:2]) == [1, 3] and list(order[2:]) == [2, 0]


@pytest.mark.parametrize('n', [2, 97, 257, 400])
def test_spread_speeds_gives_every_packet_a_bin_of_its_own(n):
    rng = np.random.default_rng(n)
    X0 = np.zeros((n, 8))
    X0[:, 4:7] = rng.normal(size=(n, 3))*1e-3
    X = M.spread_speeds(X0, 3)
    d0 = X0[:, 4:7]/np.linalg.norm(X0[:, 4:7], axis=1)[:, None]
    d1 = X[:, 4:7]/np.linalg.norm(X[:, 4:7], axis=1)[:, None]
    np.testing.assert_allclose(d1, d0, rtol=1e-14, atol=1e-15)            # directions kept
    _, bins = M.speed_order(X)
    gaps = np.diff(np.sort(bins))
    assert gaps.min() >= 4095//n - 1
    assert bins.max() >= 4094


# ---- the inputs of tests/test_gpu_lane_refill.py: what they must be for those tests to bite ----
def test_gpu_cases_put_every_packet_into_a_speed_bin_of_its_own():
    from tests import lane_refill_cases as K
    for n in (31, 32, 33, 63, 64, 65, 96, 97, 113, 200, 257, 300, 400):
        X0 = K.packets(n, 5)
        assert K.distinct_bins(X0) >= 2
        assert np.all((X0[:, 0] > 0) & (X0[:, 0] <= K.STEP*K.N_ITER))
        assert list(np.nonzero(X0[:, 7] == 0)[0]) == list(range(7, n, 19))


def test_gpu_cases_hand_lanes_a_second_packet():
    """One wave over the checker's step counts: lanes do take second packets, the lifetimes are
    many and unequal, the schedule lies within the bounds the tests of several waves use, and in
    the re-emission case the packets of the first trip bounce before their lanes move on."""
    from tests import lane_refill_cases as K
    for n in (65, 97, 257, 400):
        ref = K.reference('plain', True, n)
        trips, lane, served = K.trips_1x1(ref)
        assert (served > 1).sum() >= n - 64 and len(np.unique(ref['steps'])) > 20
        assert K.trip_bounds(ref, 1)[0] <= trips <= K.trip_bounds(ref, 1)[1]
    ref = K.reference('bounce', True, 257)
    order = M.speed_order(ref['X0'])[0]
    _, lane, served = K.trips_1x1(ref)
    first = order[:64]
    assert np.all(served[first] == 1) and (ref['nbounce'][first] > 0).sum() > 10
    assert ref['nbounce'].max() > 1
