"""The lane-refill schedule of ONE wave of k_const_fused, restated in plain Python (TEST
INFRASTRUCTURE, imported by tests only).

What is restated (nxc_kernels.hpp: the loop of k_const_fused and WaveQueue::refill):

  * the wave claims queue position 0 when it starts; every chunk load claims the next NXC_CHUNK
    positions (one wave alone: 0, 32, 64, ...);
  * at the top of every trip the lanes without a packet are served in lane order from the
    current chunk; when the chunk is used up the claimed one is loaded, min(32, n - b) long from
    its position b; b >= n means the queue is drained, for good;
  * a packet served in trip t spends that trip being binned (record 0) and every later trip
    taking one step, so it holds its lane for steps + 1 trips (a packet that starts dead, or
    n_iter = 0: one trip) and the lane asks again in trip t + steps + 1;
  * the loop ends at the first trip start at which, after the refill, no lane holds a packet.

The model takes its authority from the hand-worked cases of tests/test_lane_refill_model_cpu.py,
not from the kernel it is used to judge.

The queue order of a resident set cannot be downloaded; `speed_order` and `steps_order` compute it
as the ordering kernels define it (speed_bin / steps_bin, counting sort by descending bin).  Within
a bin the device's order is not fixed, so a caller that needs THE order uses inputs whose bins
are distinct (`spread_speeds`)."""
import numpy as np

CHUNK = 32          # NXC_CHUNK
LANES = 64
ORDER_BINS = 4096   # NXC_ORDER_BINS


def schedule(order, steps, n=None):
    """order: packet ids, front of the queue first; steps[i]: steps packet i takes; n: packets in
    the queue (len(order)).  Returns (trips, lane, served): the wave's trips through the loop
    and, per packet id, the lane that took it and the trip (from 1) in which it was handed out
    (-1 / 0 for a packet that was never handed out: there is none when the model is right)."""
    order = np.asarray(order, dtype=np.int64)
    steps = np.asarray(steps, dtype=np.int64)
    n = len(order) if n is None else int(n)
    assert len(order) == n and len(steps) >= n
    lane_of = np.full(len(steps), -1, dtype=np.int64)
    served_in = np.zeros(len(steps), dtype=np.int64)
    left = [0]*LANES                     # trips the lane's packet still holds it; 0 = free
    pending, head = 0, CHUNK             # start(): position 0 claimed, the head now at 32
    base = c_pos = c_cnt = 0
    drained = False
    trips = 0
    while True:
        free = [l for l in range(LANES) if left[l] == 0]
        if free and not drained:
            want, done = len(free), 0
            while done < want:
                if c_pos >= c_cnt:
                    b = pending
                    if b >= n:
                        drained = True
                        break
                    c_cnt, c_pos, base = min(CHUNK, n - b), 0, b
                    pending, head = head, head + CHUNK
                take = min(c_cnt - c_pos, want - done)
                for r in range(take):
                    pid, lane = order[base + c_pos + r], free[done + r]
                    lane_of[pid], served_in[pid] = lane, trips + 1
                    left[lane] = int(steps[pid]) + 1
                c_pos += take
                done += take
        if not any(left):
            break
        trips += 1
        left = [t - 1 if t else 0 for t in left]
    return trips, lane_of, served_in


def speed_bins(vx, vy, vz):
    """speed_bin of every packet before it is turned round: int(|v|^2 * (4095 / max |v|^2))."""
    v2 = (vx*vx + vy*vy) + vz*vz
    return np.minimum((v2*((ORDER_BINS - 1.0)/v2.max())).astype(np.int64), ORDER_BINS - 1)


def speed_order(X0):
    """Queue order after an upload of X0 (n, 8): descending bin of |v|^2, and the bins.  A set of
    fewer than two packets is not sorted."""
    bins = speed_bins(X0[:, 4], X0[:, 5], X0[:, 6])
    if len(X0) < 2:
        return np.arange(len(X0)), bins
    return np.argsort(-bins, kind='stable'), bins


def steps_order(steps, n_iter):
    """Queue order of pass 2 of the rows protocol: descending bin of steps * (4095 / n_iter).
    Packets of one bin took the same number of steps while n_iter <= 4095: their order within
    the bin cannot change the schedule."""
    assert 1 <= n_iter <= ORDER_BINS - 1
    bins = np.minimum((np.asarray(steps)*((ORDER_BINS - 1.0)/n_iter)).astype(np.int64),
                      ORDER_BINS - 1)
    return np.argsort(-bins, kind='stable')


def spread_speeds(X0, seed):
    """X0 with the launch speeds rescaled (directions kept) so that |v|^2 of packet i is
    v2max (j_i + 1) / n over a random permutation j of the packets: every packet in a speed bin
    of its own, at least 4095 / n - 1 bins from its neighbours."""
    X = np.array(X0, dtype=np.float64)
    n = len(X)
    v2 = np.sum(X[:, 4:7]**2, axis=1)
    j = np.random.default_rng(seed).permutation(n)
    X[:, 4:7] *= np.sqrt(v2.max()*(j + 1.0)/n/v2)[:, None]
    return X
