"""How k_los_blocks (nexoclom_amd/csrc/nxc_kernels.hpp) lays the rows of a slab out as a stream of
block slots, said once more in plain Python from the kernel's comments and code, for the tests that
must know -- before they run -- which rows form a block and which slot it takes.

The rules, as the code has them:
  * the rows are cut into REGIONS of 256 rows (NXC_LOS_FORM), and a region starts a packet of its
    own (`bnd[k] = ... || rel == 0 || id differs from the row before`);
  * a block is at most 8 consecutive rows of one packet (NXC_LOS_BLOCK; `emit[k]`: every eighth row
    counted from the packet's start inside the region; `n = min(run, 8)`, the region's end being a
    packet start too);
  * the first block of a packet whose run inside the region is LONGER than 8 rows opens a fresh
    group: its slot number is rounded up to a multiple of 8 (`fresh[k] = rel == start && run > 8`),
    the slots skipped stay empty;
  * the region's last group is completed with empty slots (`full = (tail + 7) & ~7`).
A region's slots go to the stream in one piece; the order of the regions in the stream is not
fixed (an atomic hands out the places), and nothing below depends on it."""
import numpy as np

FORM = 256        # NXC_LOS_FORM: rows per region
BLOCK = 8         # NXC_LOS_BLOCK: rows per block, slots per group
TRIP = 64         # slots a wave of k_los takes at a time


def region_slots(ids, n, first_row=0):
    """The slots of one region of n <= 256 rows, in order: (first row, rows) or None for a slot
    left empty.  ids: the region's part of the index column, or None (one packet)."""
    assert 1 <= n <= FORM
    starts = [0]
    if ids is not None:
        ids = np.asarray(ids)
        assert len(ids) == n
        starts += [int(r) for r in np.nonzero(ids[1:] != ids[:-1])[0] + 1]
    slots = []
    for s, e in zip(starts, starts[1:] + [n]):
        if e - s > BLOCK:
            slots += [None]*(-len(slots) % BLOCK)
        for rel in range(s, e, BLOCK):
            slots.append((first_row + rel, min(BLOCK, e - rel)))
    slots += [None]*(-len(slots) % BLOCK)
    return slots


def slab_layout(n_rows, index=None, first_row=0):
    """One slab (one launch of k_los_blocks) of n_rows rows whose index column is `index` (None:
    no column).  Returns dict(regions: the slots of every region, rows numbered from first_row;
    slots: the length of the stream; T: trips of 64 slots; G, H: groups of 8 and half groups of 4
    slots that hold at least one block)."""
    regions = []
    for lo in range(0, n_rows, FORM):
        n = min(FORM, n_rows - lo)
        regions.append(region_slots(None if index is None else index[lo:lo + n], n, first_row + lo))
    slots = sum(len(r) for r in regions)
    groups = sum(any(b is not None for b in r[g:g + 8]) for r in regions for g in range(0, len(r), 8))
    halves = sum(any(b is not None for b in r[g:g + 4]) for r in regions for g in range(0, len(r), 4))
    return dict(regions=regions, slots=slots, T=(slots + TRIP - 1)//TRIP, G=groups, H=halves)


def layouts(n_rows, index=None, slab_rows=1 << 24):
    """The slabs of a whole pass (los_run: slabs of 2^24 rows, or of NXC_TEST_LOS_SLAB_ROWS, at
    least 256): a list of slab_layout()s with global row numbers.  A slab's index column starts at
    the slab's first row, so a slab starts a region and with it a packet."""
    slab = max(FORM, min(n_rows, slab_rows))
    return [slab_layout(min(slab, n_rows - first),
                        None if index is None else index[first:first + slab], first)
            for first in range(0, n_rows, slab)]


def sphere_tests_without_culling(slabs, n_spectra):
    """What k_los counts in DevCounters.samples when culling is off (every block, half group and
    group that is not empty passes every cone): per spectrum 8 group tests a trip, 2 half tests per
    surviving group, 4 block tests per surviving half."""
    return n_spectra*sum(8*s['T'] + 2*s['G'] + 4*s['H'] for s in slabs)
