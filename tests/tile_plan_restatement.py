"""The plan of the tiled stored-sample image (nexoclom_amd/csrc/nxc_tile_plan.hpp) said once more in
Python, for the GPU tests that must know -- before they run -- which producer, tile, chunk and slab a
sample goes through.  tests/test_tile_plan_cpu.py compares it with the C++ (the table that
tests/tools/tile_plan_check.cpp prints), so the two cannot drift apart."""
import numpy as np

# nxc_tile_plan.hpp
STAGE = 8192              # NXC_TILE_STAGE: staged entries per pass-1 workgroup
TILE_MAX = 128            # NXC_TILE_MAX
TILE_PIXELS = 8192        # NXC_TILE_PIXELS
BIN_BLOCK = 1024          # NXC_TILE_BIN_BLOCK
LDS = 160*1024            # NXC_TILE_LDS
SLAB_DEFAULT = 1 << 28    # nxc_image_mode: slab_samples = 0
SLOTS = 256               # a chip's pass-1 workgroups at least (one per CU); see slabs()


def per_trip(sample_bytes):
    """nxc_tile_per_trip: 1024 threads x 4 float32 samples, or x 2 of 64 bits."""
    return BIN_BLOCK*(4 if sample_bytes == 4 else 2)


def room(img_bytes):
    """nxc_tile_room: float32 values leave the weight to pass 2 (DEFER)."""
    return ((img_bytes + 15) & ~15) + TILE_PIXELS*12 <= LDS


def geometry(nx, nz, tile_pixels=0, img_bytes=0):
    """tile_plan(nx, nz, ...): dict(lg, nb, tile_used, cap, lds_bin), or None when refused."""
    tile_pixels = tile_pixels or TILE_PIXELS
    if nx < 1 or nz < 1 or nz > tile_pixels:
        return None
    rows = tile_pixels//nz
    lg = 0
    while (nx + (1 << lg) - 1) >> lg > rows:
        lg += 1
    if 1 << lg > TILE_MAX:
        return None
    nb = 1 << lg
    cap = min(256, STAGE >> lg)
    lds_bin = ((img_bytes + 15) & ~15) + nb*cap*10 + (2*nb + 3)*4
    if lds_bin > LDS:
        return None
    return dict(nx=nx, nz=nz, lg=lg, nb=nb, tile_used=((nx + nb - 1) >> lg)*nz, cap=cap,
                lds_bin=lds_bin)


def slabs(geom, p, slab_samples=0, slots=SLOTS, sample_bytes=8):
    """tile_slabs(...): dict(slab, prod, span, mc, o_sl, o_list, o_n, bytes).  Any `slots` of at
    least ceil(slab / per_trip) gives the same plan: span is then one trip."""
    nb, cap, pt = geom['nb'], geom['cap'], per_trip(sample_bytes)
    slab_max = min(p, slab_samples or SLAB_DEFAULT)
    while True:
        n_slabs = (p + slab_max - 1)//slab_max
        slab = (p + n_slabs - 1)//n_slabs
        prod = max(1, min(slots, (slab + pt - 1)//pt))
        span = ((slab + prod - 1)//prod + pt - 1)//pt*pt
        if span <= (1 << 15)*cap:
            break
        slab_max = (1 << 15)*cap*prod
    mc = span//cap + nb
    entries = prod*mc*cap
    o_sl = entries*8
    o_list = o_sl + entries*2
    o_n = (o_list + prod*nb*mc*2 + 255) & ~255
    return dict(slab=slab, prod=prod, span=span, mc=mc, o_sl=o_sl, o_list=o_list, o_n=o_n,
                bytes=o_n + prod*nb*4, per_trip=pt)


def tile_of(ix, geom):
    return ix & (geom['nb'] - 1)


def place(ix, iz, geom):
    return (ix >> geom['lg'])*geom['nz'] + iz


def pixel(loc, b, geom):
    lrow = loc//geom['nz']
    return ((lrow << geom['lg']) + b)*geom['nz'] + loc - lrow*geom['nz']


def lists(geom, plan, ix):
    """What pass 1 files for samples whose image rows are `ix` in sample order (-1: the sample is
    not filed -- outside the frame, or turned away before the staging blocks).  Returns an int
    array [slab, producer, tile] of entry counts; chunks() and last_fill() read a list's shape
    from a count."""
    ix = np.asarray(ix)
    p = len(ix)
    n_slabs = (p + plan['slab'] - 1)//plan['slab']
    out = np.zeros((n_slabs, plan['prod'], geom['nb']), dtype=np.int64)
    for s in range(n_slabs):
        first = s*plan['slab']
        n = min(plan['slab'], p - first)
        for k in range((n + plan['span'] - 1)//plan['span']):
            rows = ix[first + k*plan['span']:first + min(n, (k + 1)*plan['span'])]
            rows = rows[rows >= 0]
            out[s, k] = np.bincount(rows & (geom['nb'] - 1), minlength=geom['nb'])
    return out


def chunks(m, cap):
    """Chunks of a (producer, tile) list with m entries: the high half of its nlist word."""
    return (np.asarray(m) + cap - 1)//cap


def last_fill(m, cap):
    """Entries of a list's last chunk (cap when it is full; 0 for an empty list)."""
    m = np.asarray(m)
    return np.where(m > 0, m - (chunks(m, cap) - 1)*cap, 0)


def lut_bytes(n, cells_per_node=4):
    """Bytes of a packed g-value table of n points (pack_lut, nxc_api.hip)."""
    ncell = 64
    while ncell < cells_per_node*n and ncell < 16384:
        ncell <<= 1
    return (n + 2)*32 + (((ncell + 2)*2 + 31) & ~31)


def image_part_bytes(g_tables, nx, nz):
    """Bytes of [g-value tables | x edges | z edges] (append_image_block); the image tables that
    the stored-sample kernels stage are these behind the LDS header."""
    return sum(lut_bytes(len(v)) for v, _ in g_tables) + (nx + 1 + nz + 1)*8
