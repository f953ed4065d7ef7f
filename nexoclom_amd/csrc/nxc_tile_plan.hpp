// Host-only: the plan of the tiled stored-sample image (k_image_bin + k_image_tiles in
// nxc_kernels.hpp, image_run_tiles in nxc_api.hip) -- how the image is cut into tiles, how large
// a chunk is, how the samples are cut into slabs and producers, and where the four regions of the
// chunk scratch lie.  Plain C++ without a device call or a handle, so that a stand-alone program
// checks it on the CPU (tests/tools/tile_plan_check.cpp).  The constants and the constexpr
// functions are also what the kernels use.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#ifndef NXC_TILE_STAGE_N          // (overridable: tools/gpu_exp_tile_occupancy.sh)
#define NXC_TILE_STAGE_N 8192
#endif
constexpr int NXC_TILE_STAGE = NXC_TILE_STAGE_N;   // staged entries per workgroup of pass 1 (all tiles)
constexpr int NXC_TILE_MAX = 128;           // tiles per image at most
constexpr int NXC_TILE_PIXELS = 8192;       // pixels per tile at most (96 KB of LDS)
#ifndef NXC_TILE_UNROLL_N
#define NXC_TILE_UNROLL_N 4
#endif
// samples per thread between two workgroup barriers: 4 float32 samples (1.42 / 1.26 / 1.20 / 1.19 ms
// per 1.34e8 rows for 1 / 2 / 3 / 4), 2 of 64 bits (4 would spill)
constexpr int nxc_tile_unroll_bytes(size_t sample_bytes) { return sample_bytes == 4 ? NXC_TILE_UNROLL_N : 2; }
template <typename T> constexpr int nxc_tile_unroll() { return nxc_tile_unroll_bytes(sizeof(T)); }
#ifndef NXC_TILE_BIN_BLOCK_N
#define NXC_TILE_BIN_BLOCK_N 1024
#endif
constexpr int NXC_TILE_BIN_BLOCK = NXC_TILE_BIN_BLOCK_N;      // threads of a pass-1 workgroup
// below this the two launches do not pay (measured: 2^16 samples 0.027 ms either way, 2^18 0.055
// against 0.092, 2^23 0.18 against 0.31, 2^26 0.64 against 1.57)
constexpr int64_t NXC_TILE_MIN_SAMPLES = int64_t(1) << 17;
constexpr size_t NXC_TILE_LDS = 160 * 1024;                   // LDS of a CU

// samples a pass-1 workgroup takes between two pairs of barriers
constexpr int64_t nxc_tile_per_trip(size_t sample_bytes)
{
    return (int64_t)NXC_TILE_BIN_BLOCK * nxc_tile_unroll_bytes(sample_bytes);
}

// the image tables in front of a tile or of the staging blocks
constexpr size_t nxc_tile_tables(size_t img_bytes) { return (img_bytes + 15) & ~size_t(15); }

// float32 values leave the weight to pass 2 (DEFER) when the image tables fit a CU's LDS next to
// a tile
constexpr bool nxc_tile_room(size_t img_bytes)
{
    return nxc_tile_tables(img_bytes) + (size_t)NXC_TILE_PIXELS * 12 <= NXC_TILE_LDS;
}

// Geometry of the tiled image: tile b = image rows ix = b (mod nb), nb a power of two; a tile's
// pixels (ix / nb, iz) must fit the LDS tile; the chunk shrinks as the tiles multiply
// (nb x cap = NXC_TILE_STAGE, at most 256).  False when the image has too many pixels for
// NXC_TILE_MAX tiles (above 1024^2): such images stay with k_image.
struct TilePlan {
    int nb_log2 = 0, tile_used = 0, cap = 256;
    size_t lds_bin = 0;
};
inline bool tile_plan(int nx, int nz, int tile_pixels, size_t img_bytes, TilePlan *out)
{
    if (nx < 1 || nz < 1 || nz > tile_pixels) return false;
    const int rows = tile_pixels / nz;                       // image rows per tile
    int lg = 0;
    while (((nx + (1 << lg) - 1) >> lg) > rows) lg++;
    if ((1 << lg) > NXC_TILE_MAX) return false;
    out->nb_log2 = lg;
    out->tile_used = ((nx + (1 << lg) - 1) >> lg) * nz;
    out->cap = std::min(256, NXC_TILE_STAGE >> lg);
    out->lds_bin = nxc_tile_tables(img_bytes) + (size_t)(1 << lg) * out->cap * 10 +
                   (2 * (size_t)(1 << lg) + 3) * 4;
    return out->lds_bin <= NXC_TILE_LDS;
}

// Where a pixel lives: its tile and its place in the tile (what pass 1 calls), and back (what
// pass 2's hand-over writes out in its loop).
constexpr int nxc_tile_of(int ix, int nb) { return ix & (nb - 1); }              // nb = 1 << nb_log2
constexpr int nxc_tile_loc(int ix, int iz, int nb_log2, int nz) { return (ix >> nb_log2) * nz + iz; }
constexpr int nxc_tile_pixel(int loc, int b, int nb_log2, int nz)
{
    const int lrow = loc / nz, iz = loc - lrow * nz;
    return ((lrow << nb_log2) + b) * nz + iz;
}

// The samples of a call: slabs of `slab` samples (the last may be shorter), each cut into at most
// `prod` producers of `span` samples; a producer owns `mc` chunks of the scratch and a list of mc
// chunk numbers per tile.  Scratch, in bytes from its start:
// payloads | pixels-in-tile at o_sl | chunk lists [producer][tile][mc] at o_list | their lengths
// at o_n, `bytes` in all.
struct TileSlabs {
    int64_t slab = 0, prod = 0, span = 0, mc = 0;
    size_t o_sl = 0, o_list = 0, o_n = 0, bytes = 0;
};
// slab_max: the most samples a slab may hold (1 <= slab_max); slots: the pass-1 workgroups the chip
// holds at once.
inline TileSlabs tile_slabs(const TilePlan &tp, int64_t p, int64_t slab_max, int64_t slots,
                            size_t sample_bytes)
{
    const int nb = 1 << tp.nb_log2, cap = tp.cap;
    const int64_t per_trip = nxc_tile_per_trip(sample_bytes);
    TileSlabs s;
    slab_max = std::min<int64_t>(p, slab_max);
    for (;;) {
        // slabs of equal size: a short last one would run on a fraction of the chip
        const int64_t n_slabs = (p + slab_max - 1) / slab_max;
        s.slab = (p + n_slabs - 1) / n_slabs;
        s.prod = std::max<int64_t>(1, std::min<int64_t>(slots, (s.slab + per_trip - 1) / per_trip));
        s.span = ((s.slab + s.prod - 1) / s.prod + per_trip - 1) / per_trip * per_trip;
        if (s.span <= (int64_t(1) << 15) * cap) break;
        slab_max = (int64_t(1) << 15) * cap * s.prod;         // a producer's chunk numbers are 16 bits
    }
    s.mc = s.span / cap + nb;
    const size_t entries = (size_t)s.prod * (size_t)s.mc * cap;
    s.o_sl = entries * 8;
    s.o_list = s.o_sl + entries * 2;
    s.o_n = (s.o_list + (size_t)s.prod * nb * (size_t)s.mc * 2 + 255) & ~size_t(255);
    s.bytes = s.o_n + (size_t)s.prod * nb * 4;
    return s;
}
