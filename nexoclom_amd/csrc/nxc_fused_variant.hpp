// Host-only side of the persistent kernels' launches: their launch geometry (threads per block,
// queue chunk, per-wave LDS), which instantiation of k_const_fused a call gets and how much LDS a
// persistent workgroup takes.  Plain C++ without a device call or a handle:
// the kernel table of nxc_api.hip is generated from the same constexpr functions that a stand-alone
// program checks on the CPU (tests/tools/fused_variant_check.cpp).
#pragma once
#include <stddef.h>

// The persistent kernels run ONE 12-wave workgroup per CU (3 waves per SIMD, <= 168 VGPRs): the
// waves of a workgroup share a single LDS copy of the tables (~86 KB for Na with a 512^2 image),
// which leaves room for the per-wave packet staging blocks and image queues (4.8 KB per wave)
// inside the CU's 160 KB.
#ifndef NXC_BLOCK_PERSIST_N          // overridable for occupancy experiments (tools/)
#define NXC_BLOCK_PERSIST_N 768
#endif
#ifndef NXC_CHUNK_N
#define NXC_CHUNK_N 32
#endif
constexpr int NXC_BLOCK_PERSIST = NXC_BLOCK_PERSIST_N;
constexpr int NXC_CHUNK = NXC_CHUNK_N;   // packets claimed from the global queue per atomic (<= 64: one per lane)
static_assert(NXC_CHUNK >= 1 && NXC_CHUNK <= 64, "a chunk is loaded by one wave");
constexpr int NXC_IMGQ_SLOTS = 128;      // per-wave image queue (nxc_device.hpp: ImageQueue)
constexpr int NXC_IMGQ_BYTES = NXC_IMGQ_SLOTS * (8 + 8 + 4);
constexpr int NXC_WAVE_STAGE_BYTES = NXC_CHUNK * 9 * 8;   // per-wave LDS staging: 8 columns + packet id
// per-wave LDS of the persistent kernels: the packet staging block, then the image queue
constexpr int NXC_WAVE_LDS_BYTES = NXC_WAVE_STAGE_BYTES + NXC_IMGQ_BYTES;
// the ROWS variant stages two more columns (first row, row count) and has no image queue
constexpr int NXC_WAVE_LDS_BYTES_ROWS = NXC_CHUNK * 11 * 8;

// The template arguments of k_const_fused.  image: 0 none, 1 samples binned as they are (64-bit),
// 2 binned as the float32 values save() stores (nxc_image_desc.downcast_f32); full: gravity +
// radiation pressure + photo-loss, the compile-time specialisation of the force model; rows: 0
// none, 1 wide records, 2 narrow ones.
struct FusedVariant {
    int image = 0;
    bool bounce = false, full = false, nbody = false;
    int rows = 0;
    bool streamed = false;
};

constexpr int NXC_FUSED_CODES = 3 * 2 * 2 * 2 * 3 * 2;     // encode() of a valid variant < this

constexpr int encode(const FusedVariant &v)
{
    return ((((v.image * 2 + v.bounce) * 2 + v.full) * 2 + v.nbody) * 3 + v.rows) * 2 + v.streamed;
}

constexpr FusedVariant decode(int code)
{
    return {code / 48, code / 24 % 2 != 0, code / 12 % 2 != 0, code / 6 % 2 != 0, code / 2 % 3, code % 2 != 0};
}

// The instantiations that exist: the rows pass has no image, the streamed pass is the plain one,
// re-emission comes with the run-time force model and without moons.
constexpr bool valid(const FusedVariant &v)
{
    return v.image >= 0 && v.image <= 2 && v.rows >= 0 && v.rows <= 2 && !(v.image && v.rows) &&
           !(v.streamed && (v.rows || v.bounce || v.nbody)) && !(v.bounce && (v.full || v.nbody));
}

// The variant for a launch, from the force model, what the handle has and what the call wants
// (image: one is binned, downcast_f32: as float32 samples; rows: 0 none, 1 wide, 2 narrow -- a
// rows pass bins nothing): the streamed upload first (the plain force models only: its entry
// point refuses the others), then moons (never with re-emission: refused before the launch), then
// re-emission, then plain.
constexpr FusedVariant pick_variant(bool grav, bool rad, bool loss_photo, bool have_bodies, bool have_bounce,
                                    bool image_on, bool downcast_f32, int rows, bool streamed)
{
    const int image = image_on && !rows ? (downcast_f32 ? 2 : 1) : 0;
    const bool full = grav && rad && loss_photo;
    if (streamed) return {image, false, full, false, rows, true};
    if (have_bodies) return {image, false, full, true, rows, false};
    if (have_bounce) return {image, true, false, false, rows, false};
    return {image, false, full, false, rows, false};
}

// LDS of one persistent workgroup: the tables, then a block per wave (k_var: the default variant's)
constexpr size_t persist_lds(size_t table_bytes, const FusedVariant &v = FusedVariant())
{
    return ((table_bytes + 31) & ~size_t(31)) +
           (size_t)(NXC_BLOCK_PERSIST / 64) * (v.rows ? NXC_WAVE_LDS_BYTES_ROWS : NXC_WAVE_LDS_BYTES);
}
