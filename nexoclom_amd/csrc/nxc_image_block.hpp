// Host-only: the image-shaped part of an LDS block, [g-value tables | first edges | second edges],
// as the model image (nxc_set_image: once behind the force table, once right behind the header)
// and the camera (nxc_camera_set) lay it out.  Plain C++ without a device call or a handle, over
// whatever descriptor types the caller has (LutDesc / ImageK of nxc_device.hpp in nxc_api.hip), so
// that a stand-alone program checks it on the CPU (tests/tools/image_block_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/nexoclom_hip.h"

// The descriptor of a packed table that starts at byte `base` of the LDS block.
template <class Lut>
Lut placed_lut(Lut d, size_t base)
{
    d.rec += (int)base; d.fs += (int)base; d.cell += (int)base;
    return d;
}

// Where the pieces of one block sit, in bytes from the block's first byte.
template <class Lut>
struct ImageBlock {
    int n_lines = 0;
    Lut line[NXC_MAX_LINES]{};
    size_t xedges = 0, zedges = 0, bytes = 0;
};

// Appends the block to `out`: the n_lines packed tables (luts[l].desc relative to its own
// luts[l].bytes), then the nx + 1 first and nz + 1 second edges; fills the scalars of G that
// describe it.  The offsets reach G through place_image_block.
template <class Image, class Packed>
auto append_image_block(std::vector<unsigned char> &out, Image &G, int64_t nx, int64_t nz,
                        const double *xedges, const double *zedges, int n_lines, const Packed *luts)
    -> ImageBlock<decltype(luts->desc)>
{
    ImageBlock<decltype(luts->desc)> b;
    const size_t start = out.size();
    b.n_lines = n_lines;
    for (int l = 0; l < n_lines; l++) {
        b.line[l] = placed_lut(luts[l].desc, out.size() - start);
        out.insert(out.end(), luts[l].bytes.begin(), luts[l].bytes.end());
    }
    b.xedges = out.size() - start;
    const unsigned char *xe = reinterpret_cast<const unsigned char *>(xedges);
    out.insert(out.end(), xe, xe + (nx + 1) * sizeof(double));
    b.zedges = out.size() - start;
    const unsigned char *ze = reinterpret_cast<const unsigned char *>(zedges);
    out.insert(out.end(), ze, ze + (nz + 1) * sizeof(double));
    b.bytes = out.size() - start;
    G.nx = (int)nx;
    G.nz = (int)nz;
    G.n_lines = n_lines;
    G.x_lo = xedges[0];
    G.x_inv_step = (double)nx / (xedges[nx] - xedges[0]);
    G.z_lo = zedges[0];
    G.z_inv_step = (double)nz / (zedges[nz] - zedges[0]);
    return b;
}

// G's table descriptors and edge offsets for a block whose first byte is byte `base` of the LDS.
template <class Lut, class Image>
void place_image_block(const ImageBlock<Lut> &b, size_t base, Image &G)
{
    for (int l = 0; l < b.n_lines; l++) G.line[l] = placed_lut(b.line[l], base);
    G.xedges_off = (int64_t)(base + b.xedges);
    G.zedges_off = (int64_t)(base + b.zedges);
}
