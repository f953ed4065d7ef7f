// Stand-alone driver of the image-shaped LDS block's builder and placement
// (nexoclom_amd/csrc/nxc_image_block.hpp), over descriptor types with the fields of LutDesc and
// ImageK: blocks of 0, 1 and NXC_MAX_LINES tables with 1 x 1 and 512 x 800 edges, placed at two
// bases; offsets, sizes, the bytes themselves, and every placed table inside the block.  Build and
// run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/image_block_check.cpp -o image_block_check && ./image_block_check
// Prints what it counted; exit status 0 when nothing was unexpected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_image_block.hpp"

namespace {

struct Lut {
    int rec, fs, cell, top, last, pad_;
    double xbase, inv_w;
};
struct Packed {
    Lut desc{};
    std::vector<unsigned char> bytes;
};
struct Image {
    int n_lines = -1, nx = -1, nz = -1;
    double x_lo = 0, x_inv_step = 0, z_lo = 0, z_inv_step = 0;
    int64_t xedges_off = -1, zedges_off = -1;
    Lut line[NXC_MAX_LINES]{};
};

int unexpected = 0;

void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    if (ok) return;
    unexpected++;
    std::printf("UNEXPECTED %s (%ld, %ld)\n", what, a, b);
}

// a table of `rows` rows laid out as pack_lut lays one out: 16-byte records, 16-byte {f, slope}
// pairs, then the cell index padded to 32 bytes; every byte is the table's number
Packed table(int number, int rows, int ncell)
{
    Packed p;
    const size_t cell_bytes = ((size_t)(ncell + 2) * 2 + 31) & ~size_t(31);
    p.bytes.assign((size_t)rows * 32 + cell_bytes, (unsigned char)number);
    p.desc = {0, 16 * rows, 32 * rows, ncell + 1, rows - 1, 0, -1.5, 2.0 * number};
    return p;
}

}  // namespace

int main()
{
    int blocks = 0, placements = 0;
    const int dims[2][2] = {{1, 1}, {512, 800}};
    for (int n_lines : {0, 1, NXC_MAX_LINES})
        for (const auto &dim : dims) {
            const int nx = dim[0], nz = dim[1];
            std::vector<double> xe((size_t)nx + 1), ze((size_t)nz + 1);
            for (int k = 0; k <= nx; k++) xe[(size_t)k] = -4.0 + 8.0 * k / nx;
            for (int k = 0; k <= nz; k++) ze[(size_t)k] = 1.0 + 0.25 * k;
            Packed luts[NXC_MAX_LINES];
            size_t tables = 0;
            for (int l = 0; l < n_lines; l++) {
                luts[l] = table(l + 1, 40 + 300 * l, 64 << l);
                tables += luts[l].bytes.size();
            }
            // behind bytes that are already there (the camera's header) and into an empty vector
            for (size_t front : {size_t(0), size_t(96)}) {
                std::vector<unsigned char> out(front, 0xee);
                Image G;
                const ImageBlock<Lut> b = append_image_block(out, G, nx, nz, xe.data(), ze.data(), n_lines, luts);
                blocks++;
                expect(b.n_lines == n_lines && G.n_lines == n_lines && G.nx == nx && G.nz == nz, "dims", nx, nz);
                expect(b.xedges == tables && b.zedges == tables + ((size_t)nx + 1) * 8, "edge offsets", n_lines, nx);
                expect(b.bytes == tables + ((size_t)nx + nz + 2) * 8 && out.size() == front + b.bytes, "size", n_lines, nx);
                expect(G.x_lo == -4.0 && G.x_inv_step == nx / 8.0 && G.z_lo == 1.0 && G.z_inv_step == 4.0, "axis seeds", nx, nz);
                expect(G.xedges_off == -1 && G.zedges_off == -1, "the builder places nothing", n_lines);
                for (size_t k = 0; k < front; k++) expect(out[k] == 0xee, "bytes in front", (long)k);
                expect(!std::memcmp(out.data() + front + b.xedges, xe.data(), ((size_t)nx + 1) * 8) &&
                           !std::memcmp(out.data() + front + b.zedges, ze.data(), ((size_t)nz + 1) * 8), "edge bytes", nx, nz);
                size_t at = 0;
                for (int l = 0; l < n_lines; l++) {
                    const Lut &d = b.line[l];
                    expect(d.rec == (int)at && d.fs == (int)at + luts[l].desc.fs && d.cell == (int)at + luts[l].desc.cell,
                           "table offsets", n_lines, l);
                    expect(d.top == luts[l].desc.top && d.last == luts[l].desc.last && d.xbase == -1.5 &&
                               d.inv_w == luts[l].desc.inv_w, "table scalars", n_lines, l);
                    for (size_t k = 0; k < luts[l].bytes.size(); k++)
                        expect(out[front + at + k] == (unsigned char)(l + 1), "table bytes", l, (long)k);
                    at += luts[l].bytes.size();
                }
                for (size_t base : {size_t(0), front, size_t(4640), size_t(4640 + 41024)}) {
                    Image P = G;
                    place_image_block(b, base, P);
                    placements++;
                    expect(P.xedges_off == (int64_t)(base + b.xedges) && P.zedges_off == (int64_t)(base + b.zedges),
                           "placed edges", (long)base, n_lines);
                    expect(P.zedges_off + ((int64_t)nz + 1) * 8 == (int64_t)(base + b.bytes), "the block ends with the edges", (long)base);
                    for (int l = 0; l < n_lines; l++) {
                        const Lut &d = P.line[l];
                        expect(d.rec == b.line[l].rec + (int)base && d.fs == b.line[l].fs + (int)base &&
                                   d.cell == b.line[l].cell + (int)base, "placed table", (long)base, l);
                        // rec < fs < cell, and the last cell entry (2 bytes each) inside the block, in front of the edges
                        expect(d.rec >= (int)base && d.rec < d.fs && d.fs < d.cell &&
                                   (size_t)d.cell + ((size_t)d.top + 1) * 2 <= base + b.xedges, "placed table inside the block", (long)base, l);
                        expect((size_t)d.fs + ((size_t)d.last + 1) * 16 <= (size_t)d.cell, "rows in front of the cells", (long)base, l);
                    }
                    for (int l = n_lines; l < NXC_MAX_LINES; l++)
                        expect(P.line[l].rec == 0 && P.line[l].cell == 0, "unused lines stay untouched", l);
                }
            }
        }
    std::printf("%d blocks, %d placements, %d unexpected\n", blocks, placements, unexpected);
    return unexpected ? 1 : 0;
}
