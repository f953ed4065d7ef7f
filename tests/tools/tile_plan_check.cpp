// Stand-alone driver of the tiled image's plan (nexoclom_amd/csrc/nxc_tile_plan.hpp): sweeps image
// sizes, tile sizes, table sizes, sample counts, slab limits, producer slots and both sample widths
// and checks what k_image_bin and k_image_tiles rely on -- chunk and tile sizes, the pixel <->
// (tile, place) maps, slabs and producers that cover the samples once, 16-bit chunk numbers,
// scratch regions that do not overlap, and that an image is refused exactly when it does not fit.
// Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/tile_plan_check.cpp -o tile_plan_check && ./tile_plan_check
// Prints the plans of a fixed list of inputs (tests/test_tile_plan_cpu.py compares them with
// tests/tile_plan_restatement.py), then what it counted; exit status 0 when nothing was unexpected.
#include <cstdio>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_tile_plan.hpp"

namespace {

long unexpected = 0;

void expect(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0)
{
    if (ok) return;
    if (unexpected++ < 40) std::printf("UNEXPECTED %s (%lld, %lld, %lld)\n", what, a, b, c);
}

// Does the image fit, and with how many tiles?  Said once more without the plan's loop: the
// smallest power of two nb <= NXC_TILE_MAX whose tiles (every nb-th image row) hold at most
// tile_pixels pixels, and staging blocks that fit the LDS behind the image tables.
bool fits_plainly(int nx, int nz, int tile_pixels, size_t img_bytes, int *lg_out)
{
    for (int lg = 0; (1 << lg) <= NXC_TILE_MAX; lg++) {
        const long long rows_in_tile = (nx + (1ll << lg) - 1) / (1ll << lg);
        if (rows_in_tile * nz > tile_pixels) continue;
        const long long nb = 1ll << lg, cap = NXC_TILE_STAGE / nb < 256 ? NXC_TILE_STAGE / nb : 256;
        const long long lds = (long long)((img_bytes + 15) / 16 * 16) + nb * cap * 10 + (2 * nb + 3) * 4;
        *lg_out = lg;
        return lds <= 160 * 1024;
    }
    return false;
}

long n_geoms = 0, n_fit = 0, n_pixels = 0;

void check_geometry(int nx, int nz, int tile_pixels, size_t img_bytes, bool every_pixel)
{
    TilePlan tp;
    int lg = -1;
    const bool fits = tile_plan(nx, nz, tile_pixels, img_bytes, &tp);
    const bool plainly = fits_plainly(nx, nz, tile_pixels, img_bytes, &lg);
    n_geoms++;
    expect(fits == plainly, "refused or accepted against the plain statement", nx, nz, tile_pixels);
    if (!fits) return;
    n_fit++;
    const int nb = 1 << tp.nb_log2;
    expect(tp.nb_log2 == lg, "not the fewest tiles", nx, nz, tile_pixels);
    expect(nb <= NXC_TILE_MAX, "too many tiles", nx, nz, tile_pixels);
    expect(tp.cap == 256 || tp.cap == 128 || tp.cap == 64, "a chunk size without a kernel", tp.cap);
    expect(nb * tp.cap == NXC_TILE_STAGE || tp.cap == 256, "nb x cap", nb, tp.cap);
    expect(nb * tp.cap <= NXC_TILE_STAGE, "staging blocks beyond NXC_TILE_STAGE", nb, tp.cap);
    expect(tp.tile_used >= 1 && tp.tile_used <= tile_pixels && tp.tile_used <= NXC_TILE_PIXELS,
           "tile_used", tp.tile_used, tile_pixels);
    expect(tp.tile_used <= 65536, "a place in the tile is 16 bits", tp.tile_used);
    expect(tp.lds_bin <= NXC_TILE_LDS, "pass 1 beyond the LDS", (long long)tp.lds_bin);
    expect(tp.lds_bin == nxc_tile_tables(img_bytes) + (size_t)nb * tp.cap * 10 + (2 * (size_t)nb + 3) * 4,
           "lds_bin", (long long)tp.lds_bin);
    // every pixel has one place in one tile, inside the tile, and comes back from it
    const int step_z = every_pixel || nz < 4 ? 1 : (nz - 1) / 2;
    for (int ix = 0; ix < nx; ix++)
        for (int iz = 0; iz < nz; iz += step_z) {
            const int b = nxc_tile_of(ix, nb), loc = nxc_tile_loc(ix, iz, tp.nb_log2, nz);
            n_pixels++;
            if (b < 0 || b >= nb || loc < 0 || loc >= tp.tile_used ||
                nxc_tile_pixel(loc, b, tp.nb_log2, nz) != ix * nz + iz)
                expect(false, "pixel map", ix, iz, loc);
        }
    if (!every_pixel) return;
    // ... and no two pixels share a place: every (tile, place) below tile_used is a pixel or lies
    // past the image's last row
    long long inside = 0;
    for (int b = 0; b < nb; b++)
        for (int loc = 0; loc < tp.tile_used; loc++) {
            const long long pix = nxc_tile_pixel(loc, b, tp.nb_log2, nz);
            if (pix < (long long)nx * nz) inside++;
        }
    expect(inside == (long long)nx * nz, "places and pixels differ in number", inside, nx, nz);
}

long n_plans = 0, n_slabs_walked = 0, n_forced = 0;

void check_slabs(const TilePlan &tp, int64_t p, int64_t slab_limit, int64_t slots, size_t bytes)
{
    const TileSlabs s = tile_slabs(tp, p, slab_limit, slots, bytes);
    const int nb = 1 << tp.nb_log2;
    const int64_t per_trip = nxc_tile_per_trip(bytes), cap = tp.cap;
    n_plans++;
    expect(per_trip == (bytes == 4 ? 4096 : 2048), "per_trip", per_trip);
    expect(s.slab >= 1 && s.slab <= p && s.slab <= slab_limit, "slab", s.slab, p, slab_limit);
    expect(s.prod >= 1 && s.prod <= slots, "producers beyond the slots", s.prod, slots);
    expect(s.span >= per_trip && s.span % per_trip == 0, "span is whole trips", s.span, per_trip);
    expect(s.span <= (int64_t(1) << 15) * cap, "span beyond 16-bit chunk numbers", s.span, cap);
    if (std::min(p, slab_limit) > (int64_t(1) << 15) * cap * slots) n_forced++;
    // the slabs cover [0, p) once, each with at most prod producers that cover it once
    const int64_t n_slabs = (p + s.slab - 1) / s.slab;
    expect((n_slabs - 1) * s.slab < p && n_slabs * s.slab >= p, "slabs", n_slabs, s.slab, p);
    if (n_slabs <= 4096) {
        int64_t covered = 0;
        for (int64_t first = 0; first < p; first += s.slab) {      // image_run_tiles' own loop
            const int64_t n = std::min<int64_t>(s.slab, p - first);
            const int64_t grid = (n + s.span - 1) / s.span;
            expect(first == covered && n >= 1, "a gap or an overlap between slabs", first, covered);
            expect(grid >= 1 && grid <= s.prod, "grid beyond the producers", grid, s.prod);
            expect(grid * s.span >= n && (grid - 1) * s.span < n, "producers of a slab", grid, s.span, n);
            covered += n;
            n_slabs_walked++;
        }
        expect(covered == p, "samples covered", covered, p);
    } else {
        const int64_t grid = (s.slab + s.span - 1) / s.span;
        expect(grid >= 1 && grid <= s.prod, "grid beyond the producers", grid, s.prod);
    }
    // chunks: a producer writes at most span / cap full ones and one partial per tile
    expect(s.mc >= s.span / cap + nb, "mc below what a producer can write", s.mc, s.span, cap);
    expect(s.mc <= 65535, "chunk numbers beyond 16 bits", s.mc);
    expect(s.span / cap + 1 <= 65535, "a list's length beyond 16 bits", s.span / cap);
    // scratch: payloads | places | lists | lengths, in this order, none into the next
    const size_t entries = (size_t)s.prod * (size_t)s.mc * (size_t)cap;
    const size_t lists = (size_t)s.prod * nb * (size_t)s.mc;
    expect(entries * 8 <= s.o_sl, "payloads run into the places");
    expect(s.o_sl + entries * 2 <= s.o_list, "places run into the lists");
    expect(s.o_list + lists * 2 <= s.o_n, "lists run into their lengths");
    expect(s.o_n + (size_t)s.prod * nb * 4 <= s.bytes, "lengths run past the scratch");
    expect(s.o_n % 256 == 0 && s.o_sl % 8 == 0 && s.o_list % 2 == 0, "alignment", (long long)s.o_n);
    expect(s.bytes <= s.o_n + (size_t)s.prod * nb * 4, "scratch larger than its regions");
}

void print_plan(int nx, int nz, int tile_pixels, size_t img_bytes, int64_t p, int64_t slab_limit,
                int64_t slots, size_t bytes)
{
    TilePlan tp;
    const bool fits = tile_plan(nx, nz, tile_pixels, img_bytes, &tp);
    std::printf("plan %d %d %d %zu %lld %lld %lld %zu :", nx, nz, tile_pixels, img_bytes, (long long)p,
                (long long)slab_limit, (long long)slots, bytes);
    if (!fits) { std::printf(" refused\n"); return; }
    const TileSlabs s = tile_slabs(tp, p, slab_limit, slots, bytes);
    std::printf(" %d %d %d %zu %d %lld %lld %lld %lld %zu %zu %zu %zu\n", tp.nb_log2, tp.tile_used, tp.cap,
                tp.lds_bin, (int)nxc_tile_room(img_bytes), (long long)s.slab, (long long)s.prod,
                (long long)s.span, (long long)s.mc, s.o_sl, s.o_list, s.o_n, s.bytes);
}

}  // namespace

int main()
{
    const int64_t big = int64_t(1) << 28;                    // nxc_image_mode's default slab limit
    // the plans of the GPU tests' geometries and of the suite's images, as a table
    print_plan(32, 8, 8, 0, 4096, big, 256, 4);
    print_plan(64, 8, 8, 0, 8193, big, 256, 4);
    print_plan(128, 8, 8, 0, 12293, 4097, 256, 4);
    print_plan(128, 8, 8, 0, 6149, 2048, 256, 8);
    print_plan(100, 8, 8, 4000, 4097, big, 512, 8);
    print_plan(1, 1, 8192, 0, 65, big, 256, 8);
    print_plan(5, 3, 8192, 0, 5, 1, 256, 4);
    print_plan(37, 1, 1, 0, 2049, big, 256, 8);
    print_plan(32, 8, 8, 70000, 4096, big, 256, 4);
    print_plan(32, 8, 8, 82000, 4096, big, 256, 4);
    print_plan(512, 512, 8192, 46000, 300001, big, 256, 8);
    print_plan(200, 120, 1024, 46000, 300001, 70001, 512, 4);
    print_plan(800, 800, 8192, 46000, 134000000, big, 512, 4);
    print_plan(800, 800, 8192, 46000, 300001, 100003, 256, 8);
    print_plan(1024, 1024, 8192, 0, 2000000, big, 256, 4);
    print_plan(640, 700, 8192, 46000, 300001, big, 256, 8);
    print_plan(1032, 1024, 8192, 0, 10, big, 256, 8);
    print_plan(8, 1100, 1024, 0, 10, big, 256, 8);
    print_plan(1100, 1100, 8192, 0, 10, big, 256, 8);
    print_plan(512, 512, 8192, 0, int64_t(1) << 31, int64_t(1) << 31, 256, 4);
    print_plan(800, 800, 8192, 0, int64_t(1) << 31, int64_t(1) << 31, 7, 8);
    print_plan(640, 700, 8192, 0, (int64_t(1) << 22) * 3 + 1, int64_t(1) << 31, 1, 4);

    // geometry: image sizes around every power of two and the suite's own, tiles of every size
    const std::vector<int> sizes = {1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 37, 63, 64, 65, 96, 100, 120, 127, 128,
                                    129, 200, 255, 256, 257, 511, 512, 513, 640, 700, 799, 800, 801, 1023,
                                    1024, 1025, 1032, 1099, 1100};
    const std::vector<int> tiles = {1, 2, 3, 7, 8, 9, 15, 16, 37, 64, 100, 255, 256, 1000, 1024, 1100, 4096,
                                    6400, 8191, 8192};
    const std::vector<size_t> tables = {0, 1, 16, 4000, 46000, 65536, 65537, 70000, 81651, 81652, 81653,
                                        81668, 81669, 150000, 161271, 161272, 161273, 163840, 400000};
    for (int nx : sizes)
        for (int nz : sizes)
            for (int tile : tiles) {
                const bool named = (nx == nz && (nx == 512 || nx == 800 || nx == 1024 || nx == 1100)) ||
                                   (nx == 1032 && nz == 1024) || (nx == 640 && nz == 700);
                check_geometry(nx, nz, tile, 0, named || (long)nx * nz <= 70000);
                for (size_t t : tables) check_geometry(nx, nz, tile, t, false);
            }

    // samples: every chunk size and tile count, both widths
    const int geoms[][3] = {{1, 1, 8192},  {5, 3, 8192},     {37, 1, 1},       {32, 8, 8},      {64, 8, 8},
                            {128, 8, 8},   {100, 8, 8},      {512, 512, 8192}, {640, 700, 8192},
                            {800, 800, 8192}, {1024, 1024, 8192}, {200, 120, 1024}};
    const std::vector<int64_t> slot_counts = {1, 2, 3, 4, 7, 255, 256, 257, 512, 768, 1024, 2047, 2048};
    for (const auto &g : geoms) {
        TilePlan tp;
        if (!tile_plan(g[0], g[1], g[2], 0, &tp)) { expect(false, "a swept geometry is refused", g[0], g[1]); continue; }
        for (size_t bytes : {size_t(4), size_t(8)}) {
            const int64_t pt = nxc_tile_per_trip(bytes);
            for (int64_t slots : slot_counts) {
                const int64_t edge = (int64_t(1) << 15) * tp.cap * slots;   // 16-bit chunk numbers bind here
                std::vector<int64_t> ps = {1, 2, 5, 63, 64, 65, 1023, 1025, pt - 1, pt, pt + 1, 2 * pt, 2 * pt + 1,
                                           3 * pt + 5, 12293, (1 << 17) - 1, 1 << 17, (1 << 17) + 1, 150000,
                                           300001, 2000000, (1 << 22) + 3, 134000000, big - 1, big, big + 1,
                                           (int64_t(1) << 31) - 1, int64_t(1) << 31};
                for (int64_t d : {-pt, int64_t(-1), int64_t(0), int64_t(1), pt, pt + 1})
                    for (int64_t m : {1, 2, 3})
                        if (edge * m + d >= 1 && edge * m + d <= (int64_t(1) << 31)) ps.push_back(edge * m + d);
                for (int64_t p : ps) {
                    std::vector<int64_t> limits = {1, 2, 5, pt - 1, pt, pt + 1, 70001, 100003, 1 << 22, big,
                                                   int64_t(1) << 31, edge - 1, edge, edge + 1, p, p - 1, p / 2 + 1};
                    for (int64_t limit : limits)
                        if (limit >= 1 && limit <= (int64_t(1) << 31)) check_slabs(tp, p, limit, slots, bytes);
                }
            }
        }
    }
    std::printf("%ld geometries (%ld fit, %ld pixels mapped), %ld sample plans (%ld slabs walked, "
                "%ld cut by 16-bit chunk numbers), %ld unexpected\n",
                n_geoms, n_fit, n_pixels, n_plans, n_slabs_walked, n_forced, unexpected);
    return unexpected ? 1 : 0;
}
