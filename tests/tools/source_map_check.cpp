// Stand-alone driver of the host-only check of a source-map grid
// (nexoclom_amd/csrc/nxc_source_map_check.hpp): good descriptions, then one bad one per refusal,
// and the dynamic LDS of k_smap_points and k_smap_prep one step below, at and past the 64 KiB a
// launch may ask for -- nothing is allocated or launched, so the limits are cheap to reach.  Build
// and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/source_map_check.cpp -o source_map_check && ./source_map_check
// Prints one line per case; exit status 0 when every good description was accepted and every bad
// one refused with the expected text.
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_source_map_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
const double PI = 3.141592653589793;
int unexpected = 0;

void report(const char *name, const std::string &why, const char *text)
{
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    const bool ok = !why.empty() && why.find(text) != std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(), ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

void expect_value(const char *name, long long got, long long want)
{
    std::printf("%s: %lld%s\n", name, got, got == want ? " ok" : " -- UNEXPECTED");
    if (got != want) unexpected++;
}

std::vector<double> linspace(double first, double last, int64_t n)
{
    std::vector<double> e((size_t)n + 1);
    for (int64_t k = 0; k <= n; k++) e[(size_t)k] = first + (double)k * ((last - first) / (double)n);
    e[(size_t)n] = last;
    return e;
}

// A good description over its own storage: every tile lists `per_tile` runs, each the whole grid
// (the check asks that runs lie in the grid, not that they are disjoint)
struct Case {
    std::vector<double> alt, az, lon, lat, plon, plat, pcos, thr;
    std::vector<int32_t> seg, seg_off;
    nxc_source_map_desc d{};

    Case(int64_t nlon, int64_t nlat, int64_t nvel, int64_t tile, int64_t per_tile = 1, int64_t nalt = 23,
         int64_t naz = 45)
        : alt(linspace(0, PI / 2, nalt)), az(linspace(0, 2 * PI, naz)), lon(linspace(0, 2 * PI, nlon)),
          lat(linspace(-PI / 2, PI / 2, nlat)), plon((size_t)nlon, 1.0), plat((size_t)nlat, 0.0),
          pcos((size_t)nlat, 1.0), thr((size_t)nlat, 0.01)
    {
        const int64_t ntiles = (nlon + tile - 1) / tile * nlat;
        seg_off.push_back(0);
        for (int64_t t = 0; t < ntiles; t++) {
            for (int64_t s = 0; s < per_tile; s++) {
                seg.push_back(0);
                seg.push_back((int32_t)(nlon * nlat - 1));
            }
            seg_off.push_back((int32_t)(seg.size() / 2));
        }
        d.nlon = nlon; d.nlat = nlat; d.nvel = nvel; d.nalt = nalt; d.naz = naz;
        d.tile = tile; d.r_km = 2439.7;
        point();
    }

    void point()                              // the descriptor at this object's own storage
    {
        d.alt_edges = alt.data(); d.az_edges = az.data(); d.lon_edges = lon.data(); d.lat_edges = lat.data();
        d.point_lon = plon.data(); d.point_lat = plat.data(); d.point_cos = pcos.data(); d.threshold = thr.data();
        d.n_seg = (int64_t)(seg.size() / 2);
        d.seg = seg.empty() ? nullptr : seg.data();
        d.seg_off = seg_off.data();
    }
};

void expect(const char *name, Case c, const std::function<void(Case &)> &change, const char *text,
            int64_t want_nseg_max = -1)
{
    c.point();
    if (change) change(c);
    int64_t nseg_max = -7;
    report(name, check_source_map_desc(&c.d, &nseg_max), text);
    if (want_nseg_max >= 0) expect_value("    longest segment list", nseg_max, want_nseg_max);
}

}  // namespace

int main()
{
    const Case good(180, 90, 100, 16), tiny(1, 1, 1, 1, 1, 1, 1);
    expect("180 x 90, 100 speed bins, tile 16", good, nullptr, nullptr, 1);
    expect("1 x 1 x 1", tiny, nullptr, nullptr, 1);
    expect("24 x 13, ragged tile, three runs per tile", Case(24, 13, 7, 16, 3, 5, 6), nullptr, nullptr, 3);
    expect("5 x 2, tile = nlon", Case(5, 2, 7, 5), nullptr, nullptr, 1);
    expect("no run at all", Case(4, 3, 7, 2, 0), nullptr, nullptr, 0);
    expect("2^24 points pass the grid rule, their edges not the LDS", good, [](Case &c) {
        c.d.nlon = c.d.nlat = 4096;
        c.lon = linspace(0, 2 * PI, 4096); c.lat = linspace(-PI / 2, PI / 2, 4096);
        c.seg_off.assign((size_t)256 * 4096 + 1, 0); c.seg.clear(); c.point(); },
        "edges and whole-planet histograms need 68264 bytes", 0);

    report("null description", check_source_map_desc(nullptr, nullptr), "null argument");
    expect("nlon = 0", good, [](Case &c) { c.d.nlon = 0; }, "bad nxc_source_map_desc grid");
    expect("nlat negative", good, [](Case &c) { c.d.nlat = -3; }, "bad nxc_source_map_desc grid");
    expect("nvel = 0", good, [](Case &c) { c.d.nvel = 0; }, "bad nxc_source_map_desc grid");
    expect("nalt = 0", good, [](Case &c) { c.d.nalt = 0; }, "bad nxc_source_map_desc grid");
    expect("naz = 0", good, [](Case &c) { c.d.naz = 0; }, "bad nxc_source_map_desc grid");
    expect("tile = 0", good, [](Case &c) { c.d.tile = 0; }, "bad nxc_source_map_desc grid");
    expect("tile above nlon", good, [](Case &c) { c.d.tile = 181; }, "bad nxc_source_map_desc grid");
    expect("r_km = 0", good, [](Case &c) { c.d.r_km = 0.0; }, "bad nxc_source_map_desc grid");
    expect("r_km NaN", good, [](Case &c) { c.d.r_km = NaN; }, "bad nxc_source_map_desc grid");
    expect("r_km infinite", good, [](Case &c) { c.d.r_km = INF; }, "bad nxc_source_map_desc grid");
    expect("2^24 + 4096 points", good, [](Case &c) { c.d.nlon = 4097; c.d.nlat = 4096; },
           "bad nxc_source_map_desc grid");
    expect("nlon * nlat past int64", good, [](Case &c) { c.d.nlon = c.d.nlat = int64_t(1) << 40; },
           "bad nxc_source_map_desc grid");
    expect("2^16 + 1 bins", good, [](Case &c) { c.d.nvel = 65536 - 23 - 45 + 1; }, "bad nxc_source_map_desc grid");
    expect("nvel = INT64_MAX", good, [](Case &c) { c.d.nvel = std::numeric_limits<int64_t>::max(); },
           "bad nxc_source_map_desc grid");
    expect("null alt_edges", good, [](Case &c) { c.d.alt_edges = nullptr; }, "edges must be finite and increasing");
    expect("az edge NaN", good, [](Case &c) { c.az[7] = NaN; }, "edges must be finite and increasing");
    expect("lon edge infinite", good, [](Case &c) { c.lon[180] = INF; }, "edges must be finite and increasing");
    expect("lat edges decreasing", good, [](Case &c) { c.lat[9] = c.lat[7]; }, "edges must be finite and increasing");
    expect("alt edges without extent", good, [](Case &c) { c.alt.assign(c.alt.size(), 0.5); },
           "edges must be finite and increasing");
    expect("null point_lon", good, [](Case &c) { c.d.point_lon = nullptr; }, "null table");
    expect("null point_lat", good, [](Case &c) { c.d.point_lat = nullptr; }, "null table");
    expect("null point_cos", good, [](Case &c) { c.d.point_cos = nullptr; }, "null table");
    expect("null threshold", good, [](Case &c) { c.d.threshold = nullptr; }, "null table");
    expect("null seg_off", good, [](Case &c) { c.d.seg_off = nullptr; }, "null table");
    expect("runs without their table", good, [](Case &c) { c.d.seg = nullptr; }, "null table");
    expect("offsets that start at 1", good, [](Case &c) { c.seg_off[0] = 1; }, "do not span the segments");
    expect("offsets that stop short", good, [](Case &c) { c.d.n_seg += 1; }, "do not span the segments");
    expect("n_seg negative", good, [](Case &c) { c.d.n_seg = -1; }, "do not span the segments");
    expect("offsets out of order", good, [](Case &c) { c.seg_off[5] = 9; }, "are not sorted");
    expect("run from a negative cell", good, [](Case &c) { c.seg[6] = -1; }, "segment outside the grid");
    expect("run past the last cell", good, [](Case &c) { c.seg[9] = 180 * 90; }, "segment outside the grid");
    expect("run that ends before it starts", good, [](Case &c) { c.seg[4] = 8; c.seg[5] = 7; },
           "segment outside the grid");

    // k_smap_prep: 8 * (2 (nvel + nalt + naz) + nlon + nlat + 5) bytes
    expect_value("prep LDS, default grid", (long long)smap_prep_lds_bytes(100, 23, 45, 180, 90), 4888);
    expect_value("prep LDS, 4000 speed bins", (long long)smap_prep_lds_bytes(4000, 23, 45, 180, 90), 67288);
    expect("4000 speed bins on the default grid, tile 1", Case(180, 90, 4000, 1), nullptr,
           "edges and whole-planet histograms need 67288 bytes, more than the 64 KiB");
    expect_value("prep LDS, 181 x 90 with 3890 speed bins", (long long)smap_prep_lds_bytes(3890, 23, 45, 181, 90), 65536);
    expect("prep LDS of 64 KiB exactly", Case(181, 90, 3890, 1), nullptr, nullptr, 1);
    expect("prep LDS of 64 KiB + 16", Case(181, 90, 3891, 1), nullptr, "edges and whole-planet histograms need 65552");
    expect("prep LDS of 64 KiB - 8", Case(180, 90, 3890, 1), nullptr, nullptr, 1);
    expect("a long grid: 30000 x 1", Case(30000, 1, 7, 16, 1, 5, 6), nullptr, "edges and whole-planet histograms");

    // k_smap_points: 8 * tile * (nvel + nalt + naz + 3) + 8 * (longest list + 1) bytes
    expect_value("points LDS, default grid", (long long)smap_points_lds_bytes(16, 100, 23, 45, 1), 16 * 171 * 8 + 16);
    expect_value("points LDS, 16 x 511 doubles and 15 runs", (long long)smap_points_lds_bytes(16, 440, 23, 45, 15), 65536);
    expect("points LDS of 64 KiB exactly", Case(32, 3, 440, 16, 15), nullptr, nullptr, 15);
    expect("points LDS of 64 KiB + 8 (one more run)", Case(32, 3, 440, 16, 16), nullptr,
           "a tile's histograms and segment table need 65544 bytes, more than the 64 KiB");
    expect("one long list among short ones", Case(32, 3, 440, 16, 1), [](Case &c) {
        for (int s = 0; s < 15; s++) { c.seg.push_back(3); c.seg.push_back(5); }
        c.seg_off.back() += 15; c.point(); }, "a tile's histograms and segment table need 65544", -1);
    expect("tile 16 with 500 speed bins", Case(180, 90, 500, 16), nullptr, "a tile's histograms and segment table");
    expect("the same bins at tile 8", Case(180, 90, 500, 8), nullptr, nullptr, 1);

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
