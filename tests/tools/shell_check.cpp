// Stand-alone driver of the host-only check of a shell map's description
// (nexoclom_amd/csrc/nxc_shell_check.hpp): good descriptions, then one bad one per refusal, the
// 2^31 record limit of add_record_pairs one below and at the bound for several grids, and the LDS
// limit of the blob -- nothing is allocated, so the limits are cheap to reach.  Build and run on the
// CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/shell_check.cpp -o shell_check && ./shell_check
// Prints one line per case; exit status 0 when every good description was accepted and every bad
// one refused with the expected text.
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_shell_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void report(const char *name, const std::string &why, const char *text)
{
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    const bool ok = !why.empty() && why.find(text) != std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(),
                ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

// np.linspace(first, last, n + 1): first + k * step, the last edge as given
std::vector<double> linspace(double first, double last, int64_t n)
{
    std::vector<double> e((size_t)n + 1);
    const double step = (last - first) / (double)n;
    for (int64_t k = 0; k <= n; k++) e[(size_t)k] = first + (double)k * step;
    e[(size_t)n] = last;
    return e;
}

// A good description over its own storage; `change` spoils it
struct Case {
    std::vector<double> lon, mu, v[NXC_MAX_LINES], g[NXC_MAX_LINES];
    nxc_shell_desc d{};

    Case(int64_t nlon, int64_t nlat, int64_t nalt, int quantity = 0, int n_lines = 0)
        : lon(linspace(0.0, NXC_SHELL_TWO_PI, nlon)), mu(linspace(-1.0, 1.0, nlat))
    {
        d.vrplanet = 2e-4;
        d.r_lo = 1.0;
        d.r_hi = 3.0;
        d.quantity = quantity;
        d.n_lines = n_lines;
        d.nlon = nlon; d.nlat = nlat; d.nalt = nalt;
        d.lon_edges = lon.data();
        d.mu_edges = mu.data();
        for (int l = 0; l < n_lines && l < NXC_MAX_LINES; l++) {
            v[l] = {-1e-2, 0.0, 1e-2};
            g[l] = {1.0, 2.0, 3.0};
            d.line_n[l] = 3; d.line_v[l] = v[l].data(); d.line_g[l] = g[l].data();
        }
    }
};

void expect(const char *name, Case c, const std::function<void(Case &)> &change, const char *text)
{
    c.d.lon_edges = c.lon.data();         // the copy's own storage
    c.d.mu_edges = c.mu.data();
    for (int l = 0; l < NXC_MAX_LINES; l++)
        if (c.d.line_v[l]) { c.d.line_v[l] = c.v[l].data(); c.d.line_g[l] = c.g[l].data(); }
    if (change) change(c);
    report(name, check_shell_desc(&c.d), text);
}

void expect_grid(const char *name, int64_t nlon, int64_t nlat, int64_t nalt, const char *text)
{
    report(name, check_shell_grid(nlon, nlat, nalt, 1.0, 2.0), text);
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    const Case good(72, 36, 32), lines(72, 36, 32, 1, 2);
    expect("72 x 36 x 32 column", good, nullptr, nullptr);
    expect("72 x 36 x 32 radiance, two lines", lines, nullptr, nullptr);
    expect("1 x 1 x 1", Case(1, 1, 1), nullptr, nullptr);
    expect("3 x 5 x 7", Case(3, 5, 7), nullptr, nullptr);
    expect("8192 x 8192 x 1", Case(8192, 8192, 1), nullptr, nullptr);
    expect("radiance without lines", Case(4, 4, 4, 1, 0), nullptr, nullptr);
    expect("column ignores null tables", Case(4, 4, 4, 0, 2),
           [](Case &c) { c.d.line_v[0] = nullptr; }, nullptr);
    expect("r_lo = 1 exactly, thin range", good, [](Case &c) { c.d.r_hi = 1.0 + 1e-12; }, nullptr);

    report("null description", check_shell_desc(nullptr), "null description");
    expect("nlon = 0", good, [](Case &c) { c.d.nlon = 0; }, "1..8192");
    expect("nlat = 0", good, [](Case &c) { c.d.nlat = 0; }, "1..8192");
    expect("nlon negative", good, [](Case &c) { c.d.nlon = -4; }, "1..8192");
    expect("nlon = 8193", good, [](Case &c) { c.d.nlon = 8193; }, "1..8192");
    expect("nlat = 8193", good, [](Case &c) { c.d.nlat = 8193; }, "1..8192");
    expect("nalt = 0", good, [](Case &c) { c.d.nalt = 0; }, "nalt must be at least 1");
    expect("nalt negative", good, [](Case &c) { c.d.nalt = -1; }, "nalt must be at least 1");
    expect("r_lo NaN", good, [](Case &c) { c.d.r_lo = NaN; }, "finite");
    expect("r_hi inf", good, [](Case &c) { c.d.r_hi = INF; }, "finite");
    expect("r_lo below the surface", good, [](Case &c) { c.d.r_lo = 0.5; }, "at least 1");
    expect("empty range", good, [](Case &c) { c.d.r_hi = c.d.r_lo; }, "below r_hi");
    expect("reversed range", good, [](Case &c) { c.d.r_lo = 4.0; }, "below r_hi");
    expect("vrplanet NaN", good, [](Case &c) { c.d.vrplanet = NaN; }, "vrplanet");
    expect("quantity 2", good, [](Case &c) { c.d.quantity = 2; }, "quantity");
    expect("null lon_edges", good, [](Case &c) { c.d.lon_edges = nullptr; }, "null edges");
    expect("null mu_edges", good, [](Case &c) { c.d.mu_edges = nullptr; }, "null edges");
    expect("lon edge NaN", good, [](Case &c) { c.lon[5] = NaN; }, "lon_edges must be finite");
    expect("mu edge inf", good, [](Case &c) { c.mu[3] = INF; }, "mu_edges must be finite");
    expect("lon edges not increasing", good, [](Case &c) { c.lon[7] = c.lon[6]; }, "lon_edges must increase");
    expect("mu edges not increasing", good, [](Case &c) { c.mu[9] = c.mu[3]; }, "mu_edges must increase");
    expect("lon edges from 0.1", good, [](Case &c) { c.lon[0] = 0.01; }, "lon_edges must span");
    expect("lon edges to 6.28", good, [](Case &c) { c.lon[72] = 6.28; }, "lon_edges must span");
    expect("mu edges to 0.99", good, [](Case &c) { c.mu[36] = 0.99; }, "mu_edges must span");
    expect("n_lines negative", lines, [](Case &c) { c.d.n_lines = -1; }, "n_lines");
    expect("n_lines too large", lines, [](Case &c) { c.d.n_lines = NXC_MAX_LINES + 1; }, "n_lines");
    expect("null line_v", lines, [](Case &c) { c.d.line_v[1] = nullptr; }, "g-value table");
    expect("null line_g", lines, [](Case &c) { c.d.line_g[0] = nullptr; }, "g-value table");
    expect("one-point table", lines, [](Case &c) { c.d.line_n[1] = 1; }, "g-value table");

    // nlon * nlat * (nalt + 2) one below the limit, at it, and far past it
    expect_grid("1 cell, 2^31 - 1 records", 1, 1, LIMIT - 3, nullptr);
    expect_grid("1 cell, 2^31 records", 1, 1, LIMIT - 2, "2^31");
    expect_grid("1 cell, nalt = 2^31", 1, 1, LIMIT, "2^31");
    expect_grid("2^16 cells, 2^31 - 2^16 records", 256, 256, 32765, nullptr);
    expect_grid("2^16 cells, 2^31 records", 256, 256, 32766, "2^31");
    expect_grid("3 cells, 2147483646 records", 3, 1, 715827880, nullptr);
    expect_grid("3 cells, 2147483649 records", 1, 3, 715827881, "2^31");
    expect_grid("8192 x 8192 cells, 30 records each", 8192, 8192, 28, nullptr);
    expect_grid("8192 x 8192 cells, 31 records each", 8192, 8192, 29, nullptr);
    expect_grid("8192 x 8192 cells, 2^31 records", 8192, 8192, 30, "2^31");
    expect_grid("nalt = INT64_MAX", 3, 4, std::numeric_limits<int64_t>::max(), "2^31");

    report("blob of 160 KiB", check_shell_blob(160 * 1024), nullptr);
    report("blob of 160 KiB + 8", check_shell_blob(160 * 1024 + 8), "160 KiB");

    const double inv = shell_inv_dr(32, 1.0, 3.0);
    const bool inv_ok = inv == 16.0 && shell_plane_doubles(72, 36, 32) == size_t(72) * 36 * 34 * 2;
    std::printf("inv_dr %.17g%s\n", inv, inv_ok ? "" : " -- UNEXPECTED");
    if (!inv_ok) unexpected++;

    // copies of the pair per cell: enough for 2^18 records, 1 .. 1024
    const int64_t cells[] = {1, 32, 2592, 262143, 262144, 262145, int64_t(8192) * 8192};
    const int64_t copies[] = {1024, 1024, 102, 2, 1, 1, 1};
    for (int k = 0; k < 7; k++) {
        const bool ok = shell_replicas(cells[k]) == copies[k];
        std::printf("%lld cells: %lld copies%s\n", (long long)cells[k],
                    (long long)shell_replicas(cells[k]), ok ? " ok" : " -- UNEXPECTED");
        if (!ok) unexpected++;
    }

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
