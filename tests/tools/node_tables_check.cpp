// Stand-alone driver of the host-only part of nxc_packets_sample for per-node tables
// (nexoclom_amd/csrc/nxc_source_check.hpp): descriptor validation and the staging of the tables,
// up to the point of the first device call.  The copies that would go to the device go into a
// host buffer of exactly the staged size, so a sanitizer sees every byte the upload would read
// and every offset it would write.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/node_tables_check.cpp -o node_tables_check && ./node_tables_check
// (or hipcc -x c++ with -Xarch_host -fsanitize=address,undefined).  Prints one line per case;
// exit status 0 when every good descriptor was accepted and every bad one refused.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_source_check.hpp"

namespace {

constexpr int NLON = 5, NLAT = 4, NODES = NLON * NLAT, NV = 7, NA = 3, NZ = 4;

struct Tables {
    std::vector<double> map, speed_cdf, speed_v, alt_cdf, alt, az_cdf, az;
};

std::vector<double> rising_rows(int n)
{
    std::vector<double> t((size_t)NODES * n);
    for (int c = 0; c < NODES; c++)
        for (int k = 0; k < n; k++) t[(size_t)c * n + k] = (double)k / (n - 1);
    return t;
}

std::vector<double> axis(int n, double top)
{
    std::vector<double> a(n);
    for (int k = 0; k < n; k++) a[k] = top * (k + 0.5) / n;
    return a;
}

Tables good_tables()
{
    Tables t;
    t.map.assign(NODES, 1.0);
    t.map[19] = t.map[15] = 0.0;               // two nodes without abundance ...
    t.speed_cdf = rising_rows(NV); t.speed_v = axis(NV, 5.0);
    t.alt_cdf = rising_rows(NA); t.alt = axis(NA, 1.5707963267948966);
    t.az_cdf = rising_rows(NZ); t.az = axis(NZ, 6.283185307179586);
    for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)19 * NV + k] = 0.0;   // ... one a placeholder
    return t;
}

nxc_source_desc describe(const Tables &t)
{
    nxc_source_desc d;
    std::memset(&d, 0, sizeof d);
    d.spatial_type = 2; d.speed_type = 4; d.angular_type = 2;
    d.map_nlon = NLON; d.map_nlat = NLAT; d.map = t.map.data();
    d.n_node_speed = NV; d.node_speed_cdf = t.speed_cdf.data(); d.node_speed_v = t.speed_v.data();
    d.n_node_alt = NA; d.node_alt_cdf = t.alt_cdf.data(); d.node_alt = t.alt.data();
    d.n_node_az = NZ; d.node_az_cdf = t.az_cdf.data(); d.node_az = t.az.data();
    return d;
}

// validation, then -- as nxc_packets_sample does for an accepted descriptor -- the staging
bool accepted(const nxc_source_desc &d, std::string &why)
{
    why = check_node_tables(&d);
    if (!why.empty()) return false;
    const size_t base = 11;                    // other tables in front, as on the device
    const NodeTableLayout L = node_table_layout(&d, base);
    std::vector<double> staged(base + L.total);
    size_t end = base;
    for (const NodeTableCopy &c : L.copy) {
        if (c.count) std::memcpy(staged.data() + c.at, c.from, c.count * sizeof(double));
        if (c.at != end) { why = "staging leaves a gap"; return false; }
        end = c.at + c.count;
    }
    if (end != staged.size()) { why = "staged size does not match the layout"; return false; }
    return true;
}

int failures = 0;

void expect(const char *what, const nxc_source_desc &d, bool want)
{
    std::string why;
    const bool got = accepted(d, why);
    std::printf("%-52s %s%s%s\n", what, got ? "accepted" : "refused", why.empty() ? "" : ": ", why.c_str());
    if (got != want) { failures++; std::printf("    ^ expected to be %s\n", want ? "accepted" : "refused"); }
}

}  // namespace

int main()
{
    const Tables good = good_tables();
    expect("all three tables", describe(good), true);
    { nxc_source_desc d = describe(good); d.angular_type = 1; expect("speeds only", d, true); }
    { nxc_source_desc d = describe(good); d.speed_type = 0; expect("angles only", d, true); }
    { nxc_source_desc d = describe(good); d.speed_type = 0; d.angular_type = 1;
      d.node_speed_cdf = nullptr; expect("no per-node law at all", d, true); }

    { Tables t = good; t.speed_cdf[(size_t)3 * NV + 4] = 0.1; expect("decreasing speed row", describe(t), false); }
    { Tables t = good; for (int k = 0; k < NA; k++) t.alt_cdf[(size_t)6 * NA + k] *= 0.5;
      expect("altitude row that does not reach 1", describe(t), false); }
    { Tables t = good; t.az_cdf[(size_t)2 * NZ] = 0.25; expect("azimuth row that does not start at 0", describe(t), false); }
    { Tables t = good; t.speed_cdf[(size_t)8 * NV + 2] = std::numeric_limits<double>::quiet_NaN();
      expect("NaN in a speed row", describe(t), false); }
    { Tables t = good; for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)7 * NV + k] = 0.0;
      expect("placeholder at a node with abundance", describe(t), false); }
    { Tables t = good; for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)15 * NV + k] = 0.5;
      expect("flat row that is not the placeholder", describe(t), false); }
    { Tables t = good; t.speed_v[NV - 1] = std::numeric_limits<double>::infinity();
      expect("infinite speed axis", describe(t), false); }
    { nxc_source_desc d = describe(good); d.spatial_type = 0; expect("tables with spatial_type 0", d, false); }
    { nxc_source_desc d = describe(good); d.spatial_type = 3; expect("tables with a 1-D map", d, false); }
    { nxc_source_desc d = describe(good); d.generator = 1; expect("PCG64 stream", d, false); }
    { nxc_source_desc d = describe(good); d.speed_type = 3; expect("thermal speeds with per-node directions", d, false); }
    { nxc_source_desc d = describe(good); d.speed_type = 2; expect("tabulated speeds with per-node directions", d, true); }
    { nxc_source_desc d = describe(good); d.n_node_speed = 1; expect("one entry per speed row", d, false); }
    { nxc_source_desc d = describe(good); d.n_node_az = 0; expect("no azimuth entries", d, false); }
    { nxc_source_desc d = describe(good); d.n_node_alt = NXC_NODE_TABLE_MAX + 1; expect("too many altitude entries", d, false); }
    { nxc_source_desc d = describe(good); d.node_speed_cdf = nullptr; expect("speed_type 4 without its table", d, false); }
    { nxc_source_desc d = describe(good); d.node_az = nullptr; expect("azimuth table without its axis", d, false); }
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
