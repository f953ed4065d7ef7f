// Stand-alone driver of the host-only side of the descriptors (nexoclom_amd/csrc/nxc_desc_check.hpp):
// everything nxc_packets_sample does with a source descriptor up to its first device call -- the
// refusals, the place of every table in the source buffer, the values the launch derives -- and the
// checks of nxc_set_bounce's spline and nxc_set_stick_map's nodes.  The copies that would go to the
// device go into a host buffer of exactly the planned size, so a sanitizer sees every byte the
// upload would read and every offset it would write.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/desc_check.cpp -o desc_check && ./desc_check
// (or hipcc -x c++ with -Xarch_host -fsanitize=address,undefined).  Prints one line per case;
// exit status 0 when every good descriptor was accepted with the expected plan and every bad one
// refused with the expected text.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_desc_check.hpp"

namespace {

constexpr int NLON = 5, NLAT = 4, NODES = NLON * NLAT, CELLS = (NLON - 1) * (NLAT - 1);
constexpr int NV = 7, NA = 3, NZ = 4, NSP = 7, NK = 8, NCOEF = (NK - 4) * (NK - 4);
constexpr size_t NPCG = 4 * (NXC_PCG_BITS + NXC_PCG_VECS);
constexpr double TWO_PI = 6.283185307179586, UNIT_KM = 2440.0;
const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();

// every table a source can have, each exactly as long as the descriptor says
struct Tables {
    std::vector<double> map, map_cdf, lon1d, cdf1d, spot, tab_cdf, tab_v, tx, ty, coef;
    std::vector<double> speed_cdf, speed_v, alt_cdf, alt, az_cdf, az;
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

std::vector<double> ramp(int n)                // 0 .. 1
{
    std::vector<double> a(n);
    for (int k = 0; k < n; k++) a[k] = (double)k / (n - 1);
    return a;
}

// the cumulated masses (a + b) + (c + d) of the cells of a 2-D map, divided by the total
std::vector<double> cell_cdf(const std::vector<double> &map)
{
    std::vector<double> cdf(CELLS);
    double sum = 0.0;
    for (int i = 0; i + 1 < NLON; i++)
        for (int j = 0; j + 1 < NLAT; j++) {
            const double *p = &map[(size_t)i * NLAT + j];
            sum += (p[0] + p[1]) + (p[NLAT] + p[NLAT + 1]);
            cdf[(size_t)i * (NLAT - 1) + j] = sum;
        }
    for (double &c : cdf) c /= sum;
    cdf[CELLS - 1] = 1.0;
    return cdf;
}

Tables good_tables()
{
    Tables t;
    t.map.assign(NODES, 1.0);
    t.map[19] = t.map[15] = 0.0;               // two nodes without abundance ...
    t.map_cdf = cell_cdf(t.map);
    t.lon1d = ramp(NLON);
    for (double &x : t.lon1d) x *= TWO_PI;
    t.cdf1d = ramp(NLON);
    t.spot.assign(NODES, 0.25);                // mean / max = 0.2875: 32 / that is below the floor
    t.spot[7] = 1.0;
    t.tab_cdf = ramp(NSP); t.tab_v = axis(NSP, 4.0);
    t.tab_v[2] = -6.0;                         // the bound is on |v|
    t.tx = {50, 50, 50, 50, 800, 800, 800, 800};
    t.ty = {0, 0, 0, 0, 1, 1, 1, 1};
    t.coef.resize(NCOEF);
    for (int k = 0; k < NCOEF; k++) t.coef[k] = 0.1 * (k + 1);
    t.coef[5] = -2.5;
    t.speed_cdf = rising_rows(NV); t.speed_v = axis(NV, 5.0);
    t.alt_cdf = rising_rows(NA); t.alt = axis(NA, 1.5707963267948966);
    t.az_cdf = rising_rows(NZ); t.az = axis(NZ, TWO_PI);
    for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)19 * NV + k] = 0.0;   // ... one a placeholder
    return t;
}

// ---- one good descriptor per source kind ------------------------------------------------------------
nxc_source_desc uniform_flat()
{
    nxc_source_desc d;
    std::memset(&d, 0, sizeof d);
    d.endtime = 3600.0; d.exobase = 1.0; d.sinlat0 = -1.0; d.sinlat1 = 1.0; d.lon1 = TWO_PI;
    d.vprob = 3.0; d.vwidth = 1.0; d.unit_km = UNIT_KM; d.sinalt1 = 1.0; d.az1 = TWO_PI;
    d.angular_type = 1; d.seed = 5;
    return d;
}

nxc_source_desc tabulated(const Tables &t)
{
    nxc_source_desc d = uniform_flat();
    d.speed_type = 2; d.n_speed = NSP; d.speed_cdf = t.tab_cdf.data(); d.speed_v = t.tab_v.data();
    return d;
}

nxc_source_desc spot(const std::vector<double> &map, int nlon, int nlat)
{
    nxc_source_desc d = uniform_flat();
    d.spatial_type = 1; d.map_nlon = nlon; d.map_nlat = nlat; d.map = map.data();
    return d;
}

nxc_source_desc map2d(const Tables &t)
{
    nxc_source_desc d = uniform_flat();
    d.spatial_type = 2; d.map_nlon = NLON; d.map_nlat = NLAT; d.map = t.map.data();
    d.map_cdf = t.map_cdf.data(); d.map_lon0 = 0.0; d.map_lon1 = TWO_PI; d.map_s0 = -1.0; d.map_s1 = 1.0;
    return d;
}

nxc_source_desc map1d(const Tables &t)
{
    nxc_source_desc d = uniform_flat();
    d.spatial_type = 3; d.map_nlon = NLON; d.map = t.lon1d.data(); d.map_cdf = t.cdf1d.data();
    return d;
}

nxc_source_desc thermal(const Tables &t)
{
    nxc_source_desc d = uniform_flat();
    d.speed_type = 3; d.t0 = 100.0; d.t1 = 600.0; d.nx = d.ny = NK;
    d.tx = t.tx.data(); d.ty = t.ty.data(); d.coef = t.coef.data();
    return d;
}

nxc_source_desc describe(const Tables &t)      // a 2-D map with all three per-node tables
{
    nxc_source_desc d = map2d(t);
    d.speed_type = 4; d.angular_type = 2;
    d.n_node_speed = NV; d.node_speed_cdf = t.speed_cdf.data(); d.node_speed_v = t.speed_v.data();
    d.n_node_alt = NA; d.node_alt_cdf = t.alt_cdf.data(); d.node_alt = t.alt.data();
    d.n_node_az = NZ; d.node_az_cdf = t.az_cdf.data(); d.node_az = t.az.data();
    return d;
}

nxc_source_desc pcg(nxc_source_desc d)
{
    d.generator = 1; d.pcg_state[0] = 0x0123456789abcdefULL; d.pcg_state[1] = 42;
    d.pcg_inc[0] = 0xfedcba9876543210ULL; d.pcg_inc[1] = 0x1234567ULL;
    d.pcg_n = 4000; d.pcg_row0 = 3000;
    return d;
}

// ---- what a good descriptor's plan must be ---------------------------------------------------------
// the sizes by which the buffer is laid out (zero: the source has no such table), and the derived values
struct Want {
    size_t n_sp = 0, n_map = 0, n_mcdf = 0, n_pcg = 0, nx = 0, ny = 0, n_coef = 0, nodes = 0, nv = 0, na = 0, nz = 0;
    int law = NXC_LAW_PLAIN;
    double vmax = 0.0;                         // km/s; < 0: the device finds it (k2max -1)
    int max_trials = NXC_SPOT_MIN_TRIALS;
    double map_max = 0.0, map_dlon = 0.0, map_ds = 0.0;
    int64_t stride = 1000, offset = 0;
};

std::string plan_mismatch(const SourcePlan &P, const Want &w)
{
    const size_t at_spl = 2 * w.n_sp + w.n_map + w.n_mcdf + w.n_pcg, at_nodes = at_spl + w.nx + w.ny + w.n_coef;
    const size_t at_alt = at_nodes + w.nodes * w.nv + w.nv, at_az = at_alt + w.nodes * w.na + w.na;
    const size_t at[ST_COUNT] = {0, w.n_sp, 2 * w.n_sp, 2 * w.n_sp + w.n_map, 0, at_spl, at_spl + w.nx,
                                 at_spl + w.nx + w.ny, at_nodes, at_nodes + w.nodes * w.nv, at_alt,
                                 at_alt + w.nodes * w.na, at_az, at_az + w.nodes * w.nz};
    const size_t count[ST_COUNT] = {w.n_sp, w.n_sp, w.n_map, w.n_mcdf, w.n_pcg, w.nx, w.ny, w.n_coef,
                                    w.nodes * w.nv, w.nv, w.nodes * w.na, w.na, w.nodes * w.nz, w.nz};
    // the copies, into a buffer of exactly the planned size: they tile it without gap or overlap
    std::vector<double> staged(P.total);
    size_t end = 0;
    for (int t = 0; t < ST_COUNT; t++) {
        const TableCopy &c = P.copy[t];
        if (c.count != count[t]) return "table " + std::to_string(t) + " has the wrong size";
        if (c.count && c.at != at[t]) return "table " + std::to_string(t) + " is at the wrong offset";
        if (c.at != end) return "staging leaves a gap or overlaps at table " + std::to_string(t);
        if (c.count) std::memcpy(staged.data() + c.at, c.from, c.count * sizeof(double));
        end = c.at + c.count;
    }
    if (end != P.total || P.total != at_az + w.nodes * w.nz + w.nz) return "staged size does not match the plan";
    if (w.n_pcg) {          // the first PCG64 map is one step: {multiplier, increment}
        u128 first[2];
        std::memcpy(first, staged.data(), sizeof first);
        if (first[0] != PCG_MULT || (uint64_t)first[1] != 0x1234567ULL) return "PCG64 maps are not at the start";
    }
    if (P.law != w.law) return "law " + std::to_string(P.law);
    if (P.stride != w.stride || P.offset != w.offset) return "stride / offset";
    const double bound = w.vmax / UNIT_KM;
    if (P.k2max != (w.vmax < 0 ? -1.0 : bound * bound)) return "k2max " + std::to_string(P.k2max);
    if (P.max_trials != w.max_trials) return "max_trials " + std::to_string(P.max_trials);
    if (P.map_max != w.map_max || P.map_dlon != w.map_dlon || P.map_ds != w.map_ds) return "map_max / spacings";
    return "";
}

int failures = 0;

void report(const char *what, bool got, bool want, const std::string &why)
{
    std::printf("%-52s %s%s%s\n", what, got ? "accepted" : "refused", why.empty() ? "" : ": ", why.c_str());
    if (got != want) { failures++; std::printf("    ^ expected to be %s\n", want ? "accepted" : "refused"); }
}

// a good descriptor: accepted, and planned as `w` says
void accept(const char *what, const nxc_source_desc &d, const Want &w, int64_t n = 1000)
{
    const SourcePlan P = plan_source(&d, n);
    const std::string why = P.why.empty() ? plan_mismatch(P, w) : P.why;
    report(what, why.empty(), true, why);
}

// a refusal whose text must hold `text`
void refused(const char *what, const std::string &why, const char *text)
{
    report(what, why.empty(), false, why);
    if (!why.empty() && why.find(text) == std::string::npos) {
        failures++;
        std::printf("    ^ expected the text \"%s\"\n", text);
    }
}

void refuse(const char *what, const nxc_source_desc &d, const char *text, int64_t n = 1000)
{
    refused(what, plan_source(&d, n).why, text);
}

Want node_want(size_t nv, size_t na, size_t nz, double vmax)
{
    Want w;
    w.n_map = NODES; w.n_mcdf = CELLS; w.nodes = NODES; w.nv = nv; w.na = na; w.nz = nz;
    w.law = NXC_LAW_NODES; w.vmax = vmax; w.map_dlon = TWO_PI / (NLON - 1); w.map_ds = 2.0 / (NLAT - 1);
    return w;
}

}  // namespace

int main()
{
    const Tables good = good_tables();
    const double node_vmax = good.speed_v[NV - 1];

    // ---- one good descriptor per source kind
    { Want w; w.vmax = 3.0 + 1.0; accept("uniform surface, flat speeds", uniform_flat(), w); }
    { nxc_source_desc d = uniform_flat(); d.speed_type = 1;
      Want w; w.vmax = 3.0 + 6 * 1.0; accept("gaussian speeds", d, w); }
    { Want w; w.n_sp = NSP; w.vmax = 6.0; accept("tabulated speeds", tabulated(good), w); }
    { Want w; w.n_map = NODES; w.map_max = 1.0; w.vmax = 4.0;
      accept("spot map 5 x 4 (trials at the floor)", spot(good.spot, NLON, NLAT), w); }
    { std::vector<double> one(64 * 64, 0.0); one[100] = 2.0;       // mean / max = 1 / 4096
      Want w; w.n_map = one.size(); w.map_max = 2.0; w.vmax = 4.0; w.max_trials = 32 * 4096;
      accept("spot map 64 x 64 (trials = 32 / acceptance)", spot(one, 64, 64), w); }
    { std::vector<double> one(600 * 600, 0.0); one[100] = 2.0;     // 32 * 360000 trials: the ceiling
      Want w; w.n_map = one.size(); w.map_max = 2.0; w.vmax = 4.0; w.max_trials = NXC_SPOT_MAX_TRIALS;
      accept("spot map 600 x 600 (trials at the ceiling)", spot(one, 600, 600), w); }
    { Want w = node_want(0, 0, 0, 4.0); w.law = NXC_LAW_PLAIN; accept("2-D surface map", map2d(good), w); }
    { Want w; w.n_map = NLON; w.n_mcdf = NLON; w.vmax = 4.0; accept("1-D surface map", map1d(good), w); }
    Want thermal_want;
    thermal_want.nx = thermal_want.ny = NK; thermal_want.n_coef = NCOEF; thermal_want.law = NXC_LAW_THERMAL;
    thermal_want.vmax = 2.5;
    accept("thermal speeds", thermal(good), thermal_want);
    accept("all three tables", describe(good), node_want(NV, NA, NZ, node_vmax));
    { nxc_source_desc d = describe(good); d.angular_type = 1; accept("speeds only", d, node_want(NV, 0, 0, node_vmax)); }
    { nxc_source_desc d = describe(good); d.speed_type = 0; accept("angles only", d, node_want(0, NA, NZ, 4.0)); }
    { nxc_source_desc d = describe(good); d.speed_type = 0; d.angular_type = 1; d.node_speed_cdf = nullptr;
      Want w = node_want(0, 0, 0, 4.0); w.law = NXC_LAW_PLAIN; accept("no per-node law at all", d, w); }
    { nxc_source_desc d = describe(good); d.speed_type = 2; d.n_speed = NSP; d.speed_cdf = good.tab_cdf.data();
      d.speed_v = good.tab_v.data();
      Want w = node_want(0, NA, NZ, 6.0); w.n_sp = NSP; accept("tabulated speeds with per-node directions", d, w); }
    { Want w; w.n_pcg = NPCG; w.vmax = 4.0; accept("PCG64, uniform surface, flat speeds", pcg(uniform_flat()), w); }
    { Want w = thermal_want; w.n_pcg = NPCG; accept("PCG64, thermal speeds", pcg(thermal(good)), w); }
    { nxc_source_desc d = tabulated(good); d.dest_total = 3000; d.dest_offset = 1000;
      Want w; w.n_sp = NSP; w.vmax = -1.0; w.stride = 3000; w.offset = 1000; accept("one piece of a larger set", d, w); }
    { nxc_source_desc d = uniform_flat(); d.dest_total = 3000; d.dest_offset = 2000;
      Want w; w.vmax = -1.0; w.stride = 3000; w.offset = 2000; accept("the last piece of a set", d, w); }

    // ---- one bad descriptor per refusal, in the order nxc_packets_sample meets them
    refuse("no packets", uniform_flat(), "bad arguments", 0);
    refused("no descriptor", plan_source(nullptr, 1000).why, "bad arguments");
    { nxc_source_desc d = uniform_flat(); d.unit_km = 0.0; refuse("unit_km 0", d, "bad nxc_source_desc"); }
    { nxc_source_desc d = uniform_flat(); d.speed_type = 5; refuse("speed_type 5", d, "bad nxc_source_desc"); }
    { nxc_source_desc d = uniform_flat(); d.generator = 2; refuse("generator 2", d, "generator must be 0 or 1"); }
    refuse("PCG64 with tabulated speeds", pcg(tabulated(good)), "generator 1 (PCG64) covers the sources");
    refuse("PCG64 stream", pcg(describe(good)), "generator 1 (PCG64) covers the sources");
    { nxc_source_desc d = pcg(uniform_flat()); d.pcg_row0 = 3001;
      refuse("PCG64 rows past the draw vectors", d, "PCG64 window outside its draw vectors"); }
    { nxc_source_desc d = pcg(uniform_flat()); d.pcg_inc[1] = 2;
      refuse("PCG64 with an even increment", d, "PCG64 window outside its draw vectors"); }
    { nxc_source_desc d = tabulated(good); d.n_speed = 1;
      refuse("one tabulated speed", d, "tabulated speeds need n_speed >= 2 and both tables"); }
    { nxc_source_desc d = describe(good); d.speed_type = 2;
      refuse("tabulated speeds without their table", d, "tabulated speeds need n_speed >= 2 and both tables"); }
    { Tables t = good; t.tab_cdf[3] = 0.1; refuse("decreasing speed_cdf", tabulated(t), "speed_cdf must be non-decreasing"); }
    { Tables t = good; t.tab_cdf.assign(NSP, 0.5); refuse("flat speed_cdf", tabulated(t), "speed_cdf is flat"); }
    { nxc_source_desc d = thermal(good); d.t0 = 0.0;
      refuse("thermal speeds at t0 = 0", d, "thermal speeds need finite t0 > 0 and t1 >= 0"); }
    { nxc_source_desc d = thermal(good); d.nx = 7;
      refuse("thermal spline with 7 knots", d, "nxc_source_desc: thermal speeds need a spline with 8..65536 knots"); }
    { Tables t = good; t.tx[1] = NaN; refuse("thermal spline, NaN knot", thermal(t), "nxc_source_desc: thermal spline knots tx must be finite"); }
    { Tables t = good; t.ty[4] = 0.0; refuse("thermal spline, empty inner interval", thermal(t), "spline knots ty must be finite, non-decreasing and increasing inside"); }
    { Tables t = good; t.coef[9] = INF; refuse("thermal spline, infinite coefficient", thermal(t), "spline coefficients must be finite (coef 9)"); }
    { Tables t = good; t.tx[6] = 700.0;
      refused("bounce spline, decreasing knots",
              check_bicubic_spline("nxc_bounce_desc: accommodated", NK, NK, t.tx.data(), t.ty.data(), t.coef.data(), nullptr),
              "nxc_bounce_desc: accommodated spline knots tx must be finite"); }
    { nxc_source_desc d = spot(good.spot, NLON, NLAT); d.map = nullptr; refuse("spot without its map", d, "surface spot needs a density map"); }
    { Tables t = good; t.spot[3] = -1.0; refuse("negative spot map", spot(t.spot, NLON, NLAT), "density map values must be finite and >= 0"); }
    { Tables t = good; t.spot.assign(NODES, 0.0); refuse("spot map of zeros", spot(t.spot, NLON, NLAT), "density map is all zero"); }
    { nxc_source_desc d = map2d(good); d.map_cdf = nullptr;
      refuse("surface map without its cdf", d, "a surface map needs 2..8192 nodes per axis, map and map_cdf"); }
    { Tables t = good; t.map[7] = -1.0; refuse("negative map node", map2d(t), "surface map values must be finite and >= 0 (node 7)"); }
    { Tables t = good; t.map.assign(NODES, 0.0); refuse("surface map of zeros", map2d(t), "surface map is all zero"); }
    { Tables t = good; t.map_cdf[CELLS - 1] = 0.5; refuse("map_cdf that stops at 0.5", map2d(t), "map_cdf must run from >= 0 to 1"); }
    { Tables t = good; t.map_cdf[4] = 0.01; refuse("decreasing map_cdf", map2d(t), "map_cdf must be non-decreasing"); }
    { Tables t = good; t.cdf1d.assign(NLON, 1.0); refuse("flat cdf of a 1-D map", map1d(t), "map_cdf is flat"); }
    { nxc_source_desc d = map2d(good); d.map_lon1 = d.map_lon0;
      refuse("surface map without longitude extent", d, "surface map needs map_lon0 < map_lon1"); }
    { nxc_source_desc d = uniform_flat(); d.dest_total = 3000; d.dest_offset = 2500;
      refuse("piece past the end of its set", d, "piece outside its set"); }

    // ---- per-node tables
    { Tables t = good; t.speed_cdf[(size_t)3 * NV + 4] = 0.1;
      refuse("decreasing speed row", describe(t), "node_speed_cdf: row of node 3 must be non-decreasing"); }
    { Tables t = good; for (int k = 0; k < NA; k++) t.alt_cdf[(size_t)6 * NA + k] *= 0.5;
      refuse("altitude row that does not reach 1", describe(t), "node_alt_cdf: row of node 6"); }
    { Tables t = good; t.az_cdf[(size_t)2 * NZ] = 0.25;
      refuse("azimuth row that does not start at 0", describe(t), "node_az_cdf: row of node 2"); }
    { Tables t = good; t.speed_cdf[(size_t)8 * NV + 2] = NaN; refuse("NaN in a speed row", describe(t), "node_speed_cdf: row of node 8"); }
    { Tables t = good; for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)7 * NV + k] = 0.0;
      refuse("placeholder at a node with abundance", describe(t), "node_speed_cdf: row of node 7"); }
    { Tables t = good; for (int k = 0; k < NV; k++) t.speed_cdf[(size_t)15 * NV + k] = 0.5;
      refuse("flat row that is not the placeholder", describe(t), "node_speed_cdf: row of node 15"); }
    { Tables t = good; t.speed_v[NV - 1] = INF; refuse("infinite speed axis", describe(t), "node_speed: axis must be finite (entry 6)"); }
    { nxc_source_desc d = describe(good); d.spatial_type = 0; refuse("tables with spatial_type 0", d, "need a 2-D surface map (spatial_type 2)"); }
    { nxc_source_desc d = describe(good); d.spatial_type = 3; d.map = good.lon1d.data(); d.map_cdf = good.cdf1d.data();
      refuse("tables with a 1-D map", d, "need a 2-D surface map (spatial_type 2)"); }
    { nxc_source_desc d = describe(good); d.speed_type = 3; d.t0 = 100.0; d.t1 = 600.0; d.nx = d.ny = NK;
      d.tx = good.tx.data(); d.ty = good.ty.data(); d.coef = good.coef.data();
      refuse("thermal speeds with per-node directions", d, "(angular_type 2) are not implemented"); }
    { nxc_source_desc d = describe(good); d.n_node_speed = 1; refuse("one entry per speed row", d, "node_speed needs 2..65536 entries per row"); }
    { nxc_source_desc d = describe(good); d.n_node_az = 0; refuse("no azimuth entries", d, "node_az needs 2..65536 entries per row"); }
    { nxc_source_desc d = describe(good); d.n_node_alt = NXC_NODE_TABLE_MAX + 1;
      refuse("too many altitude entries", d, "node_alt needs 2..65536 entries per row"); }
    { nxc_source_desc d = describe(good); d.node_speed_cdf = nullptr; refuse("speed_type 4 without its table", d, "node_speed needs 2..65536 entries per row"); }
    { nxc_source_desc d = describe(good); d.node_az = nullptr; refuse("azimuth table without its axis", d, "node_az needs 2..65536 entries per row"); }

    // ---- the sticking map of nxc_set_stick_map
    const std::vector<double> lon = {0.0, 1.0, 2.0, 6.0}, lat = {-1.5, 0.0, 1.5}, stick(12, 0.5);
    const nxc_stick_map_desc smap = {4, 3, lon.data(), lat.data(), stick.data()};
    report("sticking map 4 x 3", check_stick_map(&smap).empty(), true, check_stick_map(&smap));
    { nxc_stick_map_desc m = smap; m.nlat = 0; m.lat = nullptr;
      report("sticking map of longitude only", check_stick_map(&m).empty(), true, check_stick_map(&m)); }
    { nxc_stick_map_desc m = smap; m.nlon = 1; refused("sticking map with one longitude", check_stick_map(&m), "2..65536 longitude nodes, 0 or 2..65536 latitude nodes"); }
    { std::vector<double> l = lon; l[2] = 0.5; nxc_stick_map_desc m = smap; m.lon = l.data();
      refused("sticking map, longitudes out of order", check_stick_map(&m), "longitude nodes must increase within [0, 2 pi) (lon 2)"); }
    { std::vector<double> l = lat; l[0] = -1.6; nxc_stick_map_desc m = smap; m.lat = l.data();
      refused("sticking map, latitude below the pole", check_stick_map(&m), "latitude nodes must increase within [-pi/2, pi/2] (lat 0)"); }
    { std::vector<double> c = stick; c[5] = 1.5; nxc_stick_map_desc m = smap; m.coef = c.data();
      refused("sticking map, coefficient above 1", check_stick_map(&m), "coefficients must lie in [0, 1] (coef 5 = 1.500000)"); }
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
