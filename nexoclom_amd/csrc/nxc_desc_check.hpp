// Host-only side of the descriptors whose tables go to the device: what a source (nxc_packets_sample),
// a bicubic spline (nxc_set_bounce, thermal speeds) and a sticking map (nxc_set_stick_map) must
// satisfy before anything is launched, and -- for a source -- where each table goes in the handle's
// source buffer and what the launch derives from the tables.  Plain C++ without a device call or a
// handle: a refusal is a text, which nxc_api.hip hands to fail().  So the whole of it can also be
// built into a stand-alone program and run under the host sanitizers (tests/tools/desc_check.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nexoclom_hip.h"
#include "nxc_source_limits.hpp"

// Affine maps of NumPy's PCG64 for the device sampler (nxc_kernels.hpp: PcgK): entry b <
// NXC_PCG_BITS advances 2^b steps, entry NXC_PCG_BITS + v advances v*n steps (the start of draw
// vector v).  state' = mult^d state + inc (mult^d - 1)/(mult - 1), accumulated by squaring like
// pcg_advance_lcg_128 (numpy/random/src/pcg64/pcg64.c).
typedef unsigned __int128 u128;
constexpr u128 PCG_MULT = ((u128)2549297995355413924ULL << 64) | 4865540595714422341ULL;

inline void pcg_advance_map(u128 delta, u128 inc, u128 *a_out, u128 *c_out)
{
    u128 acc_mult = 1, acc_plus = 0, cur_mult = PCG_MULT, cur_plus = inc;
    while (delta > 0) {
        if (delta & 1) {
            acc_mult *= cur_mult;
            acc_plus = acc_plus * cur_mult + cur_plus;
        }
        cur_plus = (cur_mult + 1) * cur_plus;
        cur_mult *= cur_mult;
        delta >>= 1;
    }
    *a_out = acc_mult;
    *c_out = acc_plus;
}

inline std::vector<u128> pcg_tables(u128 inc, int64_t n)
{
    std::vector<u128> t((size_t)2 * (NXC_PCG_BITS + NXC_PCG_VECS));
    for (int b = 0; b < NXC_PCG_BITS; b++) pcg_advance_map((u128)1 << b, inc, &t[2 * b], &t[2 * b + 1]);
    for (int v = 0; v < NXC_PCG_VECS; v++)
        pcg_advance_map((u128)v * (u128)n, inc, &t[2 * (NXC_PCG_BITS + v)], &t[2 * (NXC_PCG_BITS + v) + 1]);
    return t;
}

// What bispev3 needs of a bicubic spline (FITPACK layout) to stay finite: 8..65536 finite,
// non-decreasing knots per axis that increase inside [t[3], t[n-4]] (a zero-width interval there
// would divide by zero) and finite coefficients.  One check for every entry that takes such a
// spline (nxc_set_bounce with accommodation, nxc_packets_sample speed_type 3).  "" or the reason,
// which `who` starts; *coef_max receives max |coef|.
inline std::string check_bicubic_spline(const char *who, int64_t nx, int64_t ny, const double *tx,
                                        const double *ty, const double *coef, double *coef_max)
{
    if (nx < 8 || ny < 8 || nx > (1 << 16) || ny > (1 << 16) || !tx || !ty || !coef)
        return std::string(who) + " speeds need a spline with 8..65536 knots per axis, tx, ty and coef";
    for (int axis = 0; axis < 2; axis++) {
        const double *t = axis ? ty : tx;
        const int64_t nk = axis ? ny : nx;
        for (int64_t k = 0; k < nk; k++)
            if (!std::isfinite(t[k]) || (k > 0 && !(t[k] >= t[k - 1])) ||
                (k > 3 && k <= nk - 4 && !(t[k] > t[k - 1])))
                return std::string(who) + " spline knots " + (axis ? "ty" : "tx") +
                       " must be finite, non-decreasing and increasing inside [t[3], t[n-4]]";
    }
    double big = 0.0;
    const int64_t n_coef = (nx - 4) * (ny - 4);
    for (int64_t k = 0; k < n_coef; k++) {
        if (!std::isfinite(coef[k]))
            return std::string(who) + " spline coefficients must be finite (coef " + std::to_string(k) + ")";
        big = std::max(big, std::fabs(coef[k]));
    }
    if (coef_max) *coef_max = big;
    return "";
}

// "" when the sticking map can be interpolated (nexoclom_hip.h: nxc_stick_map_desc), else the reason.
inline std::string check_stick_map(const nxc_stick_map_desc *d)
{
    const double TWO_PI = 6.283185307179586, HALF_PI = 1.5707963267948966;
    const int64_t nlon = d->nlon, nlat = d->nlat;
    if (nlon < 2 || nlon > (1 << 16) || nlat < 0 || nlat == 1 || nlat > (1 << 16) || !d->lon ||
        !d->coef || (nlat && !d->lat))
        return "nxc_stick_map_desc: 2..65536 longitude nodes, 0 or 2..65536 latitude nodes, lon, coef "
               "(and lat)";
    for (int64_t k = 0; k < nlon; k++)
        if (!(d->lon[k] >= 0 && d->lon[k] < TWO_PI) || (k > 0 && !(d->lon[k] > d->lon[k - 1])))
            return "nxc_stick_map_desc: longitude nodes must increase within [0, 2 pi) (lon " +
                   std::to_string(k) + ")";
    for (int64_t k = 0; k < nlat; k++)
        if (!(d->lat[k] >= -HALF_PI && d->lat[k] <= HALF_PI) || (k > 0 && !(d->lat[k] > d->lat[k - 1])))
            return "nxc_stick_map_desc: latitude nodes must increase within [-pi/2, pi/2] (lat " +
                   std::to_string(k) + ")";
    for (int64_t k = 0; k < nlon * (nlat ? nlat : 1); k++)
        if (!(d->coef[k] >= 0 && d->coef[k] <= 1))
            return "nxc_stick_map_desc: coefficients must lie in [0, 1] (coef " + std::to_string(k) +
                   " = " + std::to_string(d->coef[k]) + ")";
    return "";
}

// One per-node table: n entries per row, a finite axis, and per node a cdf that is non-decreasing
// from 0 to 1 -- or all zeros where the node's value in the map is 0 (a node that is never drawn).
inline std::string check_node_table(const char *name, int64_t n, const double *cdf, const double *axis,
                                    const double *map, int64_t nodes)
{
    const std::string what = std::string("nxc_source_desc: ") + name;
    if (n < 2 || n > NXC_NODE_TABLE_MAX || !cdf || !axis)
        return what + " needs 2..65536 entries per row, the cdf table and its axis";
    for (int64_t k = 0; k < n; k++)
        if (!std::isfinite(axis[k])) return what + ": axis must be finite (entry " + std::to_string(k) + ")";
    for (int64_t c = 0; c < nodes; c++) {
        const double *row = cdf + c * n;
        bool rising = row[0] == 0.0 && row[n - 1] == 1.0, zero = row[0] == 0.0;
        for (int64_t k = 1; k < n; k++) {
            rising = rising && row[k] >= row[k - 1];
            zero = zero && row[k] == 0.0;
        }
        if (!rising && !(zero && map[c] == 0.0))
            return what + "_cdf: row of node " + std::to_string(c) + " must be non-decreasing from 0 "
                   "to 1 (all zeros only where the node's map value is 0)";
    }
    return "";
}

// The per-node tables of a surface map (speed_type 4, angular_type 2), after the map itself.
inline std::string check_node_tables(const nxc_source_desc *d)
{
    const bool speed = d->speed_type == 4, angles = d->angular_type == 2;
    if (!speed && !angles) return "";
    if (d->spatial_type != 2)
        return "nxc_source_desc: per-node tables (speed_type 4, angular_type 2) need a 2-D surface "
               "map (spatial_type 2)";
    // k_sample<NXC_LAW_NODES> holds no thermal code: speed_type 3 would fall through to the
    // tabulated branch and read the speed_cdf it does not have
    if (d->speed_type == 3)
        return "nxc_source_desc: thermal speeds (speed_type 3) with per-node directions "
               "(angular_type 2) are not implemented";
    const int64_t nodes = d->map_nlon * d->map_nlat;
    std::string why;
    if (speed)
        why = check_node_table("node_speed", d->n_node_speed, d->node_speed_cdf, d->node_speed_v, d->map, nodes);
    if (why.empty() && angles)
        why = check_node_table("node_alt", d->n_node_alt, d->node_alt_cdf, d->node_alt, d->map, nodes);
    if (why.empty() && angles)
        why = check_node_table("node_az", d->n_node_az, d->node_az_cdf, d->node_az, d->map, nodes);
    return why;
}

// ---- a source: nxc_source_desc -> what nxc_packets_sample uploads and launches --------------------
// The tables of a source in the order they lie in the source buffer, each behind the one before;
// a table the source does not have has count 0.  (PCG64 goes with neither tabulated speeds nor maps
// nor per-node tables -- generator 1 is refused for them -- so its maps start the buffer.)
enum SourceTable {
    ST_SPEED_CDF, ST_SPEED_V, ST_MAP, ST_MAP_CDF, ST_PCG, ST_TX, ST_TY, ST_COEF,
    ST_NODE_SPEED_CDF, ST_NODE_SPEED_V, ST_NODE_ALT_CDF, ST_NODE_ALT, ST_NODE_AZ_CDF, ST_NODE_AZ,
    ST_COUNT
};

struct TableCopy {
    size_t at;                 // offset in the source buffer, in doubles
    const void *from;
    size_t count;              // doubles
};

struct SourcePlan {
    std::string why;                       // "" when the descriptor can be launched from, else the refusal
    TableCopy copy[ST_COUNT] = {};
    size_t total = 0;                      // doubles, all tables
    std::vector<u128> pcg_maps;            // what copy[ST_PCG] reads: it lives as long as the plan
    int law = NXC_LAW_PLAIN;               // which k_sample
    int64_t stride = 0, offset = 0;        // the n packets are [offset, offset + n) of a set of stride
    double map_max = 0.0;                  // spot: accept/reject ceiling
    int max_trials = NXC_SPOT_MIN_TRIALS;  // spot: 32 / acceptance rate, clamped
    double map_dlon = 0.0, map_ds = 0.0;   // 2-D map: node spacing of each axis
    double coef_max = 0.0;                 // thermal: max |coef|
    double k2max = -1.0;                   // square of the launch-speed bound [R/s]; -1: ask the device
    SourcePlan() = default;
    SourcePlan(SourcePlan &&) = default;   // (not copied: copy[ST_PCG] points into pcg_maps)
};

// The refusal of a descriptor, in the order a caller meets them, or ""; fills what the checks
// compute on their way (map_max, max_trials, coef_max, stride, offset).
inline std::string check_source(const nxc_source_desc *d, int64_t n, SourcePlan &P)
{
    if (!d || n < 1) return "bad arguments";
    if (d->speed_type < 0 || d->speed_type > 4 || d->angular_type < 0 || d->angular_type > 2 ||
        d->spatial_type < 0 || d->spatial_type > 3 || !(d->unit_km > 0) || !(d->exobase > 0))
        return "bad nxc_source_desc";
    const bool map2d = d->spatial_type == 2, map1d = d->spatial_type == 3;
    if (d->generator != 0 && d->generator != 1) return "nxc_source_desc: generator must be 0 or 1";
    if (d->generator == 1) {
        if (d->spatial_type != 0 || (d->speed_type != 0 && d->speed_type != 3))
            return "generator 1 (PCG64) covers the sources whose every draw is a random(npackets) "
                   "vector: uniform surface, flat or thermal speeds";
        if (d->pcg_n < 1 || d->pcg_row0 < 0 || d->pcg_row0 + n > d->pcg_n ||
            d->pcg_n >= ((int64_t)1 << (NXC_PCG_BITS - 1)) || !(d->pcg_inc[1] & 1ull))
            return "nxc_source_desc: PCG64 window outside its draw vectors";
    }
    if (d->speed_type == 2) {
        if (d->n_speed < 2 || d->n_speed > (1 << 24) || !d->speed_cdf || !d->speed_v)
            return "nxc_source_desc: tabulated speeds need n_speed >= 2 and both tables";
        for (int64_t k = 0; k + 1 < d->n_speed; k++)
            if (!(d->speed_cdf[k + 1] >= d->speed_cdf[k]))
                return "nxc_source_desc: speed_cdf must be non-decreasing";
        if (!(d->speed_cdf[d->n_speed - 1] > d->speed_cdf[0])) return "nxc_source_desc: speed_cdf is flat";
    }
    // thermal speeds: the surface temperature's constants and the v(T, p) spline
    if (d->speed_type == 3) {
        if (!(d->t0 > 0.0) || !std::isfinite(d->t0) || !(d->t1 >= 0.0) || !std::isfinite(d->t1))
            return "nxc_source_desc: thermal speeds need finite t0 > 0 and t1 >= 0";
        const std::string why = check_bicubic_spline("nxc_source_desc: thermal", d->nx, d->ny, d->tx,
                                                     d->ty, d->coef, &P.coef_max);
        if (!why.empty()) return why;
    }
    if (d->spatial_type == 1) {
        if (d->map_nlon < 2 || d->map_nlat < 2 || d->map_nlon > 8192 || d->map_nlat > 8192 || !d->map)
            return "nxc_source_desc: surface spot needs a density map";
        double map_sum = 0.0;
        for (int64_t k = 0; k < d->map_nlon * d->map_nlat; k++) {
            if (!(d->map[k] >= 0.0) || !std::isfinite(d->map[k]))
                return "nxc_source_desc: density map values must be finite and >= 0";
            P.map_max = std::max(P.map_max, d->map[k]);
            map_sum += d->map[k];
        }
        if (!(P.map_max > 0.0)) return "nxc_source_desc: density map is all zero";
        // acceptance rate of the uniform (lon, lat) proposal = mean / max of the map: a narrow spot
        // (sigma 0.05 rad: 8e-4) needs tens of thousands of trials for the unluckiest of 1e6 packets
        const double want = 32.0 / (map_sum / (double)(d->map_nlon * d->map_nlat) / P.map_max);
        P.max_trials = want > (double)NXC_SPOT_MAX_TRIALS ? NXC_SPOT_MAX_TRIALS
                       : (want < (double)NXC_SPOT_MIN_TRIALS ? NXC_SPOT_MIN_TRIALS : (int)want);
    }
    // surface map: node values [map_nlon][map_nlat] with the cumulated masses of the
    // (map_nlon - 1) x (map_nlat - 1) cells; 1-D map: longitude grid [map_nlon] with its cdf
    if (map2d || map1d) {
        if (d->map_nlon < 2 || d->map_nlon > 8192 || (map2d && (d->map_nlat < 2 || d->map_nlat > 8192)) ||
            !d->map || !d->map_cdf)
            return "nxc_source_desc: a surface map needs 2..8192 nodes per axis, map and map_cdf";
        const int64_t n_nodes = map2d ? d->map_nlon * d->map_nlat : d->map_nlon;
        const int64_t n_cdf = map2d ? (d->map_nlon - 1) * (d->map_nlat - 1) : d->map_nlon;
        double node_max = 0.0;
        for (int64_t k = 0; k < n_nodes; k++) {
            // (a 1-D map's `map` is its longitude grid: finite is all it has to be)
            if (!std::isfinite(d->map[k]) || (map2d && !(d->map[k] >= 0.0)))
                return "nxc_source_desc: surface map values must be finite and >= 0 (node " +
                       std::to_string(k) + ")";
            node_max = std::max(node_max, d->map[k]);
        }
        if (map2d && !(node_max > 0.0)) return "nxc_source_desc: surface map is all zero";
        if (!(d->map_cdf[0] >= 0.0) || !(d->map_cdf[n_cdf - 1] == 1.0))
            return "nxc_source_desc: map_cdf must run from >= 0 to 1 (is the map all zero?)";
        for (int64_t k = 0; k + 1 < n_cdf; k++)
            if (!(d->map_cdf[k + 1] >= d->map_cdf[k])) return "nxc_source_desc: map_cdf must be non-decreasing";
        if (map1d && !(d->map_cdf[n_cdf - 1] > d->map_cdf[0])) return "nxc_source_desc: map_cdf is flat";
        if (map2d && (!std::isfinite(d->map_lon0) || !std::isfinite(d->map_lon1) ||
                      !(d->map_lon0 < d->map_lon1) || !(d->map_s0 >= -1.0) || !(d->map_s1 <= 1.0) ||
                      !(d->map_s0 < d->map_s1)))
            return "nxc_source_desc: surface map needs map_lon0 < map_lon1 and -1 <= map_s0 < map_s1 <= 1";
    }
    const std::string why = check_node_tables(d);
    if (!why.empty()) return why;
    P.stride = d->dest_total > 0 ? d->dest_total : n;
    P.offset = d->dest_total > 0 ? d->dest_offset : 0;
    if (P.offset < 0 || P.offset + n > P.stride) return "nxc_source_desc: piece outside its set";
    return "";
}

// Everything nxc_packets_sample does with a descriptor before its first device call: the refusal,
// or where each table goes and what the launch needs of them.
inline SourcePlan plan_source(const nxc_source_desc *d, int64_t n)
{
    SourcePlan P;
    P.why = check_source(d, n, P);
    if (!P.why.empty()) return P;
    const bool map2d = d->spatial_type == 2, thermal = d->speed_type == 3;
    const bool node_speed = d->speed_type == 4, node_angles = d->angular_type == 2;
    const size_t n_sp = d->speed_type == 2 ? (size_t)d->n_speed : 0;
    const size_t nodes = d->spatial_type == 1 || map2d ? (size_t)(d->map_nlon * d->map_nlat) : 0;
    const size_t n_map = d->spatial_type == 3 ? (size_t)d->map_nlon : nodes;
    const size_t n_mcdf = map2d ? (size_t)((d->map_nlon - 1) * (d->map_nlat - 1))
                                : (d->spatial_type == 3 ? (size_t)d->map_nlon : 0);
    if (d->generator == 1) P.pcg_maps = pcg_tables(((u128)d->pcg_inc[0] << 64) | d->pcg_inc[1], d->pcg_n);
    const size_t n_nv = node_speed ? (size_t)d->n_node_speed : 0;
    const size_t n_na = node_angles ? (size_t)d->n_node_alt : 0, n_nz = node_angles ? (size_t)d->n_node_az : 0;
    const TableCopy tables[ST_COUNT] = {
        {0, d->speed_cdf, n_sp}, {0, d->speed_v, n_sp}, {0, d->map, n_map}, {0, d->map_cdf, n_mcdf},
        {0, P.pcg_maps.data(), P.pcg_maps.size() * (sizeof(u128) / sizeof(double))},
        {0, d->tx, thermal ? (size_t)d->nx : 0}, {0, d->ty, thermal ? (size_t)d->ny : 0},
        {0, d->coef, thermal ? (size_t)((d->nx - 4) * (d->ny - 4)) : 0},
        {0, d->node_speed_cdf, nodes * n_nv}, {0, d->node_speed_v, n_nv},
        {0, d->node_alt_cdf, nodes * n_na}, {0, d->node_alt, n_na},
        {0, d->node_az_cdf, nodes * n_nz}, {0, d->node_az, n_nz}};
    for (int t = 0; t < ST_COUNT; t++) {
        P.copy[t] = {P.total, tables[t].from, tables[t].count};
        P.total += tables[t].count;
    }
    P.law = node_speed || node_angles ? NXC_LAW_NODES : (thermal ? NXC_LAW_THERMAL : NXC_LAW_PLAIN);
    if (map2d) {
        P.map_dlon = (d->map_lon1 - d->map_lon0) / (double)(d->map_nlon - 1);
        P.map_ds = (d->map_s1 - d->map_s0) / (double)(d->map_nlat - 1);
    }
    // the queue order's bound on the launch speed (a set made of pieces may mix sources: there the
    // device finds its largest launch speed)
    const auto peak = [](const double *v, size_t count) {
        double big = 0.0;
        for (size_t k = 0; k < count; k++) big = std::max(big, std::fabs(v[k]));
        return big;
    };
    const double vmax = (n_sp ? peak(d->speed_v, n_sp)
                         : thermal ? P.coef_max      // |S| <= max |coef|: the bases are >= 0 and sum to 1
                         : node_speed ? peak(d->node_speed_v, n_nv)
                         : std::fabs(d->vprob) + (d->speed_type == 0 ? 1 : 6) * std::fabs(d->vwidth)) / d->unit_km;
    if (d->dest_total <= 0) P.k2max = vmax * vmax;
    return P;
}
