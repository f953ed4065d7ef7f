// Host-only part of nxc_packets_sample for the per-node tables of a surface map (speed_type 4,
// angular_type 2): what the descriptor must satisfy before anything is launched, and where the
// tables go in the handle's source buffer.  Plain C++ without a device call, so that it can also
// be built into a stand-alone program and run under the host sanitizers
// (tests/tools/node_tables_check.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/nexoclom_hip.h"

constexpr int64_t NXC_NODE_TABLE_MAX = 1 << 16;       // entries per row

struct NodeTableCopy {
    size_t at;                 // offset in the source buffer, in doubles
    const double *from;
    size_t count;
};

// Where the tables go, behind `base` doubles of other tables: speed cdf, speed axis, altitude
// cdf, altitude axis, azimuth cdf, azimuth axis.  Unused tables have count 0.
struct NodeTableLayout {
    NodeTableCopy copy[6];
    size_t total;              // doubles, all six
};

inline NodeTableLayout node_table_layout(const nxc_source_desc *d, size_t base)
{
    NodeTableLayout L{};
    const size_t nodes = (size_t)(d->map_nlon * d->map_nlat);
    const bool speed = d->speed_type == 4, angles = d->angular_type == 2;
    const size_t n[3] = {speed ? (size_t)d->n_node_speed : 0, angles ? (size_t)d->n_node_alt : 0,
                         angles ? (size_t)d->n_node_az : 0};
    const double *cdf[3] = {d->node_speed_cdf, d->node_alt_cdf, d->node_az_cdf};
    const double *axis[3] = {d->node_speed_v, d->node_alt, d->node_az};
    size_t at = base;
    for (int t = 0; t < 3; t++) {
        L.copy[2 * t] = {at, cdf[t], nodes * n[t]};
        at += nodes * n[t];
        L.copy[2 * t + 1] = {at, axis[t], n[t]};
        at += n[t];
    }
    L.total = at - base;
    return L;
}

// One table: n entries per row, a finite axis, and per node a cdf that is non-decreasing from 0
// to 1 -- or all zeros where the node's value in the map is 0 (a node that is never drawn).
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

// "" when the descriptor's per-node tables can be launched from, else the reason.  The map itself
// (map, map_nlon, map_nlat of spatial_type 2) has been checked before.
inline std::string check_node_tables(const nxc_source_desc *d)
{
    const bool speed = d->speed_type == 4, angles = d->angular_type == 2;
    if (!speed && !angles) return "";
    if (d->spatial_type != 2)
        return "nxc_source_desc: per-node tables (speed_type 4, angular_type 2) need a 2-D surface "
               "map (spatial_type 2)";
    if (d->generator != 0)
        return "nxc_source_desc: per-node tables are drawn with generator 0 (Philox) only";
    // k_sample<NXC_LAW_NODES> holds no thermal code: speed_type 3 would fall through to the
    // tabulated branch and read the speed_cdf it does not have
    if (d->speed_type == 3)
        return "nxc_source_desc: thermal speeds (speed_type 3) with per-node directions "
               "(angular_type 2) are not implemented";
    const int64_t nodes = d->map_nlon * d->map_nlat;
    std::string why;
    if (speed) {
        why = check_node_table("node_speed", d->n_node_speed, d->node_speed_cdf, d->node_speed_v,
                               d->map, nodes);
        if (!why.empty()) return why;
    }
    if (angles) {
        why = check_node_table("node_alt", d->n_node_alt, d->node_alt_cdf, d->node_alt, d->map, nodes);
        if (!why.empty()) return why;
        why = check_node_table("node_az", d->n_node_az, d->node_az_cdf, d->node_az, d->map, nodes);
    }
    return why;
}
