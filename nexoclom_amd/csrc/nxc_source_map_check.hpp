// Host-only side of nxc_source_map_desc (nxc_source_map_set): what a source-map grid must satisfy
// before anything goes to the device (include/nexoclom_hip.h, "Source maps"), and the dynamic LDS
// of the two kernels that stage it.  Plain C++ without a device call or a handle: a refusal is a
// text, which nxc_api.hip hands to fail().  So it can also be built into a stand-alone program and
// run under the host sanitizers (tests/tools/source_map_check.cpp).
//
// Both LDS requests are fixed by the descriptor: k_smap_points' by tile, bins and the longest
// segment list, k_smap_prep's by bins and grid alone (the speed edges come per Output, their
// count does not).  nxc_source_map_set refuses a grid whose either request passes the bound, so
// nxc_source_map_accumulate never launches with more.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/nexoclom_hip.h"

// what a launch may ask for without a function attribute
constexpr size_t NXC_SMAP_LDS_BYTES = 64 * 1024;
constexpr int64_t NXC_SMAP_MAX_POINTS = int64_t(1) << 24;
constexpr int64_t NXC_SMAP_MAX_BINS = int64_t(1) << 16;

// doubles per grid point: [nvel speed | nalt altitude | naz azimuth | n_total | n_included | weight]
inline int64_t smap_stride_of(int64_t nvel, int64_t nalt, int64_t naz) { return nvel + nalt + naz + 3; }

// edges k_smap_prep stages: speed, altitude, azimuth, longitude, latitude (n + 1 each)
inline size_t smap_edge_count(int64_t nvel, int64_t nalt, int64_t naz, int64_t nlon, int64_t nlat)
{
    return (size_t)(nvel + nalt + naz + nlon + nlat + 5);
}

// LDS of k_smap_prep: the edges, then the whole-planet histograms [nvel | nalt | naz]
inline size_t smap_prep_lds_bytes(int64_t nvel, int64_t nalt, int64_t naz, int64_t nlon, int64_t nlat)
{
    return 8 * (smap_edge_count(nvel, nalt, naz, nlon, nlat) + (size_t)(nvel + nalt + naz));
}

// LDS of k_smap_points: the tile's map [tile][stride] doubles, then the segment starts and their
// exclusive prefix lengths (nseg_max + 1 ints each)
inline size_t smap_points_lds_bytes(int64_t tile, int64_t nvel, int64_t nalt, int64_t naz, int64_t nseg_max)
{
    return (size_t)8 * (size_t)tile * (size_t)smap_stride_of(nvel, nalt, naz) + (size_t)4 * 2 * (size_t)(nseg_max + 1);
}

inline bool smap_linspace_ok(const double *e, int64_t n)
{
    if (!e || n < 1) return false;
    for (int64_t k = 0; k <= n; k++)
        if (!std::isfinite(e[k]) || (k && !(e[k] >= e[k - 1]))) return false;
    return e[n] > e[0];
}

// "" or why both kernels' LDS is refused
inline std::string check_source_map_lds(int64_t nlon, int64_t nlat, int64_t nvel, int64_t nalt, int64_t naz,
                                        int64_t tile, int64_t nseg_max)
{
    const size_t points = smap_points_lds_bytes(tile, nvel, nalt, naz, nseg_max);
    if (points > NXC_SMAP_LDS_BYTES)
        return "nxc_source_map_desc: a tile's histograms and segment table need " + std::to_string(points) +
               " bytes, more than the 64 KiB of LDS a launch may ask for";
    const size_t prep = smap_prep_lds_bytes(nvel, nalt, naz, nlon, nlat);
    if (prep > NXC_SMAP_LDS_BYTES)
        return "nxc_source_map_desc: the edges and whole-planet histograms need " + std::to_string(prep) +
               " bytes, more than the 64 KiB of LDS a launch may ask for (fewer bins or a coarser grid)";
    return "";
}

// "" or why nxc_source_map_set refuses the description; *nseg_max: the longest segment list of a tile
inline std::string check_source_map_desc(const nxc_source_map_desc *d, int64_t *nseg_max)
{
    if (nseg_max) *nseg_max = 0;
    if (!d) return "null argument";
    const int64_t nlon = d->nlon, nlat = d->nlat;
    if (nlon < 1 || nlat < 1 || d->nvel < 1 || d->nalt < 1 || d->naz < 1 || nlon > NXC_SMAP_MAX_POINTS ||
        nlat > NXC_SMAP_MAX_POINTS || nlon * nlat > NXC_SMAP_MAX_POINTS || d->nvel > NXC_SMAP_MAX_BINS ||
        d->nalt > NXC_SMAP_MAX_BINS || d->naz > NXC_SMAP_MAX_BINS ||
        d->nvel + d->nalt + d->naz > NXC_SMAP_MAX_BINS || d->tile < 1 || d->tile > nlon || !(d->r_km > 0.0) ||
        !std::isfinite(d->r_km))
        return "bad nxc_source_map_desc grid";
    if (!smap_linspace_ok(d->alt_edges, d->nalt) || !smap_linspace_ok(d->az_edges, d->naz) ||
        !smap_linspace_ok(d->lon_edges, nlon) || !smap_linspace_ok(d->lat_edges, nlat))
        return "nxc_source_map_desc: edges must be finite and increasing";
    if (!d->point_lon || !d->point_lat || !d->point_cos || !d->threshold || !d->seg_off || (d->n_seg && !d->seg))
        return "nxc_source_map_desc: null table";
    const int64_t tpr = (nlon + d->tile - 1) / d->tile, ntiles = tpr * nlat, ncells = nlon * nlat;
    // every segment is a run of existing cells, and the tiles' lists tile the segment array
    if (d->n_seg < 0 || d->n_seg > INT32_MAX || d->seg_off[0] != 0 || d->seg_off[ntiles] != d->n_seg)
        return "nxc_source_map_desc: segment offsets do not span the segments";
    int64_t longest = 0;
    for (int64_t t = 0; t < ntiles; t++) {
        const int64_t c = (int64_t)d->seg_off[t + 1] - d->seg_off[t];
        if (c < 0) return "nxc_source_map_desc: segment offsets are not sorted";
        if (c > longest) longest = c;
    }
    for (int64_t s = 0; s < d->n_seg; s++)
        if (d->seg[2 * s] < 0 || d->seg[2 * s] > d->seg[2 * s + 1] || d->seg[2 * s + 1] >= ncells)
            return "nxc_source_map_desc: segment outside the grid";
    if (nseg_max) *nseg_max = longest;
    return check_source_map_lds(nlon, nlat, d->nvel, d->nalt, d->naz, d->tile, longest);
}
