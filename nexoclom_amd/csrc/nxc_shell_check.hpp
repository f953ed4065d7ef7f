// Host-only side of nxc_shell_desc (nxc_shell_set): what a shell map must satisfy before anything
// goes to the device (include/nexoclom_hip.h, "ShellMap").  Plain C++ without a device call or a
// handle: a refusal is a text, which nxc_api.hip hands to fail().  So it can also be built into a
// stand-alone program and run under the host sanitizers (tests/tools/shell_check.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/nexoclom_hip.h"

constexpr int64_t NXC_SHELL_MAX_DIM = 8192;
// add_record_pairs takes the record index as an int: nlon * nlat * (nalt + 2) must stay below this
constexpr int64_t NXC_SHELL_MAX_RECORDS = int64_t(1) << 31;
constexpr size_t NXC_SHELL_LDS_BYTES = 160 * 1024;
constexpr double NXC_SHELL_TWO_PI = 0x1.921fb54442d18p+2;     // the double nearest 2 pi (2*np.pi)

// n + 1 edges from `first` to `last` exactly (np.linspace gives both ends as they are), finite and
// increasing
inline std::string check_shell_edges(const char *name, const double *e, int64_t n, double first,
                                     double last)
{
    for (int64_t k = 0; k <= n; k++)
        if (!std::isfinite(e[k])) return std::string("nxc_shell_desc: ") + name + " must be finite";
    for (int64_t k = 0; k < n; k++)
        if (!(e[k + 1] > e[k])) return std::string("nxc_shell_desc: ") + name + " must increase";
    if (e[0] != first || e[n] != last)
        return std::string("nxc_shell_desc: ") + name + " must span its whole axis (lon_edges 0 to "
               "2 pi, mu_edges -1 to 1)";
    return "";
}

// "" or why the grid is refused: dims, altitude range, record count (without forming the product)
inline std::string check_shell_grid(int64_t nlon, int64_t nlat, int64_t nalt, double r_lo, double r_hi)
{
    if (nlon < 1 || nlat < 1 || nlon > NXC_SHELL_MAX_DIM || nlat > NXC_SHELL_MAX_DIM)
        return "nxc_shell_desc: nlon and nlat must be 1..8192";
    if (nalt < 1) return "nxc_shell_desc: nalt must be at least 1";
    if (!std::isfinite(r_lo) || !std::isfinite(r_hi))
        return "nxc_shell_desc: r_lo and r_hi must be finite";
    if (!(r_lo >= 1.0)) return "nxc_shell_desc: r_lo must be at least 1 (the surface)";
    if (!(r_lo < r_hi)) return "nxc_shell_desc: r_lo must be below r_hi";
    // cells * (nalt + 2) < 2^31: nalt + 2 <= floor((2^31 - 1) / cells), cells <= 2^26
    const int64_t cells = nlon * nlat;
    if (nalt >= NXC_SHELL_MAX_RECORDS || nalt + 2 > (NXC_SHELL_MAX_RECORDS - 1) / cells)
        return "nxc_shell_desc: nlon * nlat * (nalt + 2) must be below 2^31 records";
    return "";
}

// "" or why nxc_shell_set refuses the description
inline std::string check_shell_desc(const nxc_shell_desc *d)
{
    if (!d) return "nxc_shell_desc: null description";
    std::string why = check_shell_grid(d->nlon, d->nlat, d->nalt, d->r_lo, d->r_hi);
    if (!why.empty()) return why;
    if (!std::isfinite(d->vrplanet)) return "nxc_shell_desc: vrplanet must be finite";
    if (d->quantity != 0 && d->quantity != 1) return "nxc_shell_desc: quantity must be 0 or 1";
    if (!d->lon_edges || !d->mu_edges) return "nxc_shell_desc: null edges";
    why = check_shell_edges("lon_edges", d->lon_edges, d->nlon, 0.0, NXC_SHELL_TWO_PI);
    if (why.empty()) why = check_shell_edges("mu_edges", d->mu_edges, d->nlat, -1.0, 1.0);
    if (!why.empty()) return why;
    if (d->n_lines < 0 || d->n_lines > NXC_MAX_LINES) return "nxc_shell_desc: n_lines out of range";
    if (d->quantity == 1)
        for (int l = 0; l < d->n_lines; l++)
            if (!d->line_v[l] || !d->line_g[l] || d->line_n[l] < 2)
                return "nxc_shell_desc: a g-value table is null or shorter than 2";
    return "";
}

// "" or why a blob of `bytes` [header | g tables | lon edges | mu edges] is refused
inline std::string check_shell_blob(size_t bytes)
{
    if (bytes > NXC_SHELL_LDS_BYTES)
        return "nxc_shell_desc: tables and edges exceed the 160 KiB LDS of a gfx950 CU";
    return "";
}

// altitude bins per planet radius, formed once in fp64 on the host
inline double shell_inv_dr(int64_t nalt, double r_lo, double r_hi) { return (double)nalt / (r_hi - r_lo); }

// Copies of the {c sum, count} pair per cell that k_shell's workgroups spread their adds over
// (workgroup b adds to copy b % replicas; nxc_shell_download sums them): every binned sample adds to
// that array, and on a few thousand records the adds queue up behind one another at the memory side
// ("ShellMap").  Enough copies for 2^18 records, the 512 x 512 image's, at
// which k_image_moments reaches the atomic request rate; never more than 1024.
constexpr int64_t NXC_SHELL_SPREAD_RECORDS = int64_t(1) << 18;
constexpr int64_t NXC_SHELL_MAX_REPLICAS = 1024;
inline int64_t shell_replicas(int64_t cells)
{
    const int64_t want = (NXC_SHELL_SPREAD_RECORDS + cells - 1) / cells;
    return want < 1 ? 1 : (want > NXC_SHELL_MAX_REPLICAS ? NXC_SHELL_MAX_REPLICAS : want);
}

// doubles of one plane of records, [cells][nalt + 2][2]
inline size_t shell_plane_doubles(int64_t nlon, int64_t nlat, int64_t nalt)
{
    return (size_t)nlon * (size_t)nlat * (size_t)(nalt + 2) * 2;
}
