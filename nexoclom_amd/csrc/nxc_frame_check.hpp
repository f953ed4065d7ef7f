// Host-only side of nxc_frame_rows / nxc_frame_columns[_f32]: what a moon-centred frame and the
// rows it is to move must satisfy before anything is allocated or launched (include/
// nexoclom_hip.h, "Moon-centred frame").  Plain C++ without a device call or a handle: a refusal
// is a text, which nxc_api.hip hands to fail().  So it can also be built into a stand-alone
// program and run under the host sanitizers (tests/tools/frame_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/nexoclom_hip.h"

// "" or why the description is refused
inline std::string check_frame_desc(const nxc_frame_desc *d)
{
    if (!d) return "nxc_frame_desc: the description is null";
    if (!std::isfinite(d->omega)) return "nxc_frame_desc: omega must be finite";
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(d->M[k])) return "nxc_frame_desc: M must be finite";
        if (!std::isfinite(d->U[k])) return "nxc_frame_desc: U must be finite";
    }
    if (!std::isfinite(d->scale)) return "nxc_frame_desc: scale must be finite";
    if (!(d->scale > 0.0)) return "nxc_frame_desc: scale must be above 0";
    return "";
}

// "" or why rows [first, first + count) are refused of a store of `total` rows (the sum is not
// formed: it may not fit)
inline std::string check_frame_range(int64_t total, int64_t first, int64_t count)
{
    if (first < 0 || first > total) return "frame rows: first lies outside the store";
    if (count < 0 || count > total - first) return "frame rows: count reaches outside the store";
    return "";
}

// "" or why p rows of host columns are refused; cols: t, x, y, z, vx, vy, vz, then out
inline std::string check_frame_columns(int64_t p, const void *const cols[8])
{
    if (p < 0) return "frame columns: p must not be negative";
    if (p == 0) return "";
    for (int c = 0; c < 8; c++)
        if (!cols[c]) return "frame columns: a column is null with p > 0";
    return "";
}
