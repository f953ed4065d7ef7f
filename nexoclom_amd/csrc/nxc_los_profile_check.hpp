// Host-only side of nxc_los_profile_enable: what a line-of-sight profile must satisfy before
// anything is allocated or freed (include/nexoclom_hip.h, "Line-of-sight profile").  The limits are
// the velocity cube's (nxc_cube_check.hpp: NXC_CUBE_MAX_RECORDS, cube_inv_dv) with the S spectra in
// place of the pixels.  Plain C++ without a device call or a handle: a refusal is a text, which
// nxc_api.hip hands to fail().  So it can also be built into a stand-alone program and run under
// the host sanitizers (tests/tools/los_profile_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "nxc_cube_check.hpp"

// "" or why the enable refuses nv >= 1 bins over [v_lo, v_hi) for S spectra
inline std::string check_los_profile_args(int64_t S, int64_t nv, double v_lo, double v_hi)
{
    if (S < 1) return "line-of-sight profile: S must be at least 1";
    if (nv < 1) return "line-of-sight profile: nv must be at least 1";
    if (!std::isfinite(v_lo) || !std::isfinite(v_hi))
        return "line-of-sight profile: v_lo and v_hi must be finite";
    if (!(v_lo < v_hi)) return "line-of-sight profile: v_lo must be below v_hi";
    if (!std::isfinite(v_hi - v_lo)) return "line-of-sight profile: v_hi - v_lo must be finite";
    // S * (nv + 2) < 2^31 without forming the product: nv + 2 <= floor((2^31 - 1) / S)
    if (nv >= NXC_CUBE_MAX_RECORDS || nv + 2 > (NXC_CUBE_MAX_RECORDS - 1) / S)
        return "line-of-sight profile: S * (nv + 2) must be below 2^31 records";
    return "";
}
