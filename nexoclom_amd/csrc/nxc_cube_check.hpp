// Host-only side of nxc_image_cube_enable / nxc_camera_cube_enable: what a velocity cube must
// satisfy before anything is allocated (include/nexoclom_hip.h, "Velocity cube").  Plain C++ without
// a device call or a handle: a refusal is a text, which nxc_api.hip hands to fail().  So it can also
// be built into a stand-alone program and run under the host sanitizers
// (tests/tools/cube_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

// add_record_pairs takes the record index as an int: n_pix * (nv + 2) records must stay below this
constexpr int64_t NXC_CUBE_MAX_RECORDS = int64_t(1) << 31;

// "" or why the enable refuses nv >= 1 bins over [v_lo, v_hi) on an image of n_pix >= 1 pixels
inline std::string check_cube_args(int64_t n_pix, int64_t nv, double v_lo, double v_hi)
{
    if (n_pix < 1) return "velocity cube: the image has no pixels";
    if (nv < 1) return "velocity cube: nv must be at least 1";
    if (!std::isfinite(v_lo) || !std::isfinite(v_hi)) return "velocity cube: v_lo and v_hi must be finite";
    if (!(v_lo < v_hi)) return "velocity cube: v_lo must be below v_hi";
    if (!std::isfinite(v_hi - v_lo)) return "velocity cube: v_hi - v_lo must be finite";
    // n_pix * (nv + 2) < 2^31 without forming the product: nv + 2 <= floor((2^31 - 1) / n_pix)
    if (nv >= NXC_CUBE_MAX_RECORDS || nv + 2 > (NXC_CUBE_MAX_RECORDS - 1) / n_pix)
        return "velocity cube: n_pix * (nv + 2) must be below 2^31 records";
    return "";
}

// bins per unit of velocity, formed once in fp64 on the host
inline double cube_inv_dv(int64_t nv, double v_lo, double v_hi) { return (double)nv / (v_hi - v_lo); }
