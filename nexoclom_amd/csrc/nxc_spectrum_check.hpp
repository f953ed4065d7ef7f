// Host-only side of nxc_density_spectrum_enable: what a density spectrum must satisfy before
// anything is freed or allocated (include/nexoclom_hip.h, "Density spectrum").  Plain C++ without a
// device call or a handle: a refusal is a text, which nxc_api.hip hands to fail().  So it can also
// be built into a stand-alone program and run under the host sanitizers
// (tests/tools/spectrum_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

// add_record_pairs takes the record index as an int: n_points * (nv + 2) records must stay below this
constexpr int64_t NXC_SPECTRUM_MAX_RECORDS = int64_t(1) << 31;
// how far the length of a boresight may be from 1
constexpr double NXC_SPECTRUM_UNIT_TOL = 1e-12;

// "" or why the enable refuses nv >= 1 speed bins over [s_lo, s_hi) for an aperture of half angle
// acos(cos_half) (ignored with all_sky) at the n_points >= 0 points of the index, given the frame
// records frames[n_frames][8] = {ux uy uz 0 bx by bz 0} (may be null when there are none)
inline std::string check_spectrum_args(int64_t n_points, int64_t n_frames, int64_t nv, double s_lo,
                                       double s_hi, double cos_half, int all_sky, const double *frames)
{
    if (n_points < 0) return "density spectrum: a negative number of points";
    if (n_frames != n_points)
        return "density spectrum: " + std::to_string(n_frames) + " frame records for the " +
               std::to_string(n_points) + " points of the index";
    if (nv < 1) return "density spectrum: nv must be at least 1";
    if (!std::isfinite(s_lo) || !std::isfinite(s_hi)) return "density spectrum: s_lo and s_hi must be finite";
    if (!(s_lo >= 0.0)) return "density spectrum: s_lo must not be negative (a speed)";
    if (!(s_lo < s_hi)) return "density spectrum: s_lo must be below s_hi";
    if (!std::isfinite(s_hi - s_lo)) return "density spectrum: s_hi - s_lo must be finite";
    if (!std::isfinite(cos_half) || cos_half < -1.0 || cos_half > 1.0)
        return "density spectrum: cos_half must lie in [-1, 1]";
    // n_points * (nv + 2) < 2^31 without forming the product: nv + 2 <= floor((2^31 - 1) / n_points)
    if (nv >= NXC_SPECTRUM_MAX_RECORDS ||
        (n_points > 0 && nv + 2 > (NXC_SPECTRUM_MAX_RECORDS - 1) / n_points))
        return "density spectrum: n_points * (nv + 2) must be below 2^31 records";
    if (n_points > 0 && !frames) return "density spectrum: no frame records";
    for (int64_t q = 0; q < n_points; q++) {
        const double *f = frames + 8 * q;
        for (int c = 0; c < 8; c++)
            if (!std::isfinite(f[c])) return "density spectrum: a frame value is not finite";
        if (all_sky) continue;
        const double b2 = (f[4] * f[4] + f[5] * f[5]) + f[6] * f[6];
        if (!(std::fabs(std::sqrt(b2) - 1.0) <= NXC_SPECTRUM_UNIT_TOL))
            return "density spectrum: a boresight is not of unit length";
    }
    return "";
}

// bins per unit of speed, formed once in fp64 on the host
inline double spectrum_inv_ds(int64_t nv, double s_lo, double s_hi) { return (double)nv / (s_hi - s_lo); }
