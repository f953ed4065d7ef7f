// Host-only side of nxc_los_ages_enable: what the line-of-sight ages must satisfy before anything
// is allocated or freed (include/nexoclom_hip.h, "Line-of-sight ages").  The rules and the limit are
// the age cube's (nxc_ages_check.hpp: check_ages_args, NXC_AGES_MAX_RECORDS, ages_inv_da) with the S
// spectra in place of the pixels.  Plain C++ without a device call or a handle: a refusal is a text,
// which nxc_api.hip hands to fail().  So it can also be built into a stand-alone program and run
// under the host sanitizers (tests/tools/los_ages_check.cpp).
#pragma once

#include <cstdint>
#include <string>

#include "nxc_ages_check.hpp"

// "" or why the enable refuses na >= 1 age bins over [a_lo, a_hi) at the epoch t0 for S spectra
inline std::string check_los_ages_args(int64_t S, int64_t na, double t0, double a_lo, double a_hi)
{
    if (S < 1) return "line-of-sight ages: S must be at least 1";
    const std::string why = check_ages_args(S, na, t0, a_lo, a_hi);
    if (why.empty()) return why;
    // the cube's own words, about spectra
    const std::string cube = "age cube: ", pixels = "n_pix * (na + 2)";
    std::string text = why.substr(cube.size());
    const size_t at = text.find(pixels);
    if (at != std::string::npos) text.replace(at, pixels.size(), "S * (na + 2)");
    return "line-of-sight ages: " + text;
}
