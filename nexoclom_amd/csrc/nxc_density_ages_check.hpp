// Host-only side of nxc_density_ages_enable: what the density ages must satisfy before anything is
// allocated or freed (include/nexoclom_hip.h, "Density ages").  The rules and the limit are the age
// cube's (nxc_ages_check.hpp: check_ages_args, NXC_AGES_MAX_RECORDS, ages_inv_da) with the indexed
// points in place of the pixels.  Plain C++ without a device call or a handle: a refusal is a text,
// which nxc_api.hip hands to fail().  So it can also be built into a stand-alone program and run
// under the host sanitizers (tests/tools/density_ages_check.cpp).
#pragma once

#include <cstdint>
#include <string>

#include "nxc_ages_check.hpp"

// "" or why the enable refuses na >= 1 age bins over [a_lo, a_hi) at the epoch t0 for n_points
// indexed points
inline std::string check_density_ages_args(int64_t n_points, int64_t na, double t0, double a_lo,
                                           double a_hi)
{
    if (n_points < 1) return "density ages: the index has no points";
    const std::string why = check_ages_args(n_points, na, t0, a_lo, a_hi);
    if (why.empty()) return why;
    // the cube's own words, about points
    const std::string cube = "age cube: ", pixels = "n_pix * (na + 2)";
    std::string text = why.substr(cube.size());
    const size_t at = text.find(pixels);
    if (at != std::string::npos) text.replace(at, pixels.size(), "n_points * (na + 2)");
    return "density ages: " + text;
}
