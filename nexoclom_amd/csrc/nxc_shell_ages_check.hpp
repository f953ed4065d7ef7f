// Host-only side of nxc_shell_ages_enable: what the shell map's ages must satisfy before anything is
// allocated or freed (include/nexoclom_hip.h, "ShellMap ages").  The rules and the limit are the age
// cube's (nxc_ages_check.hpp: check_ages_args, NXC_AGES_MAX_RECORDS, ages_inv_da) with the map's
// R = nlon * nlat * (nalt + 2) records in place of the pixels.  Plain C++ without a device call or a
// handle: a refusal is a text, which nxc_api.hip hands to fail().  So it can also be built into a
// stand-alone program and run under the host sanitizers (tests/tools/shell_ages_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "nxc_ages_check.hpp"

constexpr int64_t NXC_SHELL_AGE_PLANES = 2;         // age plane A {w, w w}, age plane B {c, c c}

// "" or why the enable refuses na >= 1 age bins over [a_lo, a_hi) at the epoch t0 for a map of
// n_records records per plane
inline std::string check_shell_ages_args(int64_t n_records, int64_t na, double t0, double a_lo,
                                         double a_hi)
{
    if (n_records < 1) return "shell ages: the map has no records";
    const std::string why = check_ages_args(n_records, na, t0, a_lo, a_hi);
    if (why.empty()) return why;
    // the cube's own words, about records
    const std::string cube = "age cube: ", pixels = "n_pix * (na + 2)";
    std::string text = why.substr(cube.size());
    const size_t at = text.find(pixels);
    if (at != std::string::npos) text.replace(at, pixels.size(), "nlon * nlat * (nalt + 2) * (na + 2)");
    return "shell ages: " + text;
}

// bytes of the two age planes of a map of n_records records with na bins; the arguments are ones
// check_shell_ages_args accepted, so n_records * (na + 2) < 2^31 and the bytes stay below 2^36
inline size_t shell_ages_bytes(int64_t n_records, int64_t na)
{
    return (size_t)NXC_SHELL_AGE_PLANES * (size_t)n_records * (size_t)(na + 2) * 2 * sizeof(double);
}
