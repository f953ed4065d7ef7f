// Host-only side of nxc_shell_moments_enable / _accumulate* / _download: what the shell map's
// state and the size of its planes must satisfy before anything is allocated, launched or copied
// (include/nexoclom_hip.h, "ShellMap moments").  Plain C++ without a device call or a handle: the
// state travels as a small struct and a refusal is a code and a text, which nxc_api.hip hands to
// fail().  So it can also be built into a stand-alone program and run under the host sanitizers
// (tests/tools/shell_moments_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "nxc_shell_check.hpp"

constexpr int64_t NXC_SHELL_MOMENT_PLANES = 6;      // planes of 16-byte records, twelve sums
// the six planes are one allocation addressed from its start in doubles.  A plane holds fewer than
// 2^31 records (the record index is an int), so the six hold fewer than 6 * 2^32 doubles: offsets
// and bytes (below 2^38) stay far inside an int64_t and a size_t, and what the device cannot hold
// is refused by the allocation (NXC_ERR_NOMEM)

// what the entries know of the handle
struct ShellMomentsState {
    bool handle;            // the handle is not null
    bool have_shell;        // nxc_shell_set has been called
    bool enabled;           // nxc_shell_moments_enable(h, 1) since the last nxc_shell_set
    int64_t plane;          // doubles of one plane of records (ShellK::plane): cells (nalt + 2) 2
};

struct ShellMomentsRefusal {
    int code;               // NXC_OK or the entry's return value
    const char *why;
};

constexpr const char *NXC_SHELL_UNSET = "nxc_shell_set has not been called";
constexpr const char *NXC_SHELL_MOMENTS_UNSET = "nxc_shell_moments_enable has not been called: moments not enabled";

// bytes of the six planes; 0 when the plane size cannot be addressed
inline size_t shell_moments_bytes(int64_t plane)
{
    if (plane < 2 || (plane & 1)) return 0;
    if (plane / 2 >= NXC_SHELL_MAX_RECORDS) return 0;                 // the record index is an int
    return (size_t)plane * (size_t)NXC_SHELL_MOMENT_PLANES * sizeof(double);
}

// nxc_shell_moments_enable: the set first, then the size of the planes
inline ShellMomentsRefusal check_shell_moments_enable(const ShellMomentsState &s)
{
    if (!s.handle || !s.have_shell) return {NXC_ERR_STATE, NXC_SHELL_UNSET};
    if (shell_moments_bytes(s.plane) == 0)
        return {NXC_ERR_ARG, "shell moments: a plane must hold 1 .. 2^31 - 1 whole records"};
    return {NXC_OK, ""};
}

// nxc_shell_moments_accumulate*: the set is named first, then the enable
inline ShellMomentsRefusal check_shell_moments_ready(const ShellMomentsState &s)
{
    if (!s.handle || !s.have_shell) return {NXC_ERR_STATE, NXC_SHELL_UNSET};
    if (!s.enabled) return {NXC_ERR_STATE, NXC_SHELL_MOMENTS_UNSET};
    return {NXC_OK, ""};
}

// nxc_shell_moments_download: the same, then its output
inline ShellMomentsRefusal check_shell_moments_download(const ShellMomentsState &s, const void *sums)
{
    const ShellMomentsRefusal r = check_shell_moments_ready(s);
    if (r.code != NXC_OK) return r;
    if (!sums) return {NXC_ERR_ARG, "bad arguments"};
    if (shell_moments_bytes(s.plane) == 0)
        return {NXC_ERR_ARG, "shell moments: a plane must hold 1 .. 2^31 - 1 whole records"};
    return {NXC_OK, ""};
}
