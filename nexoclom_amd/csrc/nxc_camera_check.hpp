// Host-only side of nxc_camera_desc (nxc_camera_set): what a camera must satisfy before anything
// goes to the device.  Plain C++ without a device call or a handle: a refusal is a text, which
// nxc_api.hip hands to fail().  So it can also be built into a stand-alone program and run under
// the host sanitizers (tests/tools/camera_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/nexoclom_hip.h"

constexpr int64_t NXC_CAMERA_MAX_DIM = 8192;
constexpr double NXC_CAMERA_ORTHO_TOL = 1e-12;

// nx + 1 tangent-plane edges: finite, increasing, e[k] = -e[n - k] (to 1e-12 of the half width)
inline std::string check_camera_edges(const char *name, const double *e, int64_t n)
{
    for (int64_t k = 0; k <= n; k++)
        if (!std::isfinite(e[k])) return std::string("nxc_camera_desc: ") + name + " must be finite";
    for (int64_t k = 0; k < n; k++)
        if (!(e[k + 1] > e[k])) return std::string("nxc_camera_desc: ") + name + " must increase";
    for (int64_t k = 0; k <= n - k; k++)
        if (!(std::fabs(e[k] + e[n - k]) <= 1e-12 * e[n]))
            return std::string("nxc_camera_desc: ") + name + " must be symmetric about 0";
    return "";
}

// "" or why nxc_camera_set refuses the description
inline std::string check_camera_desc(const nxc_camera_desc *d)
{
    if (!d) return "nxc_camera_desc: null description";
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(d->o[a])) return "nxc_camera_desc: the observer position must be finite";
    const double o2 = (d->o[0] * d->o[0] + d->o[1] * d->o[1]) + d->o[2] * d->o[2];
    if (!(o2 >= 1.0) || !std::isfinite(o2))
        return "nxc_camera_desc: the observer must be on or outside the unit sphere (|o| >= 1)";
    for (int i = 0; i < 3; i++)
        for (int j = i; j < 3; j++) {
            double dot = 0.0;
            for (int a = 0; a < 3; a++) dot += d->C[3 * i + a] * d->C[3 * j + a];
            if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= NXC_CAMERA_ORTHO_TOL))
                return "nxc_camera_desc: C must be orthonormal (rows right, boresight, up) to 1e-12";
        }
    if (!std::isfinite(d->vrplanet)) return "nxc_camera_desc: vrplanet must be finite";
    if (!(d->pix_area_cm2 > 0.0) || !std::isfinite(d->pix_area_cm2))
        return "nxc_camera_desc: pix_area_cm2 must be positive and finite";
    if (d->quantity != 0 && d->quantity != 1) return "nxc_camera_desc: quantity must be 0 or 1";
    if (d->nx < 1 || d->nz < 1 || d->nx > NXC_CAMERA_MAX_DIM || d->nz > NXC_CAMERA_MAX_DIM)
        return "nxc_camera_desc: dims must be 1..8192";
    if (!d->uedges || !d->vedges) return "nxc_camera_desc: null edges";
    std::string why = check_camera_edges("uedges", d->uedges, d->nx);
    if (why.empty()) why = check_camera_edges("vedges", d->vedges, d->nz);
    if (!why.empty()) return why;
    if (d->n_lines < 0 || d->n_lines > NXC_MAX_LINES)
        return "nxc_camera_desc: n_lines out of range";
    if (d->quantity == 1)
        for (int l = 0; l < d->n_lines; l++)
            if (!d->line_v[l] || !d->line_g[l] || d->line_n[l] < 2)
                return "nxc_camera_desc: a g-value table is null or shorter than 2";
    return "";
}
