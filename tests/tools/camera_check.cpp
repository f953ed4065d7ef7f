// Stand-alone driver of the host-only check of a camera description
// (nexoclom_amd/csrc/nxc_camera_check.hpp): one good descriptor, then one bad one per refusal, each
// with tables exactly as long as the descriptor says, so that a sanitizer sees every byte the check
// reads.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/camera_check.cpp -o camera_check && ./camera_check
// Prints one line per case; exit status 0 when the good descriptor was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_camera_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
constexpr int NX = 5, NZ = 3, NG = 4;

struct Tables {
    std::vector<double> u, v, gv, gg;
};

std::vector<double> edges(int n, double half)
{
    std::vector<double> e(n + 1);
    for (int k = 0; k <= n; k++) e[k] = -half + 2.0 * half * k / n;
    e[n] = half;
    return e;
}

Tables good_tables()
{
    Tables t;
    t.u = edges(NX, 0.5);
    t.v = edges(NZ, 0.25);
    t.gv = {-3.0, -1.0, 1.0, 3.0};
    t.gg = {1.0, 2.0, 2.0, 1.0};
    return t;
}

nxc_camera_desc good_desc(const Tables &t)
{
    nxc_camera_desc d;
    std::memset(&d, 0, sizeof d);
    d.o[0] = 0.0; d.o[1] = -3.0; d.o[2] = 0.0;
    const double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(d.C, C, sizeof C);
    d.vrplanet = 1e-3;
    d.pix_area_cm2 = 2.5e15;
    d.quantity = 1;
    d.n_lines = 2;
    d.nx = NX; d.nz = NZ;
    d.uedges = t.u.data(); d.vedges = t.v.data();
    for (int l = 0; l < 2; l++) {
        d.line_n[l] = NG; d.line_v[l] = t.gv.data(); d.line_g[l] = t.gg.data();
    }
    return d;
}

int unexpected = 0;

void expect(const char *name, const nxc_camera_desc *d, const char *text)
{
    const std::string why = check_camera_desc(d);
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    const bool ok = !why.empty() && why.find(text) != std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(),
                ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

}  // namespace

int main()
{
    const Tables t = good_tables();
    nxc_camera_desc d = good_desc(t);
    expect("good camera", &d, nullptr);
    d.quantity = 0; d.n_lines = 0;
    for (int l = 0; l < NXC_MAX_LINES; l++) { d.line_v[l] = nullptr; d.line_g[l] = nullptr; d.line_n[l] = 0; }
    expect("column camera without tables", &d, nullptr);
    expect("null description", nullptr, "null description");

    d = good_desc(t); d.o[1] = NaN;
    expect("observer NaN", &d, "observer position must be finite");
    d = good_desc(t); d.o[0] = INF;
    expect("observer infinite", &d, "observer position must be finite");
    d = good_desc(t); d.o[1] = -0.5;
    expect("observer inside the planet", &d, "|o| >= 1");
    d = good_desc(t); d.C[0] = 1.0 + 1e-9;
    expect("basis row not unit", &d, "orthonormal");
    d = good_desc(t); d.C[1] = 1e-9;
    expect("basis rows not orthogonal", &d, "orthonormal");
    d = good_desc(t); d.C[4] = NaN;
    expect("basis NaN", &d, "orthonormal");
    d = good_desc(t); d.vrplanet = NaN;
    expect("vrplanet NaN", &d, "vrplanet");
    d = good_desc(t); d.pix_area_cm2 = 0.0;
    expect("pixel area zero", &d, "pix_area_cm2");
    d = good_desc(t); d.quantity = 2;
    expect("quantity 2", &d, "quantity");
    d = good_desc(t); d.nx = 0;
    expect("nx = 0", &d, "dims");
    d = good_desc(t); d.nz = 8193;
    expect("nz = 8193", &d, "dims");
    d = good_desc(t); d.uedges = nullptr;
    expect("null uedges", &d, "null edges");
    {
        Tables b = good_tables(); b.u[2] = NaN;
        d = good_desc(b);
        expect("uedges NaN", &d, "uedges must be finite");
    }
    {
        Tables b = good_tables(); b.v[1] = b.v[2];
        d = good_desc(b);
        expect("vedges not increasing", &d, "vedges must increase");
    }
    {
        Tables b = good_tables();
        for (double &e : b.u) e += 0.1;
        d = good_desc(b);
        expect("uedges not symmetric", &d, "uedges must be symmetric");
    }
    {
        Tables b = good_tables(); b.v[1] += 0.01;
        d = good_desc(b);
        expect("vedges inner edge not symmetric", &d, "vedges must be symmetric");
    }
    d = good_desc(t); d.n_lines = NXC_MAX_LINES + 1;
    expect("n_lines too large", &d, "n_lines");
    d = good_desc(t); d.n_lines = -1;
    expect("n_lines negative", &d, "n_lines");
    d = good_desc(t); d.line_g[1] = nullptr;
    expect("null g table", &d, "g-value table");
    d = good_desc(t); d.line_n[0] = 1;
    expect("g table of one point", &d, "g-value table");

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
