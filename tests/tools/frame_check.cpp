// Stand-alone driver of the host-only checks of the moon-centred frame
// (nexoclom_amd/csrc/nxc_frame_check.hpp): good descriptions, row ranges and columns, then one bad
// one per refusal.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/frame_check.cpp -o frame_check && ./frame_check
// Prints one line per case; exit status 0 when every good case was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_frame_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
const int64_t BIG = std::numeric_limits<int64_t>::max();
int unexpected = 0;

void report(const char *name, const std::string &why, const char *text)
{
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

// Io around Jupiter, lengths in Jupiter radii
nxc_frame_desc io()
{
    nxc_frame_desc d{};
    d.omega = 4.11e-5;
    d.M[0] = -4.96; d.M[1] = 3.19; d.M[2] = 0.0;
    d.U[0] = -1.31e-4; d.U[1] = -2.04e-4; d.U[2] = 0.0;
    d.scale = 39.2;
    return d;
}

void desc(const char *name, const nxc_frame_desc &d, const char *text) { report(name, check_frame_desc(&d), text); }

void range(const char *name, int64_t total, int64_t first, int64_t count, const char *text)
{
    report(name, check_frame_range(total, first, count), text);
}

}  // namespace

int main()
{
    desc("Io", io(), nullptr);
    nxc_frame_desc d{};
    d.scale = 1.0;
    desc("identity", d, nullptr);
    d = io(); d.omega = -d.omega;
    desc("retrograde", d, nullptr);
    d = io(); d.scale = 5e-324;
    desc("smallest scale", d, nullptr);

    report("null description", check_frame_desc(nullptr), "description is null");
    d = io(); d.omega = NaN;       desc("omega NaN", d, "omega must be finite");
    d = io(); d.omega = INF;       desc("omega inf", d, "omega must be finite");
    for (int k = 0; k < 3; k++) {
        d = io(); d.M[k] = k == 1 ? -INF : NaN;  desc("M not finite", d, "M must be finite");
        d = io(); d.U[k] = k == 1 ? INF : NaN;   desc("U not finite", d, "U must be finite");
    }
    d = io(); d.scale = NaN;       desc("scale NaN", d, "scale must be finite");
    d = io(); d.scale = INF;       desc("scale inf", d, "scale must be finite");
    d = io(); d.scale = 0.0;       desc("scale 0", d, "scale must be above 0");
    d = io(); d.scale = -0.0;      desc("scale -0", d, "scale must be above 0");
    d = io(); d.scale = -39.2;     desc("scale negative", d, "scale must be above 0");

    range("whole store", 250, 0, 250, nullptr);
    range("a slice", 250, 97, 97, nullptr);
    range("no rows at the end", 250, 250, 0, nullptr);
    range("empty store", 0, 0, 0, nullptr);
    range("largest store", BIG, BIG - 1, 1, nullptr);
    range("first negative", 250, -1, 10, "first lies outside");
    range("first past the end", 250, 251, 0, "first lies outside");
    range("count negative", 250, 0, -1, "count reaches outside");
    range("count past the end", 250, 97, 154, "count reaches outside");
    range("first + count overflows", 250, 2, BIG, "count reaches outside");
    range("first of an empty store", 0, 1, 0, "first lies outside");

    double col[4] = {0, 0, 0, 0};
    const void *good[8] = {col, col, col, col, col, col, col, col};
    report("4 rows", check_frame_columns(4, good), nullptr);
    const void *none[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    report("no rows, no columns", check_frame_columns(0, none), nullptr);
    for (int c = 0; c < 8; c++) {
        const void *bad[8] = {col, col, col, col, col, col, col, col};
        bad[c] = nullptr;
        report("a null column", check_frame_columns(4, bad), "column is null");
    }
    report("p negative", check_frame_columns(-1, good), "must not be negative");

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
