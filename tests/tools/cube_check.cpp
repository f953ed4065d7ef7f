// Stand-alone driver of the host-only check of a velocity cube's arguments
// (nexoclom_amd/csrc/nxc_cube_check.hpp): good arguments, then one bad set per refusal, and nv one
// below and at the 2^31 record limit of add_record_pairs for several image sizes -- nothing is
// allocated, so the limit is cheap to reach.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/cube_check.cpp -o cube_check && ./cube_check
// Prints one line per case; exit status 0 when every good set was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_cube_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void expect(const char *name, int64_t n_pix, int64_t nv, double v_lo, double v_hi, const char *text)
{
    const std::string why = check_cube_args(n_pix, nv, v_lo, v_hi);
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
    const int64_t LIMIT = int64_t(1) << 31;
    expect("64 bins on 512 x 512", 512 * 512, 64, -4e-3, 4e-3, nullptr);
    expect("one bin on one pixel", 1, 1, 0.0, 1e-300, nullptr);
    expect("widest finite range", 12, 7, -8e307, 8e307, nullptr);

    expect("nv = 0", 12, 0, -1.0, 1.0, "nv must be at least 1");
    expect("nv negative", 12, -3, -1.0, 1.0, "nv must be at least 1");
    expect("no pixels", 0, 4, -1.0, 1.0, "no pixels");
    expect("v_lo NaN", 12, 4, NaN, 1.0, "finite");
    expect("v_hi NaN", 12, 4, -1.0, NaN, "finite");
    expect("v_lo -inf", 12, 4, -INF, 1.0, "finite");
    expect("v_hi inf", 12, 4, -1.0, INF, "finite");
    expect("empty range", 12, 4, 1.0, 1.0, "below v_hi");
    expect("reversed range", 12, 4, 1.0, -1.0, "below v_hi");
    expect("width overflows", 12, 4, -1.7e308, 1.7e308, "v_hi - v_lo");

    // n_pix * (nv + 2) one below the limit, at it, and far past it
    expect("1 pixel, 2^31 - 1 records", 1, LIMIT - 3, -1.0, 1.0, nullptr);
    expect("1 pixel, 2^31 records", 1, LIMIT - 2, -1.0, 1.0, "2^31");
    expect("1 pixel, nv = 2^31", 1, LIMIT, -1.0, 1.0, "2^31");
    expect("2^16 pixels, 2^31 - 2^16 records", 65536, 32765, -1.0, 1.0, nullptr);
    expect("2^16 pixels, 2^31 records", 65536, 32766, -1.0, 1.0, "2^31");
    expect("3 pixels, 2147483646 records", 3, 715827880, -1.0, 1.0, nullptr);
    expect("3 pixels, 2147483649 records", 3, 715827881, -1.0, 1.0, "2^31");
    expect("8192 x 8192 pixels, 30 bins", int64_t(8192) * 8192, 29, -1.0, 1.0, nullptr);
    expect("8192 x 8192 pixels, 2^31 records", int64_t(8192) * 8192, 30, -1.0, 1.0, "2^31");
    expect("nv = INT64_MAX", 12, std::numeric_limits<int64_t>::max(), -1.0, 1.0, "2^31");

    const double inv = cube_inv_dv(64, -4e-3, 4e-3);
    const bool inv_ok = inv == 64.0 / (4e-3 - -4e-3);
    std::printf("inv_dv %.17g%s\n", inv, inv_ok ? "" : " -- UNEXPECTED");
    if (!inv_ok) unexpected++;

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
