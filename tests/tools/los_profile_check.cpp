// Stand-alone driver of the host-only check of a line-of-sight profile's arguments
// (nexoclom_amd/csrc/nxc_los_profile_check.hpp): good arguments, then one bad set per refusal, and
// nv one below and at the 2^31 record limit for several numbers of spectra -- nothing is allocated,
// so the limit is cheap to reach.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/los_profile_check.cpp -o los_profile_check && ./los_profile_check
// Prints one line per case; exit status 0 when every good set was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_los_profile_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void expect(const char *name, int64_t S, int64_t nv, double v_lo, double v_hi, const char *text)
{
    const std::string why = check_los_profile_args(S, nv, v_lo, v_hi);
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    const bool ok = why.rfind("line-of-sight profile: ", 0) == 0 && why.find(text) != std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(),
                ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    expect("64 bins for 512 spectra", 512, 64, -4e-3, 4e-3, nullptr);
    expect("one bin for one spectrum", 1, 1, 0.0, 1e-300, nullptr);
    expect("widest finite range", 12, 7, -8e307, 8e307, nullptr);

    expect("no spectra", 0, 4, -1.0, 1.0, "S must be at least 1");
    expect("S negative", -5, 4, -1.0, 1.0, "S must be at least 1");
    expect("nv = 0", 12, 0, -1.0, 1.0, "nv must be at least 1");
    expect("nv negative", 12, -3, -1.0, 1.0, "nv must be at least 1");
    expect("v_lo NaN", 12, 4, NaN, 1.0, "finite");
    expect("v_hi NaN", 12, 4, -1.0, NaN, "finite");
    expect("v_lo -inf", 12, 4, -INF, 1.0, "finite");
    expect("v_hi inf", 12, 4, -1.0, INF, "finite");
    expect("empty range", 12, 4, 1.0, 1.0, "below v_hi");
    expect("reversed range", 12, 4, 1.0, -1.0, "below v_hi");
    expect("width overflows", 12, 4, -1.7e308, 1.7e308, "v_hi - v_lo");

    // S * (nv + 2) one below the limit, at it, and far past it
    expect("1 spectrum, 2^31 - 1 records", 1, LIMIT - 3, -1.0, 1.0, nullptr);
    expect("1 spectrum, 2^31 records", 1, LIMIT - 2, -1.0, 1.0, "2^31");
    expect("1 spectrum, nv = 2^31", 1, LIMIT, -1.0, 1.0, "2^31");
    expect("2^16 spectra, 2^31 - 2^16 records", 65536, 32765, -1.0, 1.0, nullptr);
    expect("2^16 spectra, 2^31 records", 65536, 32766, -1.0, 1.0, "2^31");
    expect("3 spectra, 2147483646 records", 3, 715827880, -1.0, 1.0, nullptr);
    expect("3 spectra, 2147483649 records", 3, 715827881, -1.0, 1.0, "2^31");
    expect("2^31 - 1 spectra, no room for 3 records each", LIMIT - 1, 1, -1.0, 1.0, "2^31");
    expect("S = INT64_MAX", std::numeric_limits<int64_t>::max(), 1, -1.0, 1.0, "2^31");
    expect("nv = INT64_MAX", 12, std::numeric_limits<int64_t>::max(), -1.0, 1.0, "2^31");

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
