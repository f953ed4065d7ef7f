// Stand-alone driver of the host-only check of the density ages' arguments
// (nexoclom_amd/csrc/nxc_ages_check.hpp, the subject AGES_OF_POINTS): good arguments, then one bad set per refusal, and
// na one below and at the 2^31 record limit for several numbers of points -- nothing is allocated,
// so the limit is cheap to reach.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/density_ages_check.cpp -o density_ages_check && ./density_ages_check
// Prints one line per case; exit status 0 when every good set was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_ages_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void expect(const char *name, int64_t Q, int64_t na, double t0, double a_lo, double a_hi, const char *text)
{
    const std::string why = check_ages_args(AGES_OF_POINTS, Q, na, t0, a_lo, a_hi);
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    // the messages speak of points: neither the cube nor its pixels are named
    const bool ok = why.rfind("density ages: ", 0) == 0 && why.find(text) != std::string::npos &&
                    why.find("age cube") == std::string::npos && why.find("n_pix") == std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(),
                ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    expect("16 bins on a 128^3 grid", 128 * 128 * 128, 16, 3600.0, 0.0, 3600.0, nullptr);
    expect("one bin at one point", 1, 1, 0.0, 0.0, 1e-300, nullptr);
    expect("negative ages, negative epoch", 12, 7, -5.0, -100.0, -1.0, nullptr);
    expect("widest finite range", 12, 7, 1.7e308, -8e307, 8e307, nullptr);
    expect("inv_da of 8 bins of 30 s", 1, 8, 0.0, 60.0, 300.0,
           ages_inv_da(8, 60.0, 300.0) == 1.0 / 30.0 ? nullptr : "never");

    expect("no points", 0, 4, 10.0, 0.0, 1.0, "the index has no points");
    expect("n_points negative", -5, 4, 10.0, 0.0, 1.0, "the index has no points");
    expect("na = 0", 12, 0, 10.0, 0.0, 1.0, "na must be at least 1");
    expect("na negative", 12, -3, 10.0, 0.0, 1.0, "na must be at least 1");
    expect("t0 NaN", 12, 4, NaN, 0.0, 1.0, "t0 must be finite");
    expect("t0 inf", 12, 4, INF, 0.0, 1.0, "t0 must be finite");
    expect("t0 -inf", 12, 4, -INF, 0.0, 1.0, "t0 must be finite");
    expect("a_lo NaN", 12, 4, 10.0, NaN, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi NaN", 12, 4, 10.0, 0.0, NaN, "a_lo and a_hi must be finite");
    expect("a_lo -inf", 12, 4, 10.0, -INF, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi inf", 12, 4, 10.0, 0.0, INF, "a_lo and a_hi must be finite");
    expect("empty range", 12, 4, 10.0, 1.0, 1.0, "below a_hi");
    expect("reversed range", 12, 4, 10.0, 1.0, -1.0, "below a_hi");
    expect("width overflows", 12, 4, 10.0, -1.7e308, 1.7e308, "a_hi - a_lo");

    // n_points * (na + 2) one below the limit, at it, and far past it
    expect("1 point, 2^31 - 1 records", 1, LIMIT - 3, 10.0, 0.0, 1.0, nullptr);
    expect("1 point, 2^31 records", 1, LIMIT - 2, 10.0, 0.0, 1.0,
           "n_points * (na + 2) must be below 2^31");
    expect("1 point, na = 2^31", 1, LIMIT, 10.0, 0.0, 1.0, "2^31");
    expect("2^16 points, 2^31 - 2^16 records", 65536, 32765, 10.0, 0.0, 1.0, nullptr);
    expect("2^16 points, 2^31 records", 65536, 32766, 10.0, 0.0, 1.0, "2^31");
    expect("3 points, 2147483646 records", 3, 715827880, 10.0, 0.0, 1.0, nullptr);
    expect("3 points, 2147483649 records", 3, 715827881, 10.0, 0.0, 1.0, "2^31");
    expect("2^31 - 1 points, no room for 3 records each", LIMIT - 1, 1, 10.0, 0.0, 1.0, "2^31");
    expect("n_points = INT64_MAX", std::numeric_limits<int64_t>::max(), 1, 10.0, 0.0, 1.0, "2^31");
    expect("na = INT64_MAX", 12, std::numeric_limits<int64_t>::max(), 10.0, 0.0, 1.0, "2^31");

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
