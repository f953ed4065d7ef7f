// Stand-alone driver of the host-only check of the shell ages' arguments
// (nexoclom_amd/csrc/nxc_ages_check.hpp, the subject AGES_OF_SHELLS): good arguments, then one bad set per refusal, and
// R * (na + 2) one below and at the 2^31 record limit for several record counts R -- nothing is
// allocated, so the limit is cheap to reach.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/shell_ages_check.cpp -o shell_ages_check && ./shell_ages_check
// Prints one line per case; exit status 0 when every good set was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_ages_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void expect(const char *name, int64_t R, int64_t na, double t0, double a_lo, double a_hi, const char *text)
{
    const std::string why = check_ages_args(AGES_OF_SHELLS, R, na, t0, a_lo, a_hi);
    if (!text) {
        std::printf("%s accepted%s\n", name, why.empty() ? "" : " -- UNEXPECTED refusal");
        if (!why.empty()) { std::printf("    %s\n", why.c_str()); unexpected++; }
        return;
    }
    // the messages speak of the map's records: neither the cube nor its pixels are named
    const bool ok = why.rfind("shell ages: ", 0) == 0 && why.find(text) != std::string::npos &&
                    why.find("age cube") == std::string::npos && why.find("n_pix") == std::string::npos;
    std::printf("%s refused: %s%s\n", name, why.empty() ? "(accepted)" : why.c_str(),
                ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

void expect_bytes(const char *name, int64_t R, int64_t na, size_t bytes)
{
    const size_t got = ages_block_bytes(NXC_SHELL_AGE_PLANES, R, na);
    std::printf("%s: %zu bytes%s\n", name, got, got == bytes ? " ok" : " -- UNEXPECTED");
    if (got != bytes) unexpected++;
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    const int64_t R = int64_t(72) * 36 * 34;                   // 72 x 36 x 32
    expect("32 bins on 72 x 36 x 32", R, 32, 3600.0, 0.0, 3600.0, nullptr);
    expect("one bin on 1 x 1 x 1", 3, 1, 0.0, 0.0, 1e-300, nullptr);
    expect("negative ages, negative epoch", R, 7, -5.0, -100.0, -1.0, nullptr);
    expect("widest finite range", R, 7, 1.7e308, -8e307, 8e307, nullptr);
    expect("inv_da of 8 bins of 30 s", R, 8, 600.0, 60.0, 300.0,
           ages_inv_da(8, 60.0, 300.0) == 1.0 / 30.0 ? nullptr : "never");

    expect("no records", 0, 4, 10.0, 0.0, 1.0, "the map has no records");
    expect("records negative", -5, 4, 10.0, 0.0, 1.0, "the map has no records");
    expect("na = 0", R, 0, 10.0, 0.0, 1.0, "na must be at least 1");
    expect("na negative", R, -3, 10.0, 0.0, 1.0, "na must be at least 1");
    expect("t0 NaN", R, 4, NaN, 0.0, 1.0, "t0 must be finite");
    expect("t0 inf", R, 4, INF, 0.0, 1.0, "t0 must be finite");
    expect("t0 -inf", R, 4, -INF, 0.0, 1.0, "t0 must be finite");
    expect("a_lo NaN", R, 4, 10.0, NaN, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi NaN", R, 4, 10.0, 0.0, NaN, "a_lo and a_hi must be finite");
    expect("a_lo -inf", R, 4, 10.0, -INF, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi inf", R, 4, 10.0, 0.0, INF, "a_lo and a_hi must be finite");
    expect("empty range", R, 4, 10.0, 1.0, 1.0, "below a_hi");
    expect("reversed range", R, 4, 10.0, 1.0, -1.0, "below a_hi");
    expect("width overflows", R, 4, 10.0, -1.7e308, 1.7e308, "a_hi - a_lo");

    // R * (na + 2) one below the limit, at it, and far past it
    expect("1 record, 2^31 - 1 age records", 1, LIMIT - 3, 10.0, 0.0, 1.0, nullptr);
    expect("1 record, 2^31 age records", 1, LIMIT - 2, 10.0, 0.0, 1.0,
           "nlon * nlat * (nalt + 2) * (na + 2) must be below 2^31");
    expect("1 record, na = 2^31", 1, LIMIT, 10.0, 0.0, 1.0, "2^31");
    expect("2^16 records, 2^31 - 2^16 age records", 65536, 32765, 10.0, 0.0, 1.0, nullptr);
    expect("2^16 records, 2^31 age records", 65536, 32766, 10.0, 0.0, 1.0, "2^31");
    expect("3 records, 2147483646 age records", 3, 715827880, 10.0, 0.0, 1.0, nullptr);
    expect("3 records, 2147483649 age records", 3, 715827881, 10.0, 0.0, 1.0, "2^31");
    expect("2^31 - 1 records, no room for 3 planes each", LIMIT - 1, 1, 10.0, 0.0, 1.0, "2^31");
    expect("records = INT64_MAX", std::numeric_limits<int64_t>::max(), 1, 10.0, 0.0, 1.0, "2^31");
    expect("na = INT64_MAX", R, std::numeric_limits<int64_t>::max(), 10.0, 0.0, 1.0, "2^31");

    expect_bytes("72 x 36 x 32, 32 bins", R, 32, (size_t)R * 34 * 32);
    expect_bytes("one record, one bin", 1, 1, 96);
    expect_bytes("2^31 - 1 age records", 1, LIMIT - 3, (size_t)(LIMIT - 1) * 32);

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
