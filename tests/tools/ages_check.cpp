// Stand-alone driver of the host-only side of the age cube (nexoclom_amd/csrc/nxc_ages_check.hpp,
// the subject AGES_OF_PIXELS): the enable's arguments -- good ones, one bad set per refusal, na one below and at the 2^31 record
// limit of add_record_pairs -- the apply's arguments, and the plan that cuts k_ages_apply to a
// workgroup's LDS: at 64 KiB and 160 KiB, for (planes, epochs) of (3, 1), (66, 1), (66, 1000) and
// the most planes that still fit one pixel; every planned chunk must fit, and the chunks must
// cover every epoch exactly once.  Nothing is allocated on a device.  Build and run on the CPU:
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/ages_check.cpp -o ages_check && ./ages_check
// Prints one line per case; exit status 0 when every case went as expected.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_ages_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

void verdict(const char *name, const std::string &why, const char *text)
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

void expect(const char *name, int64_t n_pix, int64_t na, double t0, double a_lo, double a_hi,
            const char *text)
{
    verdict(name, check_ages_args(AGES_OF_PIXELS, n_pix, na, t0, a_lo, a_hi), text);
}

// the largest number of planes whose one pixel and one epoch fit lds bytes, by the plan's own sizes
int64_t most_planes(size_t lds)
{
    int64_t planes = 3;
    while (ages_plan_bytes(planes + 1, (planes + 1) | 1, 1, 1) <= lds) planes++;
    return planes;
}

void plan_case(size_t lds, int64_t planes, int64_t ne, bool fits)
{
    AgesPlan p;
    const bool got = ages_apply_plan(planes, ne, lds, &p);
    if (!fits) {
        std::printf("plan lds %zu planes %lld ne %lld: %s\n", lds, (long long)planes, (long long)ne,
                    got ? "planned -- UNEXPECTED" : "does not fit");
        if (got) unexpected++;
        return;
    }
    bool ok = got && p.run >= 1 && p.run <= NXC_AGES_APPLY_BLOCK && p.chunk >= 1 &&
              p.chunk <= ne && p.stride >= planes && (p.stride & 1) == 1 &&
              p.bytes == ages_plan_bytes(planes, p.stride, p.run, p.chunk) && p.bytes <= lds;
    // the chunks [c chunk, min(ne, (c + 1) chunk)) cover every epoch exactly once
    if (ok) {
        std::vector<int> seen((size_t)ne, 0);
        const int64_t chunks = (ne + p.chunk - 1) / p.chunk;
        for (int64_t c = 0; c < chunks; c++) {
            const int64_t e0 = c * p.chunk, ce = std::min(p.chunk, ne - e0);
            ok = ok && ce >= 1 && ages_plan_bytes(planes, p.stride, p.run, ce) <= lds;
            for (int64_t e = e0; e < e0 + ce; e++) seen[(size_t)e]++;
        }
        for (int64_t e = 0; e < ne; e++) ok = ok && seen[(size_t)e] == 1;
    }
    std::printf("plan lds %zu planes %lld ne %lld: stride %lld run %lld chunk %lld bytes %zu%s\n",
                lds, (long long)planes, (long long)ne, (long long)p.stride, (long long)p.run,
                (long long)p.chunk, p.bytes, ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    expect("64 bins on 512 x 512", 512 * 512, 64, 50000.0, 0.0, 1920.0, nullptr);
    expect("one bin on one pixel", 1, 1, 0.0, 0.0, 1e-300, nullptr);
    expect("negative a_lo", 12, 7, 3600.0, -15.0, 195.0, nullptr);
    expect("widest finite range", 12, 7, 0.0, -8e307, 8e307, nullptr);

    expect("na = 0", 12, 0, 1.0, 0.0, 1.0, "na must be at least 1");
    expect("na negative", 12, -3, 1.0, 0.0, 1.0, "na must be at least 1");
    expect("no pixels", 0, 4, 1.0, 0.0, 1.0, "no pixels");
    expect("t0 NaN", 12, 4, NaN, 0.0, 1.0, "t0 must be finite");
    expect("t0 inf", 12, 4, INF, 0.0, 1.0, "t0 must be finite");
    expect("a_lo NaN", 12, 4, 1.0, NaN, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi NaN", 12, 4, 1.0, 0.0, NaN, "a_lo and a_hi must be finite");
    expect("a_lo -inf", 12, 4, 1.0, -INF, 1.0, "a_lo and a_hi must be finite");
    expect("a_hi inf", 12, 4, 1.0, 0.0, INF, "a_lo and a_hi must be finite");
    expect("empty range", 12, 4, 1.0, 1.0, 1.0, "below a_hi");
    expect("reversed range", 12, 4, 1.0, 1.0, -1.0, "below a_hi");
    expect("width overflows", 12, 4, 1.0, -1.7e308, 1.7e308, "a_hi - a_lo");

    // n_pix * (na + 2) one below the limit, at it, and far past it
    expect("1 pixel, 2^31 - 1 records", 1, LIMIT - 3, 1.0, 0.0, 1.0, nullptr);
    expect("1 pixel, 2^31 records", 1, LIMIT - 2, 1.0, 0.0, 1.0, "2^31");
    expect("1 pixel, na = 2^31", 1, LIMIT, 1.0, 0.0, 1.0, "2^31");
    expect("2^16 pixels, 2^31 - 2^16 records", 65536, 32765, 1.0, 0.0, 1.0, nullptr);
    expect("2^16 pixels, 2^31 records", 65536, 32766, 1.0, 0.0, 1.0, "2^31");
    expect("3 pixels, 2147483646 records", 3, 715827880, 1.0, 0.0, 1.0, nullptr);
    expect("3 pixels, 2147483649 records", 3, 715827881, 1.0, 0.0, 1.0, "2^31");
    expect("na = INT64_MAX", 12, std::numeric_limits<int64_t>::max(), 1.0, 0.0, 1.0, "2^31");

    const double inv = ages_inv_da(64, 0.0, 1920.0);
    const bool inv_ok = inv == 64.0 / 1920.0;
    std::printf("inv_da %.17g%s\n", inv, inv_ok ? "" : " -- UNEXPECTED");
    if (!inv_ok) unexpected++;

    // the apply's arguments
    const double good[6] = {1.0, 0.0, -2.5, 0.5, 1e300, -0.0};
    double bad[6] = {1.0, 0.0, -2.5, 0.5, 1e300, 0.0};
    verdict("K 3 x 2", check_ages_apply(3, 2, good), nullptr);
    verdict("K 6 x 1", check_ages_apply(6, 1, good), nullptr);
    verdict("ne = 0", check_ages_apply(3, 0, good), "ne must be at least 1");
    verdict("ne negative", check_ages_apply(3, -2, good), "ne must be at least 1");
    verdict("ne = 2^31", check_ages_apply(3, LIMIT, good), "below 2^31");
    verdict("K null", check_ages_apply(3, 2, nullptr), "K is null");
    bad[5] = NaN;
    verdict("K with a NaN at its end", check_ages_apply(3, 2, bad), "not finite");
    bad[5] = 0.0; bad[0] = INF;
    verdict("K with an inf at its start", check_ages_apply(3, 2, bad), "not finite");
    bad[0] = 1.0; bad[3] = -INF;
    verdict("K with -inf inside", check_ages_apply(3, 2, bad), "not finite");

    // the plan
    for (const size_t lds : {size_t(64) * 1024, size_t(160) * 1024}) {
        plan_case(lds, 3, 1, true);
        plan_case(lds, 66, 1, true);
        plan_case(lds, 66, 1000, true);
        plan_case(lds, 9, 65, true);
        const int64_t most = most_planes(lds);
        plan_case(lds, most, 1, true);
        plan_case(lds, most, 1000, true);
        plan_case(lds, most + 1, 1, false);
    }
    plan_case(0, 3, 1, false);
    plan_case(64 * 1024, 3, 0, false);

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
