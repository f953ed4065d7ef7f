// Stand-alone driver of the host-only check of a density spectrum's arguments
// (nexoclom_amd/csrc/nxc_spectrum_check.hpp): good arguments, then one bad set per refusal, and nv
// one below and at the 2^31 record limit of add_record_pairs -- with few points, so that the frame
// records the check reads stay small.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/spectrum_check.cpp -o spectrum_check && ./spectrum_check
// Prints one line per case; exit status 0 when every good set was accepted and every bad one
// refused with the expected text.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../nexoclom_amd/csrc/nxc_spectrum_check.hpp"

namespace {

const double NaN = std::numeric_limits<double>::quiet_NaN(), INF = std::numeric_limits<double>::infinity();
int unexpected = 0;

// Q frame records with the velocity u = (2e-4, -1e-4, 0) and the boresight b = (0.6, 0, 0.8)
std::vector<double> frames_for(int64_t Q)
{
    std::vector<double> f((size_t)Q * 8, 0.0);
    for (int64_t q = 0; q < Q; q++) {
        f[8 * q] = 2e-4; f[8 * q + 1] = -1e-4;
        f[8 * q + 4] = 0.6; f[8 * q + 6] = 0.8;
    }
    return f;
}

void expect(const char *name, int64_t Q, int64_t nv, double s_lo, double s_hi, double cos_half,
            int all_sky, const double *frames, const char *text)
{
    const std::string why = check_spectrum_args(Q, Q, nv, s_lo, s_hi, cos_half, all_sky, frames);
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
    const std::vector<double> twelve = frames_for(12), three = frames_for(3), one = frames_for(1);
    const double *f = twelve.data();
    expect("32 bins at 12 points", 12, 32, 0.0, 4e-3, 0.5, 0, f, nullptr);
    expect("one bin at one point", 1, 1, 0.0, 1e-300, 1.0, 0, one.data(), nullptr);
    expect("no points, no frames", 0, 8, 0.0, 1.0, 0.0, 0, nullptr, nullptr);
    expect("widest finite range", 12, 7, 0.0, 1.7e308, -1.0, 0, f, nullptr);
    expect("cos_half = -1", 12, 4, 1.0, 2.0, -1.0, 0, f, nullptr);

    expect("nv = 0", 12, 0, 0.0, 1.0, 0.5, 0, f, "nv must be at least 1");
    expect("nv negative", 12, -3, 0.0, 1.0, 0.5, 0, f, "nv must be at least 1");
    expect("negative point count", -1, 4, 0.0, 1.0, 0.5, 0, f, "negative number of points");
    expect("s_lo NaN", 12, 4, NaN, 1.0, 0.5, 0, f, "finite");
    expect("s_hi NaN", 12, 4, 0.0, NaN, 0.5, 0, f, "finite");
    expect("s_hi inf", 12, 4, 0.0, INF, 0.5, 0, f, "finite");
    expect("s_lo -inf", 12, 4, -INF, 1.0, 0.5, 0, f, "finite");
    expect("s_lo negative", 12, 4, -1e-9, 1.0, 0.5, 0, f, "must not be negative");
    expect("empty range", 12, 4, 1.0, 1.0, 0.5, 0, f, "below s_hi");
    expect("reversed range", 12, 4, 2.0, 1.0, 0.5, 0, f, "below s_hi");
    expect("cos_half NaN", 12, 4, 0.0, 1.0, NaN, 0, f, "cos_half");
    expect("cos_half above 1", 12, 4, 0.0, 1.0, 1.0000001, 0, f, "cos_half");
    expect("cos_half below -1", 12, 4, 0.0, 1.0, -1.0000001, 0, f, "cos_half");
    expect("cos_half NaN, all sky", 12, 4, 0.0, 1.0, NaN, 1, f, "cos_half");
    expect("null frames", 12, 4, 0.0, 1.0, 0.5, 0, nullptr, "no frame records");
    {   // the frame records must be the index's: as many as it has points, or no frame is read
        const char *text = "frame records for the";
        for (int64_t n : {int64_t(0), int64_t(11), int64_t(13), int64_t(-1)}) {
            const std::string why = check_spectrum_args(12, n, 4, 0.0, 1.0, 0.5, 0, n > 0 ? f : nullptr);
            const bool ok = why.find(text) != std::string::npos;
            std::printf("%lld frames for 12 points refused: %s%s\n", (long long)n,
                        why.empty() ? "(accepted)" : why.c_str(), ok ? "" : " -- UNEXPECTED");
            if (!ok) unexpected++;
        }
    }

    // one bad value in the last record: a velocity, a padding word, a boresight
    for (int c : {0, 3, 5, 7}) {
        std::vector<double> bad = twelve;
        bad[8 * 11 + c] = c == 5 ? INF : NaN;
        char name[64];
        std::snprintf(name, sizeof name, "frame value %d not finite", c);
        expect(name, 12, 4, 0.0, 1.0, 0.5, 0, bad.data(), "not finite");
        expect(name, 12, 4, 0.0, 1.0, 0.5, 1, bad.data(), "not finite");
    }
    {   // |b| one part in 10^11 off, then within 1e-12; a zero boresight passes only with all_sky
        std::vector<double> off = twelve, close = twelve, zero = twelve;
        off[8 * 5 + 4] = 0.6 * (1.0 + 1e-11); off[8 * 5 + 6] = 0.8 * (1.0 + 1e-11);
        close[8 * 5 + 4] = 0.6 * (1.0 + 5e-13); close[8 * 5 + 6] = 0.8 * (1.0 + 5e-13);
        zero[8 * 5 + 4] = 0.0; zero[8 * 5 + 6] = 0.0;
        expect("boresight 1e-11 too long", 12, 4, 0.0, 1.0, 0.5, 0, off.data(), "unit length");
        expect("boresight 1e-11 too long, all sky", 12, 4, 0.0, 1.0, 0.5, 1, off.data(), nullptr);
        expect("boresight 5e-13 too long", 12, 4, 0.0, 1.0, 0.5, 0, close.data(), nullptr);
        expect("zero boresight", 12, 4, 0.0, 1.0, 0.5, 0, zero.data(), "unit length");
        expect("zero boresight, all sky", 12, 4, 0.0, 1.0, 0.5, 1, zero.data(), nullptr);
    }

    // Q * (nv + 2) one below the limit, at it, and far past it
    expect("1 point, 2^31 - 1 records", 1, LIMIT - 3, 0.0, 1.0, 0.5, 0, one.data(), nullptr);
    expect("1 point, 2^31 records", 1, LIMIT - 2, 0.0, 1.0, 0.5, 0, one.data(), "2^31");
    expect("1 point, nv = 2^31", 1, LIMIT, 0.0, 1.0, 0.5, 0, one.data(), "2^31");
    expect("3 points, 2147483646 records", 3, 715827880, 0.0, 1.0, 0.5, 0, three.data(), nullptr);
    expect("3 points, 2147483649 records", 3, 715827881, 0.0, 1.0, 0.5, 0, three.data(), "2^31");
    expect("nv = INT64_MAX", 12, std::numeric_limits<int64_t>::max(), 0.0, 1.0, 0.5, 0, f, "2^31");
    {   // the limit is refused before a frame is read: 2^16 points with frames of one
        expect("2^16 points, 2^31 records", 65536, 32766, 0.0, 1.0, 0.5, 0, one.data(), "2^31");
        const std::vector<double> many = frames_for(65536);
        expect("2^16 points, 2^31 - 2^16 records", 65536, 32765, 0.0, 1.0, 0.5, 0, many.data(), nullptr);
    }

    const double inv = spectrum_inv_ds(32, 1e-4, 4e-3);
    const bool inv_ok = inv == 32.0 / (4e-3 - 1e-4);
    std::printf("inv_ds %.17g%s\n", inv, inv_ok ? "" : " -- UNEXPECTED");
    if (!inv_ok) unexpected++;

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
