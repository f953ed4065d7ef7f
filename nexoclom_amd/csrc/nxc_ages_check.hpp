// Host-only side of the age blocks (include/nexoclom_hip.h, "Age cube", "Density ages",
// "Line-of-sight ages", "ShellMap ages"): what nxc_*_ages_enable and nxc_*_ages_apply must find
// before anything is allocated or freed, the size of a block, and how nxc_*_ages_apply cuts its work
// to the LDS of a workgroup.  One check serves the four subjects; what differs between them is the
// words of the refusal (AgesSubject).  Plain C++ without a device call or a handle: a refusal is a
// text, which nxc_api.hip hands to fail().  So it can also be built into stand-alone programs and
// run under the host sanitizers (tests/tools/ages_check.cpp, density_ages_check.cpp,
// los_ages_check.cpp, shell_ages_check.cpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

// add_record_pairs takes the record index as an int: records * (na + 2) must stay below this
constexpr int64_t NXC_AGES_MAX_RECORDS = int64_t(1) << 31;

constexpr int NXC_SHELL_AGE_PLANES = 2;             // age plane A {w, w w}, age plane B {c, c c}

// What is given ages, in the words of its refusals
struct AgesSubject {
    const char *label;      // what every refusal starts with
    const char *empty;      // the sentence for a subject without a record
    const char *records;    // how the number of 16-byte records of one set is spelled
};
constexpr AgesSubject AGES_OF_PIXELS = {"age cube", "the image has no pixels", "n_pix * (na + 2)"};
constexpr AgesSubject AGES_OF_POINTS = {"density ages", "the index has no points",
                                        "n_points * (na + 2)"};
constexpr AgesSubject AGES_OF_SPECTRA = {"line-of-sight ages", "S must be at least 1", "S * (na + 2)"};
constexpr AgesSubject AGES_OF_SHELLS = {"shell ages", "the map has no records",
                                        "nlon * nlat * (nalt + 2) * (na + 2)"};

// "" or why the enable refuses na >= 1 age bins over [a_lo, a_hi) at the epoch t0 for a subject of
// n >= 1 records (pixels, points, spectra, records of the shell map) per set
inline std::string check_ages_args(const AgesSubject &who, int64_t n, int64_t na, double t0,
                                   double a_lo, double a_hi)
{
    const std::string label = std::string(who.label) + ": ";
    if (n < 1) return label + who.empty;
    if (na < 1) return label + "na must be at least 1";
    if (!std::isfinite(t0)) return label + "t0 must be finite";
    if (!std::isfinite(a_lo) || !std::isfinite(a_hi)) return label + "a_lo and a_hi must be finite";
    if (!(a_lo < a_hi)) return label + "a_lo must be below a_hi";
    if (!std::isfinite(a_hi - a_lo)) return label + "a_hi - a_lo must be finite";
    // n * (na + 2) < 2^31 without forming the product: na + 2 <= floor((2^31 - 1) / n)
    if (na >= NXC_AGES_MAX_RECORDS || na + 2 > (NXC_AGES_MAX_RECORDS - 1) / n)
        return label + who.records + " must be below 2^31 records";
    return "";
}

// bytes of `sets` sets (NXC_SHELL_AGE_PLANES for the shell map, 1 elsewhere) of records * (na + 2)
// records {sum, sum of squares}; the arguments are ones check_ages_args accepted, so the records of
// a set stay below 2^31 and the bytes below 2^36
inline size_t ages_block_bytes(int sets, int64_t records, int64_t na)
{
    return (size_t)sets * (size_t)records * (size_t)(na + 2) * 2 * sizeof(double);
}

// bins per second of age, formed once in fp64 on the host
inline double ages_inv_da(int64_t na, double a_lo, double a_hi) { return (double)na / (a_hi - a_lo); }

// "" or why nxc_*_ages_apply refuses the response matrix K[planes][ne]
inline std::string check_ages_apply(int64_t planes, int64_t ne, const double *K)
{
    if (ne < 1) return "age cube: ne must be at least 1";
    if (ne >= NXC_AGES_MAX_RECORDS) return "age cube: ne must be below 2^31";
    if (!K) return "age cube: K is null";
    for (int64_t j = 0; j < planes * ne; j++)
        if (!std::isfinite(K[j])) return "age cube: K holds a value that is not finite";
    return "";
}

// ---- the plan of k_ages_apply ---------------------------------------------------------------------
// A workgroup keeps `run` consecutive pixels' records, [run][stride] 16-byte records, and the
// `chunk` epochs' columns of K, [planes][chunk] doubles, in LDS.  stride is planes made odd: threads
// of consecutive pixels then read records an odd number of 16-byte words apart, which spreads them
// over the banks.  The plan aims at NXC_AGES_LDS_TARGET bytes, so that several workgroups share a
// CU, and goes to all of lds_bytes only where one epoch and one pixel need it.
constexpr int NXC_AGES_APPLY_BLOCK = 256;
constexpr int64_t NXC_AGES_MAX_CHUNK = 64;                 // epochs per chunk
constexpr size_t NXC_AGES_LDS_TARGET = 32 * 1024;
constexpr int64_t NXC_AGES_MAX_CHUNKS = 65535;             // the launch grid's second dimension

struct AgesPlan {
    int64_t stride = 0;      // 16-byte records from one pixel to the next in LDS
    int64_t run = 0;         // pixels per workgroup
    int64_t chunk = 0;       // epochs per workgroup; ceil(ne / chunk) chunks cover them
    size_t bytes = 0;        // the LDS of one workgroup
};

inline size_t ages_plan_bytes(int64_t planes, int64_t stride, int64_t run, int64_t chunk)
{
    return (size_t)run * (size_t)stride * 16 + (size_t)planes * (size_t)chunk * 8;
}

// false: not even one epoch and one pixel fit lds_bytes
inline bool ages_apply_plan(int64_t planes, int64_t ne, size_t lds_bytes, AgesPlan *plan)
{
    AgesPlan p;
    if (planes < 3 || ne < 1 || planes >= NXC_AGES_MAX_RECORDS) return false;
    p.stride = planes | 1;
    if (ages_plan_bytes(planes, p.stride, 1, 1) > lds_bytes) return false;
    const size_t budget = std::min(lds_bytes, std::max(NXC_AGES_LDS_TARGET,
                                                       ages_plan_bytes(planes, p.stride, 1, 1)));
    // K's chunk takes at most half of what the first pixel leaves
    const size_t for_k = (budget - (size_t)p.stride * 16) / 2;
    p.chunk = std::max<int64_t>(1, std::min<int64_t>({ne, NXC_AGES_MAX_CHUNK,
                                                      (int64_t)(for_k / ((size_t)planes * 8))}));
    const size_t left = budget - (size_t)planes * (size_t)p.chunk * 8;
    p.run = std::max<int64_t>(1, std::min<int64_t>(NXC_AGES_APPLY_BLOCK,
                                                   (int64_t)(left / ((size_t)p.stride * 16))));
    p.bytes = ages_plan_bytes(planes, p.stride, p.run, p.chunk);
    *plan = p;
    return p.bytes <= lds_bytes;
}
