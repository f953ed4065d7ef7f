// Stand-alone driver of the host-only checks of the shell moments' entries
// (nexoclom_amd/csrc/nxc_shell_moments_check.hpp): a good state per entry, then one bad one per
// refusal -- null handle, nxc_shell_set missing, moments not enabled, null output, and plane sizes
// one below, at and past what the record index and the allocation can address.  Nothing is
// allocated, so the limits are cheap to reach.  Build and run on the CPU, for instance
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//         tests/tools/shell_moments_check.cpp -o shell_moments_check && ./shell_moments_check
// Prints one line per case; exit status 0 when every good state was accepted and every bad one
// refused with the expected code and text.
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../nexoclom_amd/csrc/nxc_shell_moments_check.hpp"

namespace {

int unexpected = 0;

// code == NXC_OK: accepted; otherwise refused with that code and `text` in the message
void report(const char *name, const ShellMomentsRefusal &r, int code, const char *text)
{
    const bool ok = r.code == code && r.why && (code == NXC_OK ? r.why[0] == 0 : std::strstr(r.why, text) != nullptr);
    if (r.code == NXC_OK)
        std::printf("%s accepted%s\n", name, ok ? "" : " -- UNEXPECTED");
    else
        std::printf("%s refused (%d): %s%s\n", name, r.code, r.why ? r.why : "(null)", ok ? "" : " -- UNEXPECTED");
    if (!ok) unexpected++;
}

void expect_bytes(const char *name, int64_t plane, size_t bytes)
{
    const size_t got = shell_moments_bytes(plane);
    std::printf("%s: %zu bytes%s\n", name, got, got == bytes ? " ok" : " -- UNEXPECTED");
    if (got != bytes) unexpected++;
}

}  // namespace

int main()
{
    const int64_t LIMIT = int64_t(1) << 31;
    const int64_t plane = int64_t(72) * 36 * 34 * 2;           // 72 x 36 x 32
    const ShellMomentsState none = {false, false, false, 0}, unset = {true, false, false, 0},
                            set = {true, true, false, plane}, on = {true, true, true, plane},
                            stale = {true, false, true, plane};
    double out[2] = {0.0, 0.0};

    report("enable on a set map", check_shell_moments_enable(set), NXC_OK, "");
    report("enable again", check_shell_moments_enable(on), NXC_OK, "");
    report("enable on 1 x 1 x 1", check_shell_moments_enable({true, true, false, 6}), NXC_OK, "");
    report("enable, 2^31 - 1 records", check_shell_moments_enable({true, true, false, 2 * (LIMIT - 1)}),
           NXC_OK, "");
    report("accumulate when enabled", check_shell_moments_ready(on), NXC_OK, "");
    report("download when enabled", check_shell_moments_download(on, out), NXC_OK, "");

    report("enable, null handle", check_shell_moments_enable(none), NXC_ERR_STATE, "nxc_shell_set");
    report("enable before the set", check_shell_moments_enable(unset), NXC_ERR_STATE, "nxc_shell_set");
    report("enable, no records", check_shell_moments_enable({true, true, false, 0}), NXC_ERR_ARG, "2^31");
    report("enable, negative plane", check_shell_moments_enable({true, true, false, -8}), NXC_ERR_ARG, "2^31");
    report("enable, odd plane", check_shell_moments_enable({true, true, false, 7}), NXC_ERR_ARG, "2^31");
    report("enable, 2^31 records", check_shell_moments_enable({true, true, false, 2 * LIMIT}),
           NXC_ERR_ARG, "2^31");
    report("enable, INT64_MAX - 1 doubles",
           check_shell_moments_enable({true, true, false, std::numeric_limits<int64_t>::max() - 1}),
           NXC_ERR_ARG, "2^31");
    report("accumulate, null handle", check_shell_moments_ready(none), NXC_ERR_STATE, "nxc_shell_set");
    report("accumulate before the set", check_shell_moments_ready(unset), NXC_ERR_STATE, "nxc_shell_set");
    report("accumulate, set after an enable", check_shell_moments_ready(stale), NXC_ERR_STATE, "nxc_shell_set");
    report("accumulate before the enable", check_shell_moments_ready(set), NXC_ERR_STATE,
           "moments not enabled");
    report("download, null handle", check_shell_moments_download(none, out), NXC_ERR_STATE, "nxc_shell_set");
    report("download before the set", check_shell_moments_download(unset, out), NXC_ERR_STATE, "nxc_shell_set");
    report("download before the enable", check_shell_moments_download(set, out), NXC_ERR_STATE,
           "moments not enabled");
    report("download, null output", check_shell_moments_download(on, nullptr), NXC_ERR_ARG, "bad arguments");
    report("download, 2^31 records", check_shell_moments_download({true, true, true, 2 * LIMIT}, out),
           NXC_ERR_ARG, "2^31");

    expect_bytes("72 x 36 x 32", plane, (size_t)plane * 6 * 8);
    expect_bytes("one record", 2, 96);
    expect_bytes("2^31 - 1 records", 2 * (LIMIT - 1), (size_t)(2 * (LIMIT - 1)) * 48);
    expect_bytes("2^31 records", 2 * LIMIT, 0);
    expect_bytes("odd", 9, 0);
    expect_bytes("none", 0, 0);

    std::printf("%d unexpected\n", unexpected);
    return unexpected ? 1 : 0;
}
