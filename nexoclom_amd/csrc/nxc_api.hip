// nxc_api.hip -- C ABI (include/nexoclom_hip.h) over the gfx950 kernels of nxc_kernels.hpp.
//
// Host side of the boundary: owns the device, one stream, the packed table blob, the resident
// packet set and the resident image pair; translates nxc_forces / nxc_image_desc into kernel
// arguments; never throws across the boundary.  RCCL is loaded lazily with dlopen so that the
// library loads (and every single-GPU call works) where librccl is absent.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nexoclom_hip.h"
#include "nxc_camera_check.hpp"
#include "nxc_shell_check.hpp"
#include "nxc_shell_moments_check.hpp"
#include "nxc_cube_check.hpp"
#include "nxc_ages_check.hpp"
#include "nxc_los_profile_check.hpp"
#include "nxc_desc_check.hpp"
#include "nxc_source_map_check.hpp"
#include "nxc_frame_check.hpp"
#include "nxc_devbuf.hpp"
#include "nxc_image_block.hpp"
#include "nxc_kernels.hpp"
#include "nxc_log_table.hpp"
#include "nxc_spectrum_check.hpp"

namespace {

thread_local std::string g_error;

int fail(int code, const std::string &msg)
{
    g_error = msg;
    return code;
}

// No C++ exception may cross the C ABI: entry points that allocate on the host run inside this.
template <class F>
int guarded(F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(NXC_ERR_ARG, "out of host memory");
    } catch (const std::exception &e) {
        return fail(NXC_ERR_ARG, std::string("unexpected C++ exception: ") + e.what());
    } catch (...) {
        return fail(NXC_ERR_ARG, "unexpected C++ exception");
    }
}

// A wait that ended because a collective missed its deadline (stream_sync below) leaves its
// verdict here; the HIP-error path then reports NXC_ERR_RCCL with that text instead of the
// stand-in hipError_t.
thread_local std::string g_coll_failure;

int fail_hip(const char *expr, hipError_t e)
{
    if (!g_coll_failure.empty()) {
        std::string msg;
        msg.swap(g_coll_failure);
        return fail(NXC_ERR_RCCL, msg);
    }
    // out of device memory has a status of its own: callers split the work on it (Input.run)
    return fail(e == hipErrorOutOfMemory ? NXC_ERR_NOMEM : NXC_ERR_HIP,
                std::string(expr) + ": " + hipGetErrorString(e));
}

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail_hip(#expr, e_);                                    \
    } while (0)

constexpr int BLOCK_PERSIST = NXC_BLOCK_PERSIST;
#ifndef NXC_VAR_FAIR_PACKETS_PER_LANE_N       // (tools/gpu_exp_var_forms.sh)
#define NXC_VAR_FAIR_PACKETS_PER_LANE_N 24
#endif
constexpr double NXC_VAR_FAIR_PACKETS_PER_LANE = NXC_VAR_FAIR_PACKETS_PER_LANE_N;
static_assert(NXC_DEV_MAX_MOONS == NXC_MAX_MOONS, "device / ABI moon capacity");

// ---- RCCL, resolved at first use ------------------------------------------------------------
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t,
                              ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*CommGetAsyncError)(ncclComm_t, ncclResult_t *) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl g_rccl;

int rccl_load()
{
    if (g_rccl.ok) return NXC_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *nm : names) {
        g_rccl.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return fail(NXC_ERR_RCCL, std::string("dlopen(librccl): ") + dlerror());
#define SYM(field, name)                                                                     \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.lib, name));        \
    if (!g_rccl.field) return fail(NXC_ERR_RCCL, std::string("dlsym ") + name + " failed");
    SYM(GetUniqueId, "ncclGetUniqueId")
    SYM(CommInitRank, "ncclCommInitRank")
    SYM(AllReduce, "ncclAllReduce")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(CommAbort, "ncclCommAbort")
    SYM(CommGetAsyncError, "ncclCommGetAsyncError")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    g_rccl.ok = true;
    return NXC_OK;
}

#define NCCLCHK(expr)                                                                        \
    do {                                                                                     \
        ncclResult_t r_ = (expr);                                                            \
        if (r_ != ncclSuccess)                                                               \
            return fail(NXC_ERR_RCCL, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
    } while (0)

// ---- packed lookup table ----------------------------------------------------------------------
struct PackedLut {
    LutDesc desc{};
    std::vector<unsigned char> bytes;
};
struct LosLutCache {
    int64_t n = 0;
    std::vector<double> v, g;
    PackedLut lut;
};

// The device's cell computation (nxc_device.hpp: lut_cell), operation for operation: two roundings,
// a saturating conversion, a clamp.
int lut_cell_host(double x, double xbase, double inv_w, int ncell)
{
    const double s = (x - xbase) * inv_w;
    long long c;
    if (!(s >= 0.0)) c = 0;                       // negatives and NaN
    else if (s >= 2147483647.0) c = 2147483647ll;
    else c = (long long)s;
    return (int)std::min<long long>(c, ncell + 1);
}

// Doubles as ordered unsigned integers (monotone for finite values and the infinities).
unsigned long long ordered_key(double v)
{
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
double from_ordered_key(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

int pack_lut(const double *xp, const double *fp, int64_t n, PackedLut &out, const char *what,
             int cells_per_node = 4)
{
    if (n < 2 || n > 65000 || !xp || !fp)
        return fail(NXC_ERR_ARG, std::string(what) + ": table needs 2..65000 points");
    for (int64_t j = 0; j + 1 < n; j++)
        if (!(xp[j + 1] > xp[j]))
            return fail(NXC_ERR_ARG, std::string(what) + ": abscissae must be strictly ascending");
    for (int64_t j = 0; j < n; j++)
        if (!std::isfinite(xp[j]) || !std::isfinite(fp[j]))
            return fail(NXC_ERR_ARG, std::string(what) + ": table values must be finite");
    int ncell = 64;
    while (ncell < cells_per_node * n && ncell < 16384) ncell <<= 1;
    const int64_t rows = n + 2;
    const size_t cell_bytes = ((size_t)(ncell + 2) * sizeof(unsigned short) + 31) & ~size_t(31);
    out.bytes.assign((size_t)rows * 32 + cell_bytes, 0);
    double *rec = reinterpret_cast<double *>(out.bytes.data());     // {xp, xn} pairs
    double *fs = rec + 2 * rows;                                    // {fp, slope} pairs
    rec[0] = -std::numeric_limits<double>::max(); rec[1] = xp[0];   // row 0: below the table
    fs[0] = fp[0]; fs[1] = 0.0;
    for (int64_t j = 0; j < n; j++) {
        const bool last = j + 1 == n;
        rec[2 * (j + 1)] = xp[j];
        rec[2 * (j + 1) + 1] = last ? HUGE_VAL : xp[j + 1];
        fs[2 * (j + 1)] = fp[j];
        // np.interp's slope, the same IEEE quotient
        fs[2 * (j + 1) + 1] = last ? 0.0 : (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
        if (!std::isfinite(fs[2 * (j + 1) + 1]))
            return fail(NXC_ERR_ARG, std::string(what) + ": table slopes must be finite");
    }
    rec[2 * (n + 1)] = HUGE_VAL; rec[2 * (n + 1) + 1] = HUGE_VAL;   // sentinel: never selected
    fs[2 * (n + 1)] = fp[n - 1]; fs[2 * (n + 1) + 1] = 0.0;
    const double x0 = xp[0], xl = xp[n - 1];
    const double inv_w = (double)ncell / (xl - x0);
    const double xbase = x0 - (xl - x0) / (double)ncell;
    if (!std::isfinite(inv_w) || !std::isfinite(xbase) || !(xbase < x0))
        return fail(NXC_ERR_ARG, std::string(what) + ": abscissa range cannot be indexed");
    // cell[c] = the last row whose xp <= the smallest double that the device maps to cell c
    // (bisection over the ordered doubles with the device's own arithmetic; cell 0 starts at
    // -inf).  Row xp's: row 0 = -DBL_MAX, row j + 1 = xp[j].
    unsigned short *cell = reinterpret_cast<unsigned short *>(rec + 4 * rows);
    cell[0] = 0;
    const unsigned long long k_lo = ordered_key(-std::numeric_limits<double>::max());
    const unsigned long long k_hi = ordered_key(std::numeric_limits<double>::max());
    for (int c = 1; c <= ncell + 1; c++) {
        if (lut_cell_host(from_ordered_key(k_hi), xbase, inv_w, ncell) < c)
            return fail(NXC_ERR_ARG, std::string(what) + ": cell index is not onto");
        unsigned long long lo = k_lo, hi = k_hi;   // cell(lo) < c <= cell(hi)
        while (hi - lo > 1) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            if (lut_cell_host(from_ordered_key(mid), xbase, inv_w, ncell) >= c) hi = mid;
            else lo = mid;
        }
        const double first = from_ordered_key(hi);
        const int64_t j = std::upper_bound(xp, xp + n, first) - xp;  // nodes with xp <= first
        cell[c] = (unsigned short)j;                                  // row j = node j - 1 (0: below)
    }
    out.desc.rec = 0;                               // offsets relative to the table: placed_lut()
    out.desc.fs = 16 * (int)rows;
    out.desc.cell = 32 * (int)rows;
    out.desc.top = ncell + 1;
    out.desc.last = (int)n + 1;
    out.desc.xbase = xbase;
    out.desc.inv_w = inv_w;
    return NXC_OK;
}

// The g-value tables of an image-shaped descriptor, packed
int pack_lines(int n_lines, const double *const *v, const double *const *g, const int64_t *n, PackedLut *out)
{
    for (int l = 0; l < n_lines; l++) {
        int rc = pack_lut(v[l], g[l], n[l], out[l], "g-value table");
        if (rc) return rc;
    }
    return NXC_OK;
}

// Largest double x with sqrt(x) <= e (host sqrt is correctly rounded): r2 > x <=> sqrt(r2) > e,
// the constant driver's escape test (Output.py:395,410) without a device square root.
double sqrt_threshold(double e)
{
    if (!(e > 0) || !std::isfinite(e)) return e;
    double x = e * e;
    if (!std::isfinite(x)) return HUGE_VAL;
    while (std::sqrt(x) > e) x = std::nextafter(x, 0.0);
    while (std::sqrt(std::nextafter(x, HUGE_VAL)) <= e) x = std::nextafter(x, HUGE_VAL);
    return x;
}

// h*a[n+1][i] for a launch-uniform step: the products NumPy forms per packet (rk5.py:33).
StepW make_stepw(double h)
{
    StepW w{};
    w.h = h;
    for (int n = 0; n < 6; n++)
        for (int i = 0; i <= n; i++) w.w[n * (n + 1) / 2 + i] = h * Tableau::A[n + 1][i];
    return w;
}

// What owns a device allocation (nxc_devbuf.hpp) allocates through HIP, reports as HIPCHK does and
// has the blocks kept from freed row stores given back before an allocation is refused
void flush_all_pools();
struct HipAlloc {
    static inline thread_local hipError_t last = hipSuccess;   // for callers that word a refusal themselves
    static int alloc(void **ptr, size_t bytes)
    {
        if ((last = hipMalloc(ptr, bytes)) == hipSuccess) return NXC_OK;
        (void)hipGetLastError();
        return fail_hip("hipMalloc(ptr, bytes ? bytes : 8)", last);
    }
    static int free(void *ptr) { HIPCHK(hipFree(ptr)); return NXC_OK; }
    static int flush() { flush_all_pools(); return NXC_OK; }
};
template <typename T> using Dev = DevBuf<T, HipAlloc>;

}  // namespace

// Device-resident compact trajectory rows (nxc_rows_build): nine value columns [9][total] and the
// packet-index column, as float32/int32 (what save() stores, Output.py:528-543) or float64/int64.
struct nxc_rows {
    int device = 0;
    bool f32 = false;
    long long total = 0;
    void *d_cols = nullptr;
    void *d_index = nullptr;
    size_t cols_cap = 0, index_cap = 0;      // bytes of the two blocks (they may come from the pool)
};

// Device blocks of freed row stores, kept for the next store.  hipMalloc / hipFree themselves return
// in under a millisecond on this driver (now and then 30-150 ms beside a running kernel); what a
// fresh block costs is its first touch -- a 51 GB catalogue written into new memory takes about
// 0.1 s longer than into pooled blocks (NXC_POOL_TRACE=1 prints every take and give;
// tools/gpu_exp_run_breakdown.py).  The pool counts as free memory (nxc_mem_info) and is emptied
// before anything is refused for lack of it.
struct BlockPool {
    struct Block { void *p; size_t bytes; };
    std::vector<Block> blocks;
    size_t bytes = 0;
    std::mutex lock;                         // stores are freed by whichever thread drops them
};

// A device list of (spectrum, row) pairs: what a line-of-sight pass found with weight > 0
// (nxc_los_set_pairs), [2][cap] int64 as the kernels write them.  Owned by its creator.
struct nxc_pairs {
    int device = 0;
    long long cap = 0, n = 0;        // n: pairs the last pass found (<= cap, or that pass failed)
    Dev<long long> d;
};

// An age block on the device: `sets` sets of records x (na + 2) 16-byte records {sum, sum of
// squares}, there from its enable (ages_enable) to the next set of what owns it.  One type for the
// image, the camera, the density, the shell map and the lines of sight.
struct AgeBlock {
    bool have = false;               // nxc_X_ages_enable since the owner's last set
    AgeK K{};
    int64_t records = 0;             // per set: pixels, points, spectra, records of the shell map
    int sets = 1;                    // NXC_SHELL_AGE_PLANES for the shell map: {w, w w} | {c, c c}
    Dev<double> d;                   // [sets][records][na + 2] records
    size_t bytes() const { return ages_block_bytes(sets, records, K.na); }
    int release() { have = false; return d.release(); }     // off, its records back to the device
};

// What a pixel grid owns on the device, ModelImage's (nxc_set_image) and CameraImage's
// (nxc_camera_set) alike.  The moments, the cube and the age block are there from their enable to
// the next set, each a state of its own.
struct PixelSums {
    Dev<double> image;               // interleaved {weight sum, packet count} per pixel, fp64
    size_t npix = 0;
    bool have_mom = false;           // nxc_X_moments_enable since the last set
    Dev<double> mom;                 // the pixel moments: [2][npix] 16-byte records (k_X_moments)
    bool have_cube = false;          // nxc_X_cube_enable since the last set
    Dev<double> cube;                // the velocity cube: [npix][nv + 2] records (k_X_cube)
    CubeK cubeK{};
    AgeBlock ages;                   // the age cube: [npix][na + 2] records (k_X_ages)
};

// Stored samples on the device, as every consumer (image, line of sight, density, fit) reads them:
// a row range of a store (samples_from_rows) or host columns uploaded (samples_upload)
struct Samples {
    bool f32 = false, index64 = true;
    int64_t n = 0, shift = 0;                // rows, index shift
    const void *cols[8] = {};                // x, y, z, vy, frac, vx, vz, time (null where nobody reads it)
    const void *index = nullptr;             // null where the entry allows it
    const nxc_rows *store = nullptr;         // stores: the store, column 0 of row 0 and the
    const void *col0 = nullptr;              // distance between columns (the fit's rows copy
    int64_t stride = 0;                      // all nine columns)
    template <typename T> const T *col(int c) const { return static_cast<const T *>(cols[c]); }
    template <typename I> const I *idx() const { return static_cast<const I *>(index); }
};

struct nxc_handle {
    int device = 0;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // row-store downloads, streamed uploads: beside the compute stream
    hipStream_t stream2 = nullptr;       // streamed pass: the pieces' ordering kernels
    Dev<unsigned long long> d_piece_hist;   // streamed pass: sort bins (+ max) per piece, then the
                                            // word that publishes the queue positions ready
    hipEvent_t ev_piece[33] = {};        // ... piece p uploaded; [32]: start / join
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    char name[256] = {0};

    // Every have_* flag here and below goes false before the first call that can fail touches what
    // it guards, and true after the last such call: a set or an enable that fails leaves its entries
    // refusing with NXC_ERR_STATE, never reading half-made state.
    // tables
    bool have_forces = false, have_image = false;
    ForceK F{};
    ImageK G{};
    PackedLut force_lut;
    std::vector<double> force_v, force_a;        // raw table (re-packed with fewer cells if LDS is short)
    int force_cells_per_node = 16;
    int force_lut_cells = 0;                     // cells per node force_lut was packed with
    std::vector<unsigned char> image_part;       // lines, then xedges, zedges
    LdsHeader header{};                          // host copy of the blob's first bytes
    ImageBlock<LutDesc> image_block;             // where image_part's pieces sit
    Dev<unsigned char> d_blob;
    size_t force_bytes = 0, all_bytes = 0;
    Dev<unsigned char> d_blob_img;               // [LdsHeader | image part] for the kernels that bin
    size_t img_bytes = 0;                        // stored samples: no force table in their LDS

    // resident data
    PixelSums img;                   // ModelImage's pair, moments and cube
    Dev<double> d_packets;
    int64_t n_packets = 0;
    Dev<unsigned> d_order;           // packet indices by decreasing launch speed (queue order)
    Dev<double> d_queue;             // the packets in that order, one 64-byte record each: [n][8]
    bool have_order = false;
    int order_key = 0;               // what the queue is sorted by: 0 |v|^2, 1 known lifetimes, 2 the adaptive driver's key
    int64_t first_id = 0;            // global index of resident packet 0 (RNG counter space)
    bool have_bounce = false;
    Dev<double> d_bounce;            // spline knots + coefficients of the accommodation table
    bool have_stick_map = false;
    Dev<double> d_stick_map;         // sticking map: longitude nodes, latitude nodes, coefficients
    Dev<double> d_source;            // sampler tables: speed CDF + speeds, surface density map
    Dev<DevCounters> d_ctr;
    Dev<double> d_scratch;           // final states / generic device scratch
    Dev<unsigned char> d_samples;    // host sample columns on their way to k_image / k_los
    Dev<unsigned char> d_tiles;      // chunk scratch of the tiled image (k_image_bin -> k_image_tiles)
    Dev<unsigned char> d_losblk;     // block descriptors + spheres (k_los_blocks -> k_los)
    int image_mode = 0;                   // nxc_image_mode: 0 by size, 1 k_image, 2 tiles
    int tile_pixels = NXC_TILE_PIXELS;
    int64_t tile_slab = int64_t(1) << 28; // samples per pass of the tiled image (bounds its scratch)
    Dev<long long> d_steps;
    Dev<unsigned long long> d_hist;  // counting-sort bins of the queue order
    Dev<void> d_rec;                 // pass 2's records on their way to columns (grow-only)

    BlockPool pool;
    LosLutCache los_lut[NXC_MAX_LINES];   // the g-value tables of the last line-of-sight call, packed

    // compact-rows protocol (nxc_integrate_const_rows -> nxc_rows_fetch)
    Dev<long long> d_offsets;
    long long rows_total = -1;
    double rows_step = 0, rows_edge = 0;
    int64_t rows_n_iter = 0, rows_n = 0;
    // adaptive-step rows (nxc_integrate_var_resident -> nxc_var_rows_build): the packets whose finals
    // [8][n] and stored steps [n] sit in d_scratch, or -1
    int64_t var_n = -1;

    bool have_bodies = false;
    nxc_bodies_desc bodies{};
    Dev<double> d_moonpos;           // [n_iter][n_moons][cos, sin] of the per-step base phase

    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    bool streamed_pending = false;   // nxc_integrate_const_streamed since the last nxc_synchronize
    bool coll_pending = false;       // a collective sits on `stream` and nobody has waited for it yet
    hipEvent_t ev_pre_coll = nullptr; // recorded in front of the first pending collective
    std::atomic<bool> abort_requested{false};   // nxc_comm_request_abort (any thread)
    double coll_timeout_s = 120.0;   // nxc_comm_set_timeout / NXC_COLLECTIVE_TIMEOUT_S
    Dev<double> d_reduce;            // one double for control-plane reductions
    Dev<double> d_reduce_n;          // nxc_allreduce_f64's staging (grow-only)

    // ModelDensity (nxc_density_set): the point index and the {frac sum, count} pair per point
    bool have_density = false;
    DensityK dens{};
    int64_t dens_q = 0;
    Dev<double> d_dens_pts;          // [Q][4]: x, y, z, 0 (two 16-byte loads per candidate)
    Dev<int> d_dens_cell;            // cell starts [ncells + 1]
    Dev<double> d_dens_acc;          // interleaved pair [Q][2], as the image's
    bool have_dens_mom = false;      // nxc_density_moments_enable since the last nxc_density_set
    Dev<double> d_dens_mom;          // the moment sums: [5][Q] 16-byte records (k_density_moments)
    bool have_dens_spec = false;     // nxc_density_spectrum_enable since the last nxc_density_set
    SpectrumK dens_spec{};
    Dev<double> d_dens_spec;         // the spectrum: [2][Q][nv + 2] records (k_density_spectrum)
    Dev<double> d_dens_frames;       // [Q][8]: ux uy uz 0 bx by bz 0 per indexed point
    AgeBlock dens_ages;              // the ages: [Q][na + 2] records {f, f f} (k_density_ages)

    // CameraImage (nxc_camera_set): the camera, its LDS blob [LdsHeader | g tables | u edges |
    // v edges] and its own {weight sum, count} image
    bool have_camera = false;
    CameraK cam{};
    Dev<unsigned char> d_blob_cam;
    size_t cam_bytes = 0;
    PixelSums cam_px;                // the camera's pair, moments and cube

    // ShellMap (nxc_shell_set): the altitude axis, its LDS blob [LdsHeader | g tables | lon edges |
    // mu edges], its own {c sum, count} pair per cell and the two planes of records
    bool have_shell = false;
    ShellK shell{};
    Dev<unsigned char> d_blob_shell;
    size_t shell_bytes = 0;
    PixelSums shell_px;              // shell.replicas copies of the pair per cell, summed by the
                                     // download (its moments and cube stay off)
    Dev<double> d_shell_planes;      // [2][cells][nalt + 2] records: {w, w w} | {c, c c} (k_shell)
    bool have_shell_mom = false;     // nxc_shell_moments_enable since the last nxc_shell_set
    Dev<double> d_shell_mom;         // [6][cells][nalt + 2] records: the twelve sums (k_shell_moments)
    AgeBlock shell_ages;             // [2][cells (nalt + 2)][na + 2] records: {w, w w} | {c, c c} (k_shell_ages)

    // LOSResultFitted: the pair list the line-of-sight passes fill (nxc_los_set_pairs); the fit's
    // per-spectrum data, its sample source and per-packet sums (nxc_fit_*)
    nxc_pairs *los_pairs = nullptr;
    // the line-of-sight profile (nxc_los_profile_enable): there from its enable to the next one
    bool have_los_prof = false;
    int64_t los_prof_S = 0;          // spectra it was enabled for
    CubeK los_profK{};
    Dev<double> d_los_prof;          // [S][nv + 2] records {w, w w} | [S][4] sums m1 m2 m3 ww
    // the line-of-sight ages (nxc_los_ages_enable): a block of their own, from enable to enable
    AgeBlock los_ages;               // [S][na + 2] records {w, w w}; records: the S it was enabled for
    bool have_fit = false;
    int64_t fit_S = 0, fit_np = -1;  // fit_np: packets whose multipliers are ready (nxc_fit_packets)
    int fit_mode = 0;
    bool have_fit_src = false;
    Samples fit_src;
    Dev<double> d_fit_spec;          // position [3][S] | ratio | weight | radiance sums | mask bytes
    Dev<unsigned char> d_fit_pk;     // num | den | mult (f64) | cnt | lengths (u32) per packet
    Dev<unsigned char> d_fit_smp;    // host columns of the fit on the device
    Dev<unsigned char> d_fit_aux;    // blob | counters, or nxc_fit_rows' tile scratch

    // source maps (nxc_source_map_*): the grid and tile segments, the resident map and unsmeared
    // histogram, and one Output's packets
    bool have_smap = false;
    SmapK smap{};
    int64_t smap_ntiles = 0, smap_ncells = 0;
    std::vector<double> smap_edges;  // alt | az | lon | lat edges (the speed edges come per Output)
    Dev<unsigned char> d_smap_grid;  // pt_lon | pt_lat | pt_cos | thr | seg_off | seg
    Dev<double> d_smap_acc;          // map [npoints][stride] | hist2d [npoints]
    Dev<unsigned char> d_smap_pk;    // columns | geo | bins | cell starts | edges | small
};

static int order_on_device(nxc_handle *h, double k2max, const long long *d_lifetimes,
                           int64_t max_steps, bool flight_key = false);

namespace {

// Wait for the handle's stream.  Without a collective in flight this is hipStreamSynchronize.
// With one (nxc_image_allreduce / nxc_allreduce_* since the last wait) the wait is bounded: the
// stream is polled together with ncclCommGetAsyncError, and when `coll_timeout_s` have passed --
// a peer rank died or never issued its half -- the communicator is aborted (ncclCommAbort makes
// the RCCL kernel leave), the handle is left without a communicator and the caller gets
// NXC_ERR_RCCL (through fail_hip) instead of waiting forever.
hipError_t stream_sync(nxc_handle *h)
{
    if (!h->coll_pending || !h->comm || !g_rccl.ok) {
        h->coll_pending = false;
        return hipStreamSynchronize(h->stream);
    }
    // what was queued before the collective is this process's own work: it ends by itself, and is
    // waited for the ordinary way (no polling beside a 40 ms kernel); the deadline runs from there
    if (h->ev_pre_coll) {
        const hipError_t e = hipEventSynchronize(h->ev_pre_coll);
        if (e != hipSuccess) { h->coll_pending = false; return e; }
    }
    timespec t0{};
    clock_gettime(CLOCK_MONOTONIC, &t0);
    auto elapsed = [&]() {
        timespec t{};
        clock_gettime(CLOCK_MONOTONIC, &t);
        return double(t.tv_sec - t0.tv_sec) + 1e-9 * double(t.tv_nsec - t0.tv_nsec);
    };
    std::string why;
    for (long spin = 0;; spin++) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) {
            h->coll_pending = false;
            return hipSuccess;
        }
        if (q != hipErrorNotReady) {
            h->coll_pending = false;
            return q;
        }
        if (h->abort_requested.load(std::memory_order_relaxed)) {
            why = "a peer rank reported a failure while this rank waited for a collective";
            break;
        }
        if ((spin & 63) == 63) {
            ncclResult_t async = ncclSuccess;
            const ncclResult_t r = g_rccl.CommGetAsyncError(h->comm, &async);
            if (r != ncclSuccess || (async != ncclSuccess && async != ncclInProgress)) {
                why = std::string("RCCL reported an asynchronous error (") +
                      g_rccl.GetErrorString(r != ncclSuccess ? r : async) + ")";
                break;
            }
            const double dt = elapsed();
            if (dt > h->coll_timeout_s) {
                char buf[160];
                std::snprintf(buf, sizeof buf,
                              "a collective of rank %d of %d did not complete within %.1f s (a peer "
                              "rank is gone or never joined it)", h->rank, h->nranks, h->coll_timeout_s);
                why = buf;
                break;
            }
            if (dt > 2e-3) {                       // past the latency of a healthy collective
                timespec nap{0, 200000};
                nanosleep(&nap, nullptr);
            }
        }
    }
    (void)g_rccl.CommAbort(h->comm);               // frees the communicator; its kernel exits
    h->comm = nullptr;
    h->nranks = 1;
    h->rank = 0;
    h->coll_pending = false;
    g_coll_failure = why + "; the communicator was aborted";
    return hipErrorNotReady;
}

// The handle's generic scratch with room for `bytes`.  Whoever takes it overwrites the finals an
// adaptive-step run may have left there (nxc_integrate_var_resident -> nxc_var_rows_build).
int scratch_for(nxc_handle *h, size_t bytes)
{
    h->var_n = -1;
    return h->d_scratch.ensure(bytes);
}

// NXC_POOL_TRACE=1: every take / give that reaches the driver, with its duration, on stderr
const bool g_pool_trace = std::getenv("NXC_POOL_TRACE") != nullptr;
size_t pool_bytes(nxc_handle *h);

void pool_flush(nxc_handle *h)
{
    std::lock_guard<std::mutex> g(h->pool.lock);
    for (const auto &b : h->pool.blocks) (void)hipFree(b.p);
    h->pool.blocks.clear();
    h->pool.bytes = 0;
}

// A block of at least `bytes`: the best fit in the pool that wastes less than a quarter, else new
// memory (the pool is given back to the driver before an allocation is allowed to fail).
hipError_t pool_take(nxc_handle *h, size_t bytes, void **out, size_t *cap)
{
    {
        std::lock_guard<std::mutex> g(h->pool.lock);
        int best = -1;
        for (int k = 0; k < (int)h->pool.blocks.size(); k++) {
            const size_t have = h->pool.blocks[(size_t)k].bytes;
            if (have >= bytes && have - bytes <= bytes / 4 &&
                (best < 0 || have < h->pool.blocks[(size_t)best].bytes))
                best = k;
        }
        if (best >= 0) {
            *out = h->pool.blocks[(size_t)best].p;
            *cap = h->pool.blocks[(size_t)best].bytes;
            h->pool.bytes -= *cap;
            h->pool.blocks.erase(h->pool.blocks.begin() + best);
            if (g_pool_trace) std::fprintf(stderr, "[nxc pool] hit  %8.1f MB in a block of %8.1f MB\n", bytes / 1e6, *cap / 1e6);
            return hipSuccess;
        }
    }
    timespec t0{}, t1{};
    if (g_pool_trace) clock_gettime(CLOCK_MONOTONIC, &t0);
    hipError_t e = hipMalloc(out, bytes ? bytes : 8);
    if (g_pool_trace) {
        clock_gettime(CLOCK_MONOTONIC, &t1);
        std::fprintf(stderr, "[nxc pool] miss %8.1f MB: hipMalloc %.1f ms (pool holds %.1f MB in %zu blocks)\n", bytes / 1e6,
                     (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6, pool_bytes(h) / 1e6, h->pool.blocks.size());
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pool_flush(h);
        e = hipMalloc(out, bytes ? bytes : 8);
    }
    *cap = e == hipSuccess ? bytes : 0;
    return e;
}

void pool_give(nxc_handle *h, void *p, size_t bytes)
{
    if (!p) return;
    size_t free_b = 0, total_b = 0;
    const bool known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    std::lock_guard<std::mutex> g(h->pool.lock);
    // small blocks are cheap to allocate; the pool never holds more than a third of the device
    if (!known || bytes < (size_t(64) << 20) || h->pool.bytes + bytes > total_b / 3 ||
        h->pool.blocks.size() >= 64) {
        timespec t0{}, t1{};
        if (g_pool_trace) clock_gettime(CLOCK_MONOTONIC, &t0);
        (void)hipFree(p);
        if (g_pool_trace && bytes >= (size_t(64) << 20)) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            std::fprintf(stderr, "[nxc pool] full: hipFree of %8.1f MB %.1f ms\n", bytes / 1e6,
                         (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6);
        }
        return;
    }
    h->pool.blocks.push_back({p, bytes});
    h->pool.bytes += bytes;
}

// every live handle, for allocations that have no handle at hand (HipAlloc::flush)
std::mutex g_handles_lock;
std::vector<nxc_handle *> g_handles;

void flush_all_pools()
{
    std::lock_guard<std::mutex> g(g_handles_lock);
    for (nxc_handle *h : g_handles) pool_flush(h);
}

size_t pool_bytes(nxc_handle *h)
{
    std::lock_guard<std::mutex> g(h->pool.lock);
    return h->pool.bytes;
}

// Device blob = [LdsHeader | force table | g-value tables | x edges | z edges]; kernels stage
// the first force_bytes (integrator only) or all_bytes (image) of it into LDS.  `with_image`: the
// handle's image part goes in (have_image, or nxc_set_image on its way to setting it).
int upload_blob(nxc_handle *h, bool with_image)
{
    const size_t hb = NXC_HEADER_BYTES;
    const size_t ib = with_image ? h->image_part.size() : 0;
    const size_t limit = 160 * 1024 - 32 - (size_t)(BLOCK_PERSIST / 64) * NXC_WAVE_LDS_BYTES;
    // (the row-writing kernels stage two more words per queued packet and no image tables)
    const size_t limit_rows = 160 * 1024 - 32 - (size_t)(BLOCK_PERSIST / 64) * NXC_WAVE_LDS_BYTES_ROWS;
    size_t fb = h->have_forces ? h->force_lut.bytes.size() : 0;
    while (h->have_forces && (hb + fb + ib > limit || hb + fb > limit_rows) &&
           h->force_cells_per_node > 2) {
        h->force_cells_per_node /= 2;          // trade lookup hit rate for LDS space
        PackedLut lut;
        int rc2 = pack_lut(h->force_v.data(), h->force_a.data(), (int64_t)h->force_v.size(), lut,
                           "nxc_forces radiation table", h->force_cells_per_node);
        if (rc2) return rc2;
        h->force_lut = std::move(lut);
        h->force_lut_cells = h->force_cells_per_node;
        fb = h->force_lut.bytes.size();
    }
    h->force_bytes = hb + fb;
    h->all_bytes = hb + fb + ib;
    if (h->all_bytes > limit || h->force_bytes > limit_rows)
        return fail(NXC_ERR_ARG, "lookup tables exceed the 160 KiB LDS of a gfx950 CU");
    int rc = h->d_blob.ensure(h->all_bytes);
    if (rc) return rc;
    h->F.tab = placed_lut(h->force_lut.desc, hb);
    if (with_image) place_image_block(h->image_block, hb + fb, h->G);
    h->header.G = h->G;
    HIPCHK(hipMemcpyAsync(h->d_blob, &h->header, sizeof(LdsHeader), hipMemcpyHostToDevice,
                          h->stream));
    if (fb) HIPCHK(hipMemcpyAsync(h->d_blob + hb, h->force_lut.bytes.data(), fb,
                                  hipMemcpyHostToDevice, h->stream));
    if (ib) HIPCHK(hipMemcpyAsync(h->d_blob + hb + fb, h->image_part.data(), ib,
                                  hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    if (with_image) {
        // the same image tables right behind the header: k_image stages 45 KB instead of 100+, so
        // that several of its workgroups fit a CU (it was one 256-thread group per CU)
        LdsHeader hdr = h->header;
        place_image_block(h->image_block, hb, hdr.G);
        h->img_bytes = hb + ib;
        rc = h->d_blob_img.ensure(h->img_bytes);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h->d_blob_img, &hdr, sizeof(LdsHeader), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_blob_img + hb, h->image_part.data(), ib, hipMemcpyHostToDevice,
                              h->stream));
        HIPCHK(stream_sync(h));      // hdr is a local
    }
    return NXC_OK;
}

// Put this launch's step weights into the header (stream-ordered before the kernel).
int upload_step(nxc_handle *h, double step)
{
    h->header.W = make_stepw(step);
    HIPCHK(hipMemcpyAsync(h->d_blob + offsetof(LdsHeader, W), &h->header.W, sizeof(StepW),
                          hipMemcpyHostToDevice, h->stream));
    return NXC_OK;
}

template <class K>
int prep_kernel(K kernel, size_t lds_bytes)
{
    if (lds_bytes > 64 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return NXC_OK;
}

int begin_timed(nxc_handle *h)
{
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return NXC_OK;
}
int end_timed(nxc_handle *h)
{
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return NXC_OK;
}

// In front of a persistent kernel's launch: its LDS limit is raised, its grid is formed, and the
// timing that end_timed() closes after the launch is started.  The grid: one resident block per CU slot.  When there are fewer packets than
// lanes (one reference-sized chunk of 80 467 packets against 196 608 lanes), the packets are
// spread over ALL CUs with fewer waves per block instead of filling a few CUs three waves deep: a
// packet's steps run one after the other, and a wave that has its SIMD to itself takes them
// faster.  *block comes back as the number of threads to launch per block (a multiple of 64).
template <class K>
int prepare_persistent_launch(nxc_handle *h, K kernel, int *block, size_t lds_bytes, int64_t n, int *grid)
{
    int per_cu = 0, rc;
    if ((rc = prep_kernel(kernel, lds_bytes))) return rc;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, *block, lds_bytes));
    if (per_cu < 1) per_cu = 1;
    int64_t g = (int64_t)h->n_cu * per_cu;
    const int64_t waves = (n + 63) / 64;
    if (waves < g * (*block / 64)) {
        int64_t per_block = (waves + g - 1) / g;
        if (per_block < 1) per_block = 1;
        *block = (int)per_block * 64;
        g = (waves + per_block - 1) / per_block;
    }
    if (g < 1) g = 1;
    *grid = (int)g;
    return begin_timed(h);
}

int flat_grid(nxc_handle *h, int64_t n, int block)
{
    int64_t g = (n + block - 1) / block;
    const int64_t cap = (int64_t)h->n_cu * 8;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

int need_forces(nxc_handle *h)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (!h->have_forces) return fail(NXC_ERR_STATE, "nxc_set_forces has not been called");
    HIPCHK(hipSetDevice(h->device));
    return NXC_OK;
}

// Per-step base phases of the moons, (cos, sin)(phi - omega (t0 - k h)), and the per-stage rotations
// (cos, sin)(omega c_n h) in the header.  Host libm sincos(); the oracle builds the same numbers
// the same way.
int upload_moon_table(nxc_handle *h, double step, int64_t n_iter)
{
    static const double cn[6] = {0, 0.2, 0.3, 0.8, 8. / 9., 1.};
    const nxc_bodies_desc &b = h->bodies;
    const int nm = b.n_moons;
    BodyK &K = h->header.Bd;
    for (int n = 0; n < 6; n++)
        for (int m = 0; m < nm; m++) {
            double sn, cs;
            ::sincos(b.omega[m] * (cn[n] * step), &sn, &cs);
            K.cd[n][m] = cs; K.sd[n][m] = sn;
        }
    HIPCHK(hipMemcpyAsync(h->d_blob + offsetof(LdsHeader, Bd), &h->header.Bd, sizeof(BodyK),
                          hipMemcpyHostToDevice, h->stream));
    const size_t count = (size_t)(n_iter > 0 ? n_iter : 1) * 2 * (size_t)(nm > 0 ? nm : 1);
    std::vector<double> base(count, 0.0);
    for (int64_t k = 0; k < n_iter; k++) {
        const double t = b.t0 - (double)k * step;
        for (int m = 0; m < nm; m++) {
            double sn, cs;
            ::sincos(b.phi[m] - b.omega[m] * t, &sn, &cs);
            base[((size_t)k * nm + m) * 2] = cs;
            base[((size_t)k * nm + m) * 2 + 1] = sn;
        }
    }
    int rc = h->d_moonpos.ensure(count * sizeof(double));
    if (rc) return rc;
    // pageable source: the copy is staged before the call returns
    HIPCHK(hipMemcpyAsync(h->d_moonpos, base.data(), count * sizeof(double), hipMemcpyHostToDevice,
                          h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

// What one launch of the persistent integrator works on besides the handle's resident set: the
// packets in the order they are taken, and where the per-packet results go.
struct FusedJob {
    const double *soa = nullptr;
    const unsigned *order = nullptr;
    const unsigned long long *avail = nullptr;   // streamed upload: positions published so far
    double *final = nullptr;                     // per-packet outputs: final states [8][n] ...
    long long *steps = nullptr;                  // ... and steps taken [n]
    const long long *offsets = nullptr;          // rows pass: every packet's first row [n + 1] ...
    void *rec = nullptr;                         // ... of the record buffer
};

FusedJob whole_set(nxc_handle *h)
{
    FusedJob j;
    j.soa = h->have_order ? h->d_queue : h->d_packets;
    j.order = h->have_order ? h->d_order : nullptr;
    return j;
}

// Every instantiation of k_const_fused that exists, at its variant's code: the template arguments
// are decode()'s, what exists is valid()'s (nxc_fused_variant.hpp).
using FusedKernel = decltype(&k_const_fused<0, false, false>);

template <int CODE>
constexpr FusedKernel fused_kernel()
{
    constexpr FusedVariant v = decode(CODE);
    if constexpr (valid(v)) return k_const_fused<v.image, v.bounce, v.full, v.nbody, v.rows, v.streamed>;
    else return nullptr;
}

template <int... CODE>
FusedKernel fused_kernel(int code, std::integer_sequence<int, CODE...>)
{
    static const FusedKernel table[] = {fused_kernel<CODE>()...};
    return table[code];
}

// The one launch of k_const_fused, over `job`: the variant for the handle's force model, moons or
// re-emission and this call (image: binned; rows: 0 none, 1 wide, 2 narrow records).
int launch_fused(nxc_handle *h, bool image, int rows, int64_t n_iter, double outeredge, const FusedJob &job)
{
    const FusedVariant v = pick_variant(h->F.grav != 0, h->F.rad != 0, h->F.loss == LOSS_PHOTO, h->have_bodies,
                                        h->have_bounce, image, h->G.downcast_f32 != 0, rows, job.avail != nullptr);
    const FusedKernel kernel =
        valid(v) ? fused_kernel(encode(v), std::make_integer_sequence<int, NXC_FUSED_CODES>()) : nullptr;
    if (!kernel) return fail(NXC_ERR_STATE, "no constant-step kernel for this combination of passes");
    const size_t tables = v.image ? h->all_bytes : h->force_bytes, lds = persist_lds(tables, v);
    int grid = 1, block = BLOCK_PERSIST, rc;
    if ((rc = prepare_persistent_launch(h, kernel, &block, lds, h->n_packets, &grid))) return rc;
    // tests: "<blocks>x<waves per block>" -- fewer lanes than packets at small sizes, so that lanes
    // take second packets; anything else is ignored.  lds stays sized for a full block.
    if (const char *t = std::getenv("NXC_TEST_FUSED_WAVES")) {
        int b = 0, w = 0;
        char rest = 0;
        if (std::sscanf(t, "%dx%d%c", &b, &w, &rest) == 2 && b >= 1 && b <= h->n_cu && w >= 1 &&
            w <= BLOCK_PERSIST / 64) {
            grid = b; block = w * 64;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, h->stream, h->F, h->d_blob,
                       (int64_t)tables, h->n_packets, job.soa, job.order, h->first_id, n_iter,
                       sqrt_threshold(outeredge), job.final, job.steps,
                       v.image ? h->img.image : (double *)nullptr, h->d_ctr,
                       v.nbody ? h->d_moonpos : (const double *)nullptr, job.offsets, job.rec, job.avail);
    HIPCHK(hipGetLastError());
    return end_timed(h);
}

// The constant-step kernels want the fastest (longest-lived) packets first: a resident set that the
// adaptive driver has re-sorted for itself goes back to that order.
int speed_order_for_const(nxc_handle *h)
{
    if (h->order_key != 2 || h->n_packets < 2) return NXC_OK;
    return order_on_device(h, -1.0, nullptr, 0);
}

// In front of a constant-step launch over the resident packets: what cannot run is refused before
// anything is touched (sticking law 2 reads the map at every impact: no launch without one), then
// the step weights, the zeroed counters and the moons' phases.
int const_preamble(nxc_handle *h, double step, int64_t n_iter)
{
    if (h->have_bodies && h->have_bounce)
        return fail(NXC_ERR_STATE, "surface re-emission is not available with moons set");
    if (h->have_bounce && h->header.B.temp_dependent == 2 && !h->have_stick_map)
        return fail(NXC_ERR_STATE, "the bounce description asks for sticking from a surface map "
                                   "(temp_dependent = 2) and no map is set (nxc_set_stick_map)");
    if (int rc = upload_step(h, step)) return rc;
    HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
    return h->have_bodies ? upload_moon_table(h, step, n_iter) : NXC_OK;
}

int launch_const(nxc_handle *h, double step, int64_t n_iter, double outeredge, bool image,
                 double *d_final, long long *d_steps)
{
    if (int rc = const_preamble(h, step, n_iter)) return rc;
    FusedJob job = whole_set(h);
    job.final = d_final; job.steps = d_steps;
    return launch_fused(h, image, 0, n_iter, outeredge, job);
}

// Pass 1 of every trajectory-producing run: the persistent integrator (optionally binning the
// image) with final states and step counts kept on the device, then the row offsets: records
// 0..k of a packet exist, the last one is live unless the packet died in iteration k.
int count_rows(nxc_handle *h, double step, int64_t n_iter, double outeredge, bool image,
               int64_t *lengths_out, long long *total_out)
{
    const int64_t n = h->n_packets;
    const size_t col = (size_t)n * sizeof(double);
    int rc;
    h->rows_total = -1;
    if ((rc = scratch_for(h, 8 * col))) return rc;
    if ((rc = h->d_steps.ensure((size_t)n * sizeof(long long))))
        return rc;
    if ((rc = launch_const(h, step, n_iter, outeredge, image, h->d_scratch, h->d_steps))) return rc;
    std::vector<long long> steps((size_t)n), off((size_t)n + 1);
    std::vector<double> frac((size_t)n);
    HIPCHK(hipMemcpyAsync(steps.data(), h->d_steps, (size_t)n * sizeof(long long),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(frac.data(), h->d_scratch + 7 * n, col, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    long long acc = 0;
    for (int64_t i = 0; i < n; i++) {
        off[(size_t)i] = acc;
        const long long len = steps[(size_t)i] + (frac[(size_t)i] > 0.0 ? 1 : 0);
        if (lengths_out) lengths_out[i] = len;
        acc += len;
    }
    off[(size_t)n] = acc;
    if ((rc = h->d_offsets.ensure(((size_t)n + 1) * sizeof(long long))))
        return rc;
    HIPCHK(hipMemcpyAsync(h->d_offsets, off.data(), ((size_t)n + 1) * sizeof(long long),
                          hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    // the lifetimes are now known exactly: re-sort the queue by them (longest first) for pass 2
    // and for every later pass over these packets
    if ((rc = order_on_device(h, 0.0, h->d_steps, n_iter))) return rc;
    h->rows_total = acc;
    h->rows_step = step; h->rows_edge = outeredge; h->rows_n_iter = n_iter; h->rows_n = n;
    *total_out = acc;
    return NXC_OK;
}

// Pass 2: the records themselves, rec[total][10] (doubles, or floats + int32 when narrow) in the
// handle's record scratch.  `reserve`: bytes the caller is about to allocate next to it (checked
// against free memory).
int write_records(nxc_handle *h, bool narrow, size_t reserve)
{
    int rc = need_forces(h);
    if (rc) return rc;
    if (h->rows_total < 0 || h->rows_n != h->n_packets)
        return fail(NXC_ERR_STATE, "the trajectory rows need a preceding nxc_integrate_const_rows");
    const long long total = h->rows_total;
    if (total == 0) {
        // nothing to write: the counters of "pass 2" are zeros, not a second copy of pass 1's
        HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
        return NXC_OK;
    }
    const size_t bytes = (size_t)total * 10 * (narrow ? sizeof(float) : sizeof(double));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t grow = bytes > h->d_rec.cap ? bytes : 0, back = grow ? h->d_rec.cap : 0;
    if (grow + reserve > free_b + back + pool_bytes(h))
        return fail(NXC_ERR_NOMEM, "trajectory rows do not fit in device memory; run fewer packets "
                                 "per call (the reference chunks too, Input.py:219-222)");
    if (grow > free_b + back) pool_flush(h);      // the scratch grows into what the pool holds
    // the launch groups of an Input.run differ by a per cent or so: an eighth of slack saves the
    // later ones a free + malloc of ten-odd GB each
    const size_t roomy = bytes + bytes / 8;
    const bool slack = grow && roomy + reserve <= free_b + back;
    if ((rc = h->d_rec.ensure(slack ? roomy : bytes))) return rc;
    if ((rc = const_preamble(h, h->rows_step, h->rows_n_iter))) return rc;
    FusedJob job = whole_set(h);
    job.offsets = h->d_offsets; job.rec = h->d_rec;
    return launch_fused(h, false, narrow ? 2 : 1, h->rows_n_iter, h->rows_edge, job);
}

template <typename T, typename I>
int transpose_rows(nxc_handle *h, const void *d_rec, long long total, void *d_cols, void *d_index)
{
    int64_t g = (total + NXC_TR_ROWS - 1) / NXC_TR_ROWS;
    const int64_t cap = (int64_t)h->n_cu * 16;
    if (g > cap) g = cap;
    hipLaunchKernelGGL((k_rows_transpose<T, I>), dim3((unsigned)g), dim3(NXC_TR_ROWS), 0, h->stream,
                       d_rec, total, static_cast<T *>(d_cols), static_cast<I *>(d_index));
    HIPCHK(hipGetLastError());
    return NXC_OK;
}

// A new store of `total` rows, its two blocks from the pool (a store without rows has none).
// `what`: the producer, for the report of a failed allocation, which leaves nothing behind.
int new_rows(nxc_handle *h, long long total, bool f32, nxc_rows **out, const char *what)
{
    *out = nullptr;
    nxc_rows *r = new (std::nothrow) nxc_rows();
    if (!r) return fail(NXC_ERR_ARG, "out of host memory");
    r->device = h->device; r->f32 = f32; r->total = total;
    hipError_t e = hipSuccess;
    if (total > 0) {
        const size_t vsz = f32 ? 4 : 8;          // values, and the index column beside them
        e = pool_take(h, (size_t)total * 9 * vsz, &r->d_cols, &r->cols_cap);
        if (e == hipSuccess) e = pool_take(h, (size_t)total * vsz, &r->d_index, &r->index_cap);
    }
    if (e != hipSuccess) {
        nxc_rows_free(h, r);
        return fail_hip(what, e);
    }
    *out = r;
    return NXC_OK;
}

// Passes 1 -> 2 -> columns: the device-resident row store of the run counted last.
int rows_build(nxc_handle *h, bool narrow, nxc_rows **out)
{
    *out = nullptr;
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    const long long total = h->rows_total;
    const size_t store_bytes = (size_t)(total > 0 ? total : 0) * 10 * (narrow ? 4 : 8);
    int rc = write_records(h, narrow, store_bytes);
    if (rc) return rc;
    h->rows_total = -1;
    nxc_rows *r = nullptr;
    if ((rc = new_rows(h, total, narrow, &r, "rows run"))) return rc;
    if (total > 0) {
        rc = narrow ? transpose_rows<float, int>(h, h->d_rec, total, r->d_cols, r->d_index)
                    : transpose_rows<double, long long>(h, h->d_rec, total, r->d_cols, r->d_index);
        const hipError_t e = rc ? hipSuccess : stream_sync(h);
        if (rc || e != hipSuccess) {
            nxc_rows_free(h, r);
            return rc ? rc : fail_hip("rows run", e);
        }
    }
    *out = r;
    return NXC_OK;
}

int rows_check(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (!h || !r) return fail(NXC_ERR_ARG, "null argument");
    if (r->device != h->device) return fail(NXC_ERR_ARG, "the rows live on another device");
    if (first < 0 || count < 0 || first + count > r->total)
        return fail(NXC_ERR_ARG, "row range outside the store");
    return NXC_OK;
}

// ---- sample views ------------------------------------------------------------------------------
constexpr int N_SAMPLE_COLS = 8;
constexpr int ROW_SAMPLE_COLS[N_SAMPLE_COLS] = {1, 2, 3, 5, 7, 4, 6, 0};   // the store columns of x, y, z, vy, frac, vx, vz, time

// rows [first, first + count) of a store (its index is int32 beside float32 rows, else int64)
int samples_from_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count, int64_t shift,
                      Samples *s)
{
    int rc = rows_check(h, r, first, count);
    if (rc) return rc;
    const size_t vsz = r->f32 ? 4 : 8;
    const char *c = static_cast<const char *>(r->d_cols) + (size_t)first * vsz;
    *s = Samples{};
    for (int k = 0; k < N_SAMPLE_COLS; k++) s->cols[k] = c + (size_t)ROW_SAMPLE_COLS[k] * r->total * vsz;
    s->index = static_cast<const char *>(r->d_index) + (size_t)first * vsz;
    s->f32 = r->f32; s->index64 = !r->f32; s->n = count; s->shift = shift;
    s->store = r; s->col0 = c; s->stride = r->total;
    return NXC_OK;
}

// P samples in host memory, 64-bit or as save() keeps them (32-bit), to the device buffer *buf:
// each column (null ones are skipped) 256-byte aligned, then the int64 index if there is one
template <typename T>
int samples_upload(nxc_handle *h, Dev<unsigned char> &buf, int64_t P,
                   const T *const cols[N_SAMPLE_COLS], const int64_t *index, Samples *s)
{
    const size_t bytes = (size_t)P * sizeof(T), col = (bytes + 255) & ~size_t(255);
    const size_t n_cols = N_SAMPLE_COLS - std::count(cols, cols + N_SAMPLE_COLS, nullptr);
    int rc = buf.ensure(n_cols * col + (index ? (size_t)P * 8 : 0));
    if (rc) return rc;
    *s = Samples{};
    s->f32 = sizeof(T) == 4; s->n = P;
    unsigned char *d = buf;
    for (int c = 0; c < N_SAMPLE_COLS; c++) {
        if (!cols[c]) continue;
        if (P) HIPCHK(hipMemcpyAsync(d, cols[c], bytes, hipMemcpyHostToDevice, h->stream));
        s->cols[c] = d;
        d += col;
    }
    if (index && P) HIPCHK(hipMemcpyAsync(d, index, (size_t)P * 8, hipMemcpyHostToDevice, h->stream));
    s->index = index ? d : nullptr;
    return NXC_OK;
}

// Calls f(T(), I()) with the value and index types of s: (double, long long), (float, int) for
// float32 stores or (float, long long) for float32 host columns -- the only instantiations
template <typename Fn>
int with_sample_types(const Samples &s, Fn &&f)
{
    if (!s.f32) return f(double(), (long long)0);
    if (s.index64) return f(float(), (long long)0);
    return f(float(), int());
}

// nxc_rows_fetch / nxc_rows_fetch_f32: build, copy out, free
int rows_fetch(nxc_handle *h, void *rows_out, bool narrow)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (h->rows_total < 0 || h->rows_n != h->n_packets)
        return fail(NXC_ERR_STATE, "nxc_rows_fetch needs a preceding nxc_integrate_const_rows");
    if (h->rows_total > 0 && !rows_out) return fail(NXC_ERR_ARG, "rows_out is null");
    nxc_rows *r = nullptr;
    int rc = rows_build(h, narrow, &r);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (r->total > 0) {
        e = hipMemcpyAsync(rows_out, r->d_cols, (size_t)r->total * 9 * (narrow ? 4 : 8),
                           hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = stream_sync(h);
    }
    nxc_rows_free(h, r);
    if (e != hipSuccess) return fail_hip("rows copy", e);
    return NXC_OK;
}

// records of the handle's line-of-sight profile
size_t los_profile_records(const nxc_handle *h) { return (size_t)h->los_prof_S * (size_t)(h->los_profK.nv + 2); }

// The pass constants and the LDS blob [header space | g-value tables] of a line-of-sight
// descriptor (los_run, fit_radiance)
int los_tables(nxc_handle *h, const nxc_los_desc *d, LosK &K, std::vector<unsigned char> &blob)
{
    blob.assign((size_t)NXC_HEADER_BYTES, 0);
    std::memcpy(blob.data(), &h->header, sizeof(LdsHeader));      // nxc_log's table lives there
    K.sin_dphi = d->sin_dphi;
    K.sin_2dphi = d->sin_2dphi;
    K.cos_thr = d->cos_threshold;
    K.cos_thr2_lo = d->cos_threshold * d->cos_threshold * (1.0 - 1e-9);
    K.vrplanet = d->vrplanet;
    K.unit_cm2 = d->unit_cm * d->unit_cm;
    K.t0 = d->ladder[0];
    K.log1p_s_inv = 1.0 / std::log1p(d->sin_dphi);
    K.n_lines = d->n_lines;
    K.n_ladder = (int)d->n_ladder;
    K.tan_dphi = std::tan(d->dphi);
    for (int l = 0; l < d->n_lines; l++) {
        // a run's Outputs share their g-value tables (one aplanet): the packed form of the last
        // call's tables is kept (packing places every cell by bisection: 0.5 ms a table, which for
        // the 125 Outputs of an Input.run(1e7) was a third of LOSResult's time)
        const size_t nb = (size_t)d->line_n[l] * sizeof(double);
        LosLutCache &c = h->los_lut[l];
        const bool same = c.n == d->line_n[l] && d->line_n[l] > 0 && c.v.size() * sizeof(double) == nb &&
                          std::memcmp(c.v.data(), d->line_v[l], nb) == 0 &&
                          std::memcmp(c.g.data(), d->line_g[l], nb) == 0;
        if (!same) {
            c.n = 0;
            int rc = pack_lut(d->line_v[l], d->line_g[l], d->line_n[l], c.lut, "g-value table");
            if (rc) return rc;
            c.v.assign(d->line_v[l], d->line_v[l] + d->line_n[l]);
            c.g.assign(d->line_g[l], d->line_g[l] + d->line_n[l]);
            c.n = d->line_n[l];
        }
        K.line[l] = placed_lut(c.lut.desc, blob.size());
        blob.insert(blob.end(), c.lut.bytes.begin(), c.lut.bytes.end());
    }
    return NXC_OK;
}

// f-1 over stored samples that are already on the device (64-bit, or 32-bit as save() keeps them)
// LOS_PROFILE: the pass of nxc_los_profile_accumulate*, which also adds to the handle's line-of-sight
// profile (dvx, dvz: the two columns only it reads); LOS_AGES: the pass of nxc_los_ages_accumulate*,
// which also adds to the handle's line-of-sight ages (dtime: the column only it reads); the plain
// pass launches what it always did
template <LosMode MODE, typename T, typename I>
int los_run(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc, int64_t P,
            const T *dx, const T *dy, const T *dz, const T *dvy, const T *dfrac, const T *dvx,
            const T *dvz, const T *dtime, const I *d_index,
            int64_t index_shift, int64_t n_index, double *radiance, int64_t *npackets, uint8_t *included,
            int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    // LDS block: [header space | g-value tables | spectra tile]
    std::vector<unsigned char> blob;
    LosK K{};
    int rc = los_tables(h, d, K, blob);
    if (rc) return rc;
    K.index_shift = index_shift;
    // block culling measures distances along the boresights: they must be unit vectors (the
    // reference's are); anything else switches the culling off, never the exact pair test
    K.cull = (d->dphi > 0 && d->dphi < 1.5 && std::isfinite(K.tan_dphi)) ? 1 : 0;
    for (int64_t i = 0; i < S && K.cull; i++) {
        const double b2 = sc[3 * S + i] * sc[3 * S + i] + sc[4 * S + i] * sc[4 * S + i] +
                          sc[5 * S + i] * sc[5 * S + i];
        if (!(std::fabs(b2 - 1.0) <= 1e-9)) K.cull = 0;
    }
    const size_t stage_bytes = blob.size();
    K.tile_off = (int64_t)((stage_bytes + 31) & ~size_t(31));
    // ... | per-wave candidate queues
    // all the spectra of a launch in LDS, 512 at a time -- fewer when the g-value tables are large
    // (four lines of 389 points: 66 KB) and leave less room beside the per-wave lists
    const size_t lds_rest = (size_t)K.tile_off + (size_t)(NXC_LOS_THREADS / 64) * NXC_LOS_WAVE_BYTES + 32;
    K.tile_cap = NXC_LOS_TILE;
    while (K.tile_cap > 32 && lds_rest + (size_t)K.tile_cap * NXC_LOS_SP * sizeof(double) > 160 * 1024)
        K.tile_cap >>= 1;
    const size_t lds = lds_rest + (size_t)K.tile_cap * NXC_LOS_SP * sizeof(double);   // (+ trip counter, counter sums)
    if (lds > 160 * 1024) return fail(NXC_ERR_ARG, "g-value tables exceed the LDS");

    // device scratch: blob | sc | ladder | radiance | npackets | included | used
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    const size_t o_blob = take(stage_bytes), o_sc = take((size_t)8 * S * 8),
                 o_lad = take((size_t)d->n_ladder * 8),
                 o_rad = take((size_t)S * 8), o_np = take((size_t)S * 8),
                 o_inc = take(included ? (size_t)n_index : 0),
                 o_used = take(used_pairs ? (size_t)used_cap * 16 : 0), o_nu = take(8);
    if ((rc = scratch_for(h, off))) return rc;
    unsigned char *base = reinterpret_cast<unsigned char *>(h->d_scratch.get());
    // the used pairs go to the host copy (used_pairs) or stay on the device (nxc_los_set_pairs)
    nxc_pairs *const sink = used_pairs ? nullptr : h->los_pairs;
    long long *const d_used = used_pairs ? reinterpret_cast<long long *>(base + o_used)
                                         : sink ? sink->d : nullptr;
    const long long cap_used = used_pairs ? (long long)used_cap : sink ? sink->cap : 0;
    if (sink) sink->n = 0;
    hipStream_t st = h->stream;
    HIPCHK(hipMemcpyAsync(base + o_blob, blob.data(), stage_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(base + o_sc, sc, (size_t)8 * S * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(base + o_lad, d->ladder, (size_t)d->n_ladder * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(base + o_rad, 0, (size_t)S * 8, st));
    HIPCHK(hipMemsetAsync(base + o_np, 0, (size_t)S * 8, st));
    if (included) HIPCHK(hipMemsetAsync(base + o_inc, 0, (size_t)n_index, st));
    HIPCHK(hipMemsetAsync(base + o_nu, 0, 8, st));
    HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), st));
    if (P > 0) {
        if ((rc = prep_kernel(k_los<T, I, MODE>, lds))) return rc;
        const int tiles = (int)((S + K.tile_cap - 1) / K.tile_cap);
        constexpr int WPG = NXC_LOS_THREADS / 64;                  // waves per workgroup of k_los
        // the samples go through in slabs: the block scratch is sized for the worst case of one
        // slot per row (40 bytes; the bench cloud uses a fifth of a slot per row)
        int64_t slab = std::min<int64_t>(P, int64_t(1) << 24);
        if (const char *t = std::getenv("NXC_TEST_LOS_SLAB_ROWS"))       // tests: several slabs at small sizes
            slab = std::max<int64_t>(256, std::min<int64_t>(slab, std::atoll(t)));
        // (every region may add 7 empty slots to complete its last group)
        const int64_t max_regions = (slab + NXC_LOS_FORM - 1) / NXC_LOS_FORM;
        const size_t max_slots = (size_t)(slab + 8 * max_regions);
        const size_t o_desc = 0, o_sph = (max_slots * 8 + 255) & ~size_t(255),
                     o_n = o_sph + max_slots * 32;
        // the list of (row, spectrum) pairs near a cone: chunks of 64 (k_los -> k_los_pairs); when
        // it is full k_los decides the pairs itself
        constexpr int pair_cap = 1 << 15;
        int pair_chunks = pair_cap;             // (the scratch is laid out for pair_cap whatever this says)
        if (const char *t = std::getenv("NXC_TEST_LOS_PAIR_CHUNKS"))     // tests: a full list at small sizes
            pair_chunks = (int)std::max<long long>(1, std::min<long long>(pair_cap, std::atoll(t)));
        const size_t o_fill = o_n + 256, o_list = o_fill + (size_t)pair_cap * 4;
        if ((rc = h->d_losblk.ensure(o_list + (size_t)pair_cap * 64 * 8)))
            return rc;
        size_t lds_pairs = ((stage_bytes + 31) & ~size_t(31)) + (size_t)((d->n_ladder + 3) & ~int64_t(3)) * 8;
        if (lds_pairs > 160 * 1024) return fail(NXC_ERR_ARG, "the ladder of ball centres exceeds the LDS");
        // the per-spectrum sums of a workgroup in LDS when they leave room for two workgroups per CU
        // (a profile pass: radiance, count and the four moment sums; an ages pass has no sums of
        // its own)
        const size_t sums_bytes = (size_t)S * (MODE == LOS_PROFILE ? 48 : 16);
        const int lds_sums = lds_pairs + sums_bytes <= 80 * 1024 ? 1 : 0;
        if (lds_sums) lds_pairs += sums_bytes;
        if ((rc = prep_kernel(k_los_pairs<T, I, MODE>, lds_pairs))) return rc;
        LosProf<T, MODE> prof{};
        if constexpr (MODE == LOS_PROFILE) {
            prof.bins = h->los_profK;
            prof.rec = h->d_los_prof;
            prof.mom = h->d_los_prof + los_profile_records(h) * 2;
        }
        if constexpr (MODE == LOS_AGES) {
            prof.bins = h->los_ages.K;
            prof.rec = h->los_ages.d;
        }
        unsigned *pair_used = reinterpret_cast<unsigned *>(h->d_losblk + o_n + 8);
        unsigned *pair_fill = reinterpret_cast<unsigned *>(h->d_losblk + o_fill);
        unsigned long long *pair_list = reinterpret_cast<unsigned long long *>(h->d_losblk + o_list);
        unsigned long long *bdesc = reinterpret_cast<unsigned long long *>(h->d_losblk + o_desc);
        double *bsph = reinterpret_cast<double *>(h->d_losblk + o_sph);
        unsigned long long *n_slots = reinterpret_cast<unsigned long long *>(h->d_losblk + o_n);
        if ((rc = begin_timed(h))) return rc;
        for (int64_t first = 0; first < P; first += slab) {
            const int64_t n = std::min<int64_t>(slab, P - first);
            const int64_t regions = (n + NXC_LOS_FORM - 1) / NXC_LOS_FORM;
            K.row_base = first;
            if constexpr (MODE == LOS_PROFILE) { prof.vx = dvx + first; prof.vz = dvz + first; }
            if constexpr (MODE == LOS_AGES) prof.time = dtime + first;
            HIPCHK(hipMemsetAsync(n_slots, 0, 256 + (size_t)pair_cap * 4, st));   // counters + chunk fills
            hipLaunchKernelGGL((k_los_blocks<T, I>),
                               dim3((unsigned)((regions + NXC_LOS_BLOCKS_THREADS / 64 - 1) /
                                               (NXC_LOS_BLOCKS_THREADS / 64))),
                               dim3(NXC_LOS_BLOCKS_THREADS), 0, st, n, K.cull, dx + first, dy + first, dz + first,
                               d_index ? d_index + first : d_index, bdesc, bsph, n_slots);
            HIPCHK(hipGetLastError());
            // persistent waves, one workgroup per CU (its LDS holds all the spectra of a tile)
            const int64_t groups = std::max<int64_t>(1, std::min<int64_t>(h->n_cu, (n / 8 / 64 + WPG) / WPG));
            hipLaunchKernelGGL((k_los<T, I, MODE>), dim3((unsigned)groups, tiles),
                               dim3(NXC_LOS_THREADS), lds, st, K, base + o_blob,
                               (int64_t)stage_bytes, S, reinterpret_cast<const double *>(base + o_sc),
                               n_slots, bdesc, bsph, pair_list, pair_fill, pair_used, pair_chunks,
                               dx + first, dy + first, dz + first, dvy + first, dfrac + first,
                               d_index ? d_index + first : d_index,
                               reinterpret_cast<const double *>(base + o_lad),
                               reinterpret_cast<double *>(base + o_rad),
                               reinterpret_cast<unsigned long long *>(base + o_np),
                               included ? base + o_inc : nullptr, cap_used, d_used,
                               reinterpret_cast<unsigned long long *>(base + o_nu), h->d_ctr, prof);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL((k_los_pairs<T, I, MODE>), dim3((unsigned)(h->n_cu * 2)), dim3(NXC_BLOCK),
                               lds_pairs, st, K, base + o_blob, (int64_t)stage_bytes, S,
                               reinterpret_cast<const double *>(base + o_sc), pair_list, pair_fill,
                               pair_used, pair_chunks, lds_sums, dx + first, dy + first, dz + first,
                               dvy + first, dfrac + first, d_index ? d_index + first : d_index,
                               reinterpret_cast<const double *>(base + o_lad),
                               reinterpret_cast<double *>(base + o_rad),
                               reinterpret_cast<unsigned long long *>(base + o_np),
                               included ? base + o_inc : nullptr, cap_used, d_used,
                               reinterpret_cast<unsigned long long *>(base + o_nu), h->d_ctr, prof);
            HIPCHK(hipGetLastError());
        }
        if ((rc = end_timed(h))) return rc;
    }
    HIPCHK(hipMemcpyAsync(radiance, base + o_rad, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(npackets, base + o_np, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    if (included) HIPCHK(hipMemcpyAsync(included, base + o_inc, (size_t)n_index, hipMemcpyDeviceToHost, st));
    unsigned long long nu = 0;
    HIPCHK(hipMemcpyAsync(&nu, base + o_nu, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_used) *n_used = (int64_t)nu;
    if (sink) {
        sink->n = (long long)std::min<unsigned long long>(nu, (unsigned long long)sink->cap);
        if (nu > (unsigned long long)sink->cap)
            return fail(NXC_ERR_OVERFLOW, "the pair list holds " + std::to_string(sink->cap) + " pairs, the pass found " +
                                              std::to_string(nu));
    }
    if (used_pairs) {
        const size_t got = (size_t)std::min<unsigned long long>(nu, (unsigned long long)used_cap);
        HIPCHK(hipMemcpy(used_pairs, base + o_used, got * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(used_pairs + used_cap, base + o_used + (size_t)used_cap * 8, got * 8,
                         hipMemcpyDeviceToHost));
    }
    return NXC_OK;
}

int los_check(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc, int64_t P,
              const double *radiance, const int64_t *npackets, const uint8_t *included,
              int64_t n_index, int64_t used_cap, const int64_t *used_pairs, const int64_t *n_used)
{
    if (!h || !d || S < 1 || P < 0 || !sc || !radiance || !npackets)
        return fail(NXC_ERR_ARG, "bad arguments");
    if (d->n_lines < 0 || d->n_lines > NXC_MAX_LINES || d->n_ladder < 1 || !d->ladder)
        return fail(NXC_ERR_ARG, "bad nxc_los_desc");
    if (included && n_index < 1) return fail(NXC_ERR_ARG, "included needs n_index");
    if (used_pairs && (used_cap < 1 || !n_used)) return fail(NXC_ERR_ARG, "used_pairs needs a capacity");
    if (used_pairs && h->los_pairs) return fail(NXC_ERR_ARG, "used_pairs with a device pair list set");
    HIPCHK(hipSetDevice(h->device));
    return NXC_OK;
}

// ... over a sample view
template <LosMode MODE>
int los_run(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc, const Samples &s,
            int64_t n_index, double *radiance, int64_t *npackets, uint8_t *included, int64_t used_cap,
            int64_t *used_pairs, int64_t *n_used)
{
    return with_sample_types(s, [&](auto t, auto i) {
        using T = decltype(t);
        return los_run<MODE>(h, d, S, sc, s.n, s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(3),
                             s.col<T>(4), s.col<T>(5), s.col<T>(6), s.col<T>(7), s.idx<decltype(i)>(),
                             s.shift, n_index, radiance, npackets, included, used_cap, used_pairs, n_used);
    });
}

// What a profile entry checks in front of the plain entry's own checks
int los_profile_check(const nxc_handle *h, int64_t S)
{
    if (!h) return fail(NXC_ERR_ARG, "bad arguments");
    if (!h->have_los_prof) return fail(NXC_ERR_STATE, "nxc_los_profile_enable has not been called");
    if (S != h->los_prof_S)
        return fail(NXC_ERR_ARG, "the profile was enabled for " + std::to_string(h->los_prof_S) +
                                     " spectra, this call has " + std::to_string(S));
    return NXC_OK;
}

// What an ages entry checks in front of the plain entry's own checks
constexpr const char *LOS_AGES_UNSET = "nxc_los_ages_enable has not been called";
int los_ages_check(const nxc_handle *h, int64_t S)
{
    if (!h) return fail(NXC_ERR_ARG, "bad arguments");
    if (!h->los_ages.have) return fail(NXC_ERR_STATE, LOS_AGES_UNSET);
    if (S != h->los_ages.records)
        return fail(NXC_ERR_ARG, "the ages were enabled for " + std::to_string(h->los_ages.records) +
                                     " spectra, this call has " + std::to_string(S));
    return NXC_OK;
}

// ... over samples in host memory: five columns, seven for a profile pass, six for an ages pass
// (+ the index column) go to the device first
template <LosMode MODE, typename T>
int los_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc, int64_t P,
                   const T *x, const T *y, const T *z, const T *vx, const T *vy, const T *vz,
                   const T *frac, const T *time, const int64_t *index, int64_t n_index,
                   double *radiance, int64_t *npackets, uint8_t *included, int64_t used_cap,
                   int64_t *used_pairs, int64_t *n_used)
{
    int rc = MODE == LOS_PROFILE ? los_profile_check(h, S) : MODE == LOS_AGES ? los_ages_check(h, S) : NXC_OK;
    if (rc) return rc;
    rc = los_check(h, d, S, sc, P, radiance, npackets, included, n_index, used_cap, used_pairs, n_used);
    if (rc) return rc;
    if (P && (!x || !y || !z || !vy || !frac)) return fail(NXC_ERR_ARG, "bad arguments");
    if (MODE == LOS_PROFILE && P && (!vx || !vz)) return fail(NXC_ERR_ARG, "bad arguments");
    if (MODE == LOS_AGES && P && !time) return fail(NXC_ERR_ARG, "bad arguments");
    const T *cols[N_SAMPLE_COLS] = {x, y, z, vy, frac, vx, vz, time};
    Samples s;
    if ((rc = samples_upload(h, h->d_samples, P, cols, index, &s))) return rc;
    return los_run<MODE>(h, d, S, sc, s, n_index, radiance, npackets, included, used_cap, used_pairs,
                         n_used);
}

// nxc_los_profile_enable: S (nv + 2) zeroed records and S x 4 moment sums in one block, or none; the
// arguments are checked (check_los_profile_args) before the profile there is is touched
int los_profile_enable(nxc_handle *h, int64_t S, int64_t nv, double v_lo, double v_hi)
{
    if (!h) return fail(NXC_ERR_ARG, "bad arguments");
    if (nv != 0) {
        const std::string why = check_los_profile_args(S, nv, v_lo, v_hi);
        if (!why.empty()) return fail(NXC_ERR_ARG, why.c_str());
    }
    HIPCHK(hipSetDevice(h->device));
    h->have_los_prof = false;
    int rc = h->d_los_prof.release();
    if (rc || nv == 0) return rc;
    h->los_prof_S = S;
    h->los_profK = CubeK{(int)nv, v_lo, cube_inv_dv(nv, v_lo, v_hi)};
    const size_t bytes = (los_profile_records(h) * 2 + (size_t)S * 4) * sizeof(double);
    if ((rc = h->d_los_prof.ensure(bytes))) return rc;
    HIPCHK(hipMemsetAsync(h->d_los_prof, 0, bytes, h->stream));
    HIPCHK(stream_sync(h));
    h->have_los_prof = true;
    return NXC_OK;
}

// nxc_los_profile_download: sums[S][nv + 2][2] and moments[S][4], the device's own order
int los_profile_download(nxc_handle *h, double *sums, double *moments)
{
    if (!h) return fail(NXC_ERR_ARG, "bad arguments");
    if (!h->have_los_prof) return fail(NXC_ERR_STATE, "nxc_los_profile_enable has not been called");
    if (!sums || !moments) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const size_t n_rec = los_profile_records(h) * 2;
    HIPCHK(hipMemcpyAsync(sums, h->d_los_prof, n_rec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(moments, h->d_los_prof + n_rec, (size_t)h->los_prof_S * 4 * sizeof(double),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

// The plan of the tiled image for this handle's image and mode (nxc_tile_plan.hpp).
bool tile_plan(const nxc_handle *h, TilePlan *out)
{
    return tile_plan(h->header.G.nx, h->header.G.nz, h->tile_pixels, h->img_bytes, out);
}

// a-6..a-8 over samples on the device, through LDS-privatised tiles (nxc_kernels.hpp: k_image_bin,
// k_image_tiles).  The samples go through in slabs so that the chunk scratch stays bounded
// (10 bytes per sample of a slab at worst: every sample inside the image).
template <typename T, bool DEFER, int CAP>
int image_run_tiles(nxc_handle *h, const TilePlan &tp, int64_t p, const T *dx, const T *dy,
                    const T *dz, const T *dvy, const T *dfrac)
{
    int rc, per_cu = 0;
    // pass 2 forms the weights (DEFER): the image tables sit in front of its tile
    const size_t tables = DEFER ? nxc_tile_tables(h->img_bytes) : 0;
    const size_t lds_tiles = tables + (size_t)NXC_TILE_PIXELS * 12;
    if ((rc = prep_kernel(k_image_bin<T, DEFER, CAP>, tp.lds_bin))) return rc;
    if ((rc = prep_kernel(k_image_tiles<DEFER, CAP>, lds_tiles))) return rc;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_image_bin<T, DEFER, CAP>,
                                                        NXC_TILE_BIN_BLOCK, tp.lds_bin));
    const int nb = 1 << tp.nb_log2;
    const int ng = std::max(1, h->n_cu / nb);             // consumer groups per tile
    const int64_t slots = (int64_t)h->n_cu * (per_cu > 0 ? per_cu : 1);
    int64_t slab_max = h->tile_slab;
    TileSlabs ts;
    for (;;) {
        ts = tile_slabs(tp, p, slab_max, slots, sizeof(T));
        rc = h->d_tiles.ensure(ts.bytes);
        if (rc == NXC_OK) break;
        if (ts.slab <= (int64_t(1) << 22)) return rc;     // HBM is full: not even 50 MB
        (void)hipGetLastError();
        slab_max = ts.slab >> 1;                          // a smaller slab needs less scratch
    }
    const int64_t slab = ts.slab, span = ts.span, mc = ts.mc;
    const size_t o_sl = ts.o_sl, o_list = ts.o_list, o_n = ts.o_n;
    double *sw = reinterpret_cast<double *>(h->d_tiles.get());
    unsigned short *sl = reinterpret_cast<unsigned short *>(h->d_tiles + o_sl);
    unsigned short *list = reinterpret_cast<unsigned short *>(h->d_tiles + o_list);
    unsigned *nlist = reinterpret_cast<unsigned *>(h->d_tiles + o_n);
    if ((rc = begin_timed(h))) return rc;
    for (int64_t first = 0; first < p; first += slab) {
        const int64_t n = std::min<int64_t>(slab, p - first);
        const int64_t grid = (n + span - 1) / span;       // <= prod; the scratch regions keep their place
        hipLaunchKernelGGL((k_image_bin<T, DEFER, CAP>), dim3((unsigned)grid), dim3(NXC_TILE_BIN_BLOCK),
                           tp.lds_bin, h->stream, h->d_blob_img, (int64_t)h->img_bytes, n, span,
                           (int)mc, tp.nb_log2, dx + first, dy + first, dz + first, dvy + first,
                           dfrac + first, sw, sl, list, nlist, h->d_ctr);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((k_image_tiles<DEFER, CAP>), dim3((unsigned)(nb * ng)), dim3(NXC_IMAGE_BLOCK),
                           lds_tiles, h->stream, h->d_blob_img, (int64_t)h->img_bytes, (int)grid,
                           (int)mc, tp.nb_log2, ng, tp.tile_used, (int)h->header.G.nz, sw, sl, list,
                           nlist, h->img.image, h->d_ctr);
        HIPCHK(hipGetLastError());
    }
    if ((rc = end_timed(h))) return rc;
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

// An occupancy-sized, grid-stride pass over p stored samples: as many workgroups as the chip holds
// at once (never more than the samples fill), each striding over the samples; timed and waited for.
// (The arguments come by reference: the handle's buffers turn into pointers at the kernel's own
// parameters.)
template <class K, class... Args>
int launch_sample_pass(nxc_handle *h, K kernel, int block, size_t lds_bytes, int64_t p,
                       const Args &...args)
{
    int per_cu = 0, rc;
    if ((rc = prep_kernel(kernel, lds_bytes))) return rc;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds_bytes));
    int64_t grid = (int64_t)h->n_cu * (per_cu > 0 ? per_cu : 1);
    grid = std::max<int64_t>(1, std::min<int64_t>(grid, (p + block - 1) / block));
    if ((rc = begin_timed(h))) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds_bytes, h->stream, args...);
    HIPCHK(hipGetLastError());
    if ((rc = end_timed(h))) return rc;
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

// a-6..a-8 over samples on the device
int image_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        const int64_t p = s.n;
        const T *dx = s.col<T>(0), *dy = s.col<T>(1), *dz = s.col<T>(2), *dvy = s.col<T>(3),
                *dfrac = s.col<T>(4);
        TilePlan tp;
        const bool fits = tile_plan(h, &tp);
        if (h->image_mode == 2 && !fits)
            return fail(NXC_ERR_ARG, "this image does not fit the tiled path (too many pixels)");
        if (fits && (h->image_mode == 2 || (h->image_mode == 0 && p >= NXC_TILE_MIN_SAMPLES))) {
            // float32 samples (stored rows, the down-cast image) leave the weight to pass 2 when the
            // image tables fit a CU's LDS next to a tile
            const bool f32_values = sizeof(T) == 4 || h->header.G.downcast_f32 != 0;
            const bool defer = f32_values && nxc_tile_room(h->img_bytes);
#define NXC_TILES_CASE(C)                                                                       \
            case C:                                                                             \
                return defer ? image_run_tiles<T, true, C>(h, tp, p, dx, dy, dz, dvy, dfrac)    \
                             : image_run_tiles<T, false, C>(h, tp, p, dx, dy, dz, dvy, dfrac);
            switch (tp.cap) {
                NXC_TILES_CASE(256)
                NXC_TILES_CASE(128)
                NXC_TILES_CASE(64)
            default:
                return fail(NXC_ERR_STATE, "tile plan with an unknown chunk size");
            }
#undef NXC_TILES_CASE
        }
        // as many 1024-thread groups as fit a CU (two for Na's 45 KB of tables), each staging the
        // tables once and striding over the samples
        return launch_sample_pass(h, k_image<T>, NXC_IMAGE_BLOCK, h->img_bytes, p, h->d_blob_img,
                                  (int64_t)h->img_bytes, p, dx, dy, dz, dvy, dfrac, h->img.image, h->d_ctr);
    });
}

// ModelDensity over samples on the device (k_density; vy is not read)
int density_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_density<T>, NXC_BLOCK, 0, s.n, h->dens, s.n, s.col<T>(0),
                                  s.col<T>(1), s.col<T>(2), s.col<T>(4), h->d_dens_pts,
                                  h->d_dens_cell, h->d_dens_acc);
    });
}

// ModelDensity(moments=True) over samples on the device (k_density_moments)
int moments_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_density_moments<T>, NXC_BLOCK, 0, s.n, h->dens, s.n, h->dens_q,
                                  s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3),
                                  s.col<T>(6), s.col<T>(4), h->d_dens_pts, h->d_dens_cell,
                                  h->d_dens_acc, h->d_dens_mom);
    });
}

// ModelDensity(spectrum=...) over samples on the device (k_density_spectrum)
int spectrum_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_density_spectrum<T>, NXC_BLOCK, 0, s.n, h->dens, h->dens_spec,
                                  s.n, h->dens_q, s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5),
                                  s.col<T>(3), s.col<T>(6), s.col<T>(4), h->d_dens_pts,
                                  h->d_dens_cell, h->d_dens_frames, h->d_dens_acc, h->d_dens_spec);
    });
}

// ModelDensity(ages=...) over samples on the device (k_density_ages: time, x, y, z, frac)
int density_ages_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_density_ages<T>, NXC_BLOCK, 0, s.n, h->dens, h->dens_ages.K, s.n,
                                  s.col<T>(7), s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(4),
                                  h->d_dens_pts, h->d_dens_cell, h->d_dens_acc, h->dens_ages.d);
    });
}

// CameraImage over samples on the device (k_camera)
int camera_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_camera<T>, NXC_CAMERA_BLOCK, h->cam_bytes, s.n, h->cam,
                                  h->d_blob_cam, (int64_t)h->cam_bytes, s.n, s.col<T>(0), s.col<T>(1),
                                  s.col<T>(2), s.col<T>(3), s.col<T>(4), h->cam_px.image, h->d_ctr);
    });
}

// ShellMap over samples on the device (k_shell)
int shell_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_shell<T>, NXC_SHELL_BLOCK, h->shell_bytes, s.n, h->shell,
                                  h->d_blob_shell, (int64_t)h->shell_bytes, s.n, s.col<T>(0),
                                  s.col<T>(1), s.col<T>(2), s.col<T>(3), s.col<T>(4),
                                  h->shell_px.image, h->d_shell_planes, h->d_ctr);
    });
}

// ShellMap(moments=True) over samples on the device (k_shell_moments)
int shell_moments_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_shell_moments<T>, NXC_SHELL_BLOCK, h->shell_bytes, s.n, h->shell,
                                  h->d_blob_shell, (int64_t)h->shell_bytes, s.n, s.col<T>(0),
                                  s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3), s.col<T>(6),
                                  s.col<T>(4), h->shell_px.image, h->d_shell_planes, h->d_shell_mom,
                                  h->d_ctr);
    });
}

// ShellMap(ages=...) over samples on the device (k_shell_ages: time, x, y, z, vy, frac)
int shell_ages_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_shell_ages<T>, NXC_SHELL_BLOCK, h->shell_bytes, s.n, h->shell,
                                  h->shell_ages.K, h->d_blob_shell, (int64_t)h->shell_bytes, s.n,
                                  s.col<T>(7), s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(3),
                                  s.col<T>(4), h->shell_px.image, h->d_shell_planes, h->shell_ages.d,
                                  h->d_ctr);
    });
}

// ModelImage(moments=True) over samples on the device (k_image_moments: atomics, never the tiles)
int image_moments_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_image_moments<T>, NXC_IMAGE_MOMENTS_BLOCK, h->img_bytes, s.n,
                                  h->d_blob_img, (int64_t)h->img_bytes, s.n, (int64_t)h->img.npix,
                                  s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3),
                                  s.col<T>(6), s.col<T>(4), h->img.image, h->img.mom, h->d_ctr);
    });
}

// CameraImage(moments=True) over samples on the device (k_camera_moments)
int camera_moments_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_camera_moments<T>, NXC_CAMERA_BLOCK, h->cam_bytes, s.n, h->cam,
                                  h->d_blob_cam, (int64_t)h->cam_bytes, s.n, (int64_t)h->cam_px.npix,
                                  s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3),
                                  s.col<T>(6), s.col<T>(4), h->cam_px.image, h->cam_px.mom, h->d_ctr);
    });
}

// ModelImage(cube=...) over samples on the device (k_image_cube: atomics, never the tiles)
int image_cube_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_image_cube<T>, NXC_IMAGE_MOMENTS_BLOCK, h->img_bytes, s.n,
                                  h->d_blob_img, (int64_t)h->img_bytes, s.n, h->img.cubeK,
                                  s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3),
                                  s.col<T>(6), s.col<T>(4), h->img.image, h->img.cube, h->d_ctr);
    });
}

// CameraImage(cube=...) over samples on the device (k_camera_cube)
int camera_cube_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_camera_cube<T>, NXC_CAMERA_BLOCK, h->cam_bytes, s.n, h->cam,
                                  h->d_blob_cam, (int64_t)h->cam_bytes, s.n, h->cam_px.cubeK,
                                  s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(5), s.col<T>(3),
                                  s.col<T>(6), s.col<T>(4), h->cam_px.image, h->cam_px.cube, h->d_ctr);
    });
}

// ModelImage(ages=...) over samples on the device (k_image_ages: atomics, never the tiles)
int image_ages_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_image_ages<T>, NXC_IMAGE_MOMENTS_BLOCK, h->img_bytes, s.n,
                                  h->d_blob_img, (int64_t)h->img_bytes, s.n, h->img.ages.K,
                                  s.col<T>(7), s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(3),
                                  s.col<T>(4), h->img.image, h->img.ages.d, h->d_ctr);
    });
}

// CameraImage(ages=...) over samples on the device (k_camera_ages)
int camera_ages_run(nxc_handle *h, const Samples &s)
{
    return with_sample_types(s, [&](auto t, auto) -> int {
        using T = decltype(t);
        return launch_sample_pass(h, k_camera_ages<T>, NXC_CAMERA_BLOCK, h->cam_bytes, s.n, h->cam,
                                  h->d_blob_cam, (int64_t)h->cam_bytes, s.n, h->cam_px.ages.K,
                                  s.col<T>(7), s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(3),
                                  s.col<T>(4), h->cam_px.image, h->cam_px.ages.d, h->d_ctr);
    });
}

// What tells one consumer of stored samples from another at its entry points
struct SampleConsumer {
    bool (*have)(const nxc_handle *);            // its nxc_*_set has been called ...
    const char *unset;                           // ... or this is the NXC_ERR_STATE message
    bool needs_vy, clears_ctr;                   // reads the vy column; zeroes d_ctr per accepted call
    bool needs_vxz;                              // reads the vx and vz columns too
    bool (*idle)(const nxc_handle *);            // nothing to add to, whatever the samples (or null)
    int (*run)(nxc_handle *, const Samples &);
    PixelSums nxc_handle::*px = nullptr;         // the pixel sums its moments and cube sit beside
    bool needs_time = false;                     // reads the time column (host entries: an eighth array)
};
const SampleConsumer IMAGE_SAMPLES = {[](const nxc_handle *h) { return h->have_image; },
                                      "nxc_set_image has not been called",
                                      true, true, false, nullptr, image_run, &nxc_handle::img};
const SampleConsumer DENSITY_SAMPLES = {[](const nxc_handle *h) { return h->have_density; },
                                        "nxc_density_set has not been called",
                                        false, false, false,
                                        [](const nxc_handle *h) { return h->dens_q == 0; }, density_run};
// the moments' state is the enable; its entries check nxc_density_set's first (moments_need_set)
const SampleConsumer MOMENT_SAMPLES = {[](const nxc_handle *h) { return h->have_dens_mom; },
                                       "nxc_density_moments_enable has not been called",
                                       true, false, true,
                                       [](const nxc_handle *h) { return h->dens_q == 0; }, moments_run};
// the state check that comes in front of MOMENT_SAMPLES' and SPECTRUM_SAMPLES': nxc_density_set is
// the missing call
int moments_need_set(const nxc_handle *h)
{
    if (h && h->have_density) return NXC_OK;
    return guarded([&]() -> int { return fail(NXC_ERR_STATE, DENSITY_SAMPLES.unset); });
}
// the spectrum's state is its enable too, checked after nxc_density_set's (moments_need_set)
const SampleConsumer SPECTRUM_SAMPLES = {[](const nxc_handle *h) { return h->have_dens_spec; },
                                         "nxc_density_spectrum_enable has not been called",
                                         true, false, true,
                                         [](const nxc_handle *h) { return h->dens_q == 0; }, spectrum_run};
// bytes of the two planes of a spectrum over Q points
size_t spectrum_bytes(size_t Q, const SpectrumK &S) { return 2 * Q * (size_t)(S.nv + 2) * 2 * sizeof(double); }

// the spectrum off, its records and frame records back to the device
int spectrum_free(nxc_handle *h)
{
    h->have_dens_spec = false;
    const int rc = h->d_dens_spec.release(), rc2 = h->d_dens_frames.release();
    return rc ? rc : rc2;
}
// the density ages' state is their enable too, checked after nxc_density_set's (moments_need_set);
// the pass reads the time column and no velocity
const SampleConsumer DENSITY_AGES_SAMPLES = {[](const nxc_handle *h) { return h->dens_ages.have; },
                                             "nxc_density_ages_enable has not been called",
                                             false, false, false,
                                             [](const nxc_handle *h) { return h->dens_q == 0; },
                                             density_ages_run, nullptr, true};
const SampleConsumer CAMERA_SAMPLES = {[](const nxc_handle *h) { return h->have_camera; },
                                       "nxc_camera_set has not been called",
                                       true, true, false, nullptr, camera_run, &nxc_handle::cam_px};
const SampleConsumer SHELL_SAMPLES = {[](const nxc_handle *h) { return h->have_shell; },
                                      "nxc_shell_set has not been called",
                                      true, true, false, nullptr, shell_run, &nxc_handle::shell_px};
// the shell moments' state is their enable, checked after nxc_shell_set's (shell_moments_state,
// check_shell_moments_ready)
const SampleConsumer SHELL_MOMENT_SAMPLES = {[](const nxc_handle *h) { return h->have_shell_mom; },
                                             NXC_SHELL_MOMENTS_UNSET,
                                             true, true, true, nullptr, shell_moments_run};
ShellMomentsState shell_moments_state(const nxc_handle *h)
{
    if (!h) return {false, false, false, 0};
    return {true, h->have_shell, h->have_shell_mom, h->shell.plane};
}
// the state checks in front of SHELL_MOMENT_SAMPLES' entries: the set is named first
int shell_moments_ready(const nxc_handle *h)
{
    const ShellMomentsRefusal r = check_shell_moments_ready(shell_moments_state(h));
    if (r.code == NXC_OK) return NXC_OK;
    return guarded([&]() -> int { return fail(r.code, r.why); });
}
// the shell ages' state is their enable too, checked after nxc_shell_set's (pixel_moments_need_set);
// the pass reads the time column and neither vx nor vz
const SampleConsumer SHELL_AGES_SAMPLES = {[](const nxc_handle *h) { return h->shell_ages.have; },
                                           "nxc_shell_ages_enable has not been called",
                                           true, true, false, nullptr, shell_ages_run, nullptr, true};
// records of one plane of the shell map: cells (nalt + 2)
int64_t shell_records(const nxc_handle *h) { return h->shell.plane / 2; }

// the pixel moments' state is their enable, checked after the set's (pixel_moments_need_set)
const SampleConsumer IMAGE_MOMENT_SAMPLES = {[](const nxc_handle *h) { return h->img.have_mom; },
                                             "nxc_image_moments_enable has not been called",
                                             true, true, true, nullptr, image_moments_run};
const SampleConsumer CAMERA_MOMENT_SAMPLES = {[](const nxc_handle *h) { return h->cam_px.have_mom; },
                                              "nxc_camera_moments_enable has not been called",
                                              true, true, true, nullptr, camera_moments_run};
// the state check in front of a moments consumer's own: the set of `base` is the missing call
int pixel_moments_need_set(const nxc_handle *h, const SampleConsumer &base)
{
    if (h && base.have(h)) return NXC_OK;
    return guarded([&]() -> int { return fail(NXC_ERR_STATE, base.unset); });
}

// nxc_X_moments_enable: [2][npix] zeroed records beside the image pair of `base`, or none
int pixel_moments_enable(nxc_handle *h, const SampleConsumer &base, int on)
{
    if (int rc = pixel_moments_need_set(h, base)) return rc;
    return guarded([&]() -> int {
        PixelSums &px = h->*base.px;
        HIPCHK(hipSetDevice(h->device));
        px.have_mom = false;
        int rc = px.mom.release();
        if (rc || !on) return rc;
        const size_t bytes = px.npix * 4 * sizeof(double);
        if ((rc = px.mom.ensure(bytes))) return rc;
        HIPCHK(hipMemsetAsync(px.mom, 0, bytes, h->stream));
        HIPCHK(stream_sync(h));
        px.have_mom = true;
        return NXC_OK;
    });
}

// nxc_X_moments_download: sums[npix][4] = m1 m2 m3 ww from the two planes
int pixel_moments_download(nxc_handle *h, const SampleConsumer &base, const SampleConsumer &mom,
                           double *sums)
{
    if (int rc = pixel_moments_need_set(h, base)) return rc;
    return guarded([&]() -> int {
        if (!mom.have(h)) return fail(NXC_ERR_STATE, mom.unset);
        if (!sums) return fail(NXC_ERR_ARG, "bad arguments");
        HIPCHK(hipSetDevice(h->device));
        const size_t npix = (h->*base.px).npix;
        std::vector<double> planes(npix * 4);
        HIPCHK(hipMemcpyAsync(planes.data(), (h->*base.px).mom, planes.size() * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
        HIPCHK(stream_sync(h));
        for (size_t q = 0; q < npix; q++)
            for (size_t k = 0; k < 2; k++) {
                sums[4 * q + 2 * k] = planes[2 * (k * npix + q)];
                sums[4 * q + 2 * k + 1] = planes[2 * (k * npix + q) + 1];
            }
        return NXC_OK;
    });
}

// the velocity cube's state is its enable too, checked after the set's (pixel_moments_need_set)
const SampleConsumer IMAGE_CUBE_SAMPLES = {[](const nxc_handle *h) { return h->img.have_cube; },
                                           "nxc_image_cube_enable has not been called",
                                           true, true, true, nullptr, image_cube_run};
const SampleConsumer CAMERA_CUBE_SAMPLES = {[](const nxc_handle *h) { return h->cam_px.have_cube; },
                                            "nxc_camera_cube_enable has not been called",
                                            true, true, true, nullptr, camera_cube_run};

size_t cube_bytes(size_t npix, const CubeK &Q) { return npix * (size_t)(Q.nv + 2) * 2 * sizeof(double); }

// nxc_X_cube_enable: [npix][nv + 2] zeroed records beside the image pair of `base`, or none; the
// arguments are checked (check_cube_args) before the cube there is is touched
int pixel_cube_enable(nxc_handle *h, const SampleConsumer &base, int64_t nv, double v_lo, double v_hi)
{
    if (int rc = pixel_moments_need_set(h, base)) return rc;
    return guarded([&]() -> int {
        PixelSums &px = h->*base.px;
        if (nv != 0) {
            const std::string why = check_cube_args((int64_t)px.npix, nv, v_lo, v_hi);
            if (!why.empty()) return fail(NXC_ERR_ARG, why.c_str());
        }
        HIPCHK(hipSetDevice(h->device));
        px.have_cube = false;
        int rc = px.cube.release();
        if (rc || nv == 0) return rc;
        px.cubeK = CubeK{(int)nv, v_lo, cube_inv_dv(nv, v_lo, v_hi)};
        const size_t bytes = cube_bytes(px.npix, px.cubeK);
        if ((rc = px.cube.ensure(bytes))) return rc;
        HIPCHK(hipMemsetAsync(px.cube, 0, bytes, h->stream));
        HIPCHK(stream_sync(h));
        px.have_cube = true;
        return NXC_OK;
    });
}

// nxc_X_cube_download: sums[npix][nv + 2][2], the device's own order
int pixel_cube_download(nxc_handle *h, const SampleConsumer &base, const SampleConsumer &cube,
                        double *sums)
{
    if (int rc = pixel_moments_need_set(h, base)) return rc;
    return guarded([&]() -> int {
        if (!cube.have(h)) return fail(NXC_ERR_STATE, cube.unset);
        if (!sums) return fail(NXC_ERR_ARG, "bad arguments");
        HIPCHK(hipSetDevice(h->device));
        const PixelSums &px = h->*base.px;
        HIPCHK(hipMemcpyAsync(sums, px.cube, cube_bytes(px.npix, px.cubeK), hipMemcpyDeviceToHost,
                              h->stream));
        HIPCHK(stream_sync(h));
        return NXC_OK;
    });
}

// the age block's state is its enable too, checked after the set's (pixel_moments_need_set); its
// passes read the time column and neither vx nor vz
const SampleConsumer IMAGE_AGES_SAMPLES = {[](const nxc_handle *h) { return h->img.ages.have; },
                                           "nxc_image_ages_enable has not been called",
                                           true, true, false, nullptr, image_ages_run, nullptr, true};
const SampleConsumer CAMERA_AGES_SAMPLES = {[](const nxc_handle *h) { return h->cam_px.ages.have; },
                                            "nxc_camera_ages_enable has not been called",
                                            true, true, false, nullptr, camera_ages_run, nullptr, true};

// Who owns an age block, for the entries that enable, copy and contract it (ages_*)
struct AgesOwner {
    AgeBlock &(*block)(nxc_handle *);
    const SampleConsumer *base;      // its "has not been called" comes first; null (the lines of
                                     // sight): no set to wait for, and a null handle is NXC_ERR_ARG
    const char *unset;               // the ages consumer's "has not been called"
    const AgesSubject &subject;      // the words of the enable's refusals
    int64_t (*records)(const nxc_handle *);     // records per set; null: the enable's argument S
    int sets;
    bool out_first;                  // the apply refuses a null `out` before it looks at K
};
const AgesOwner IMAGE_AGES = {[](nxc_handle *h) -> AgeBlock & { return h->img.ages; }, &IMAGE_SAMPLES,
                              IMAGE_AGES_SAMPLES.unset, AGES_OF_PIXELS,
                              [](const nxc_handle *h) { return (int64_t)h->img.npix; }, 1, false};
const AgesOwner CAMERA_AGES = {[](nxc_handle *h) -> AgeBlock & { return h->cam_px.ages; },
                               &CAMERA_SAMPLES, CAMERA_AGES_SAMPLES.unset, AGES_OF_PIXELS,
                               [](const nxc_handle *h) { return (int64_t)h->cam_px.npix; }, 1, false};
const AgesOwner DENSITY_AGES = {[](nxc_handle *h) -> AgeBlock & { return h->dens_ages; },
                                &DENSITY_SAMPLES, DENSITY_AGES_SAMPLES.unset, AGES_OF_POINTS,
                                [](const nxc_handle *h) { return h->dens_q; }, 1, true};
const AgesOwner SHELL_AGES = {[](nxc_handle *h) -> AgeBlock & { return h->shell_ages; }, &SHELL_SAMPLES,
                              SHELL_AGES_SAMPLES.unset, AGES_OF_SHELLS, shell_records,
                              NXC_SHELL_AGE_PLANES, true};
const AgesOwner LOS_AGES_BLOCK = {[](nxc_handle *h) -> AgeBlock & { return h->los_ages; }, nullptr,
                                  LOS_AGES_UNSET, AGES_OF_SPECTRA, nullptr, 1, false};

// the state check every entry of an owner starts with: its set is the missing call
int ages_need_set(const nxc_handle *h, const AgesOwner &o)
{
    if (!o.base) return h ? NXC_OK : fail(NXC_ERR_ARG, "bad arguments");
    if (!h || !o.base->have(h)) return fail(NXC_ERR_STATE, o.base->unset);
    return NXC_OK;
}

// ... and the download, the upload and the apply go on with: the enable is
int ages_need_enable(nxc_handle *h, const AgesOwner &o)
{
    if (int rc = ages_need_set(h, o)) return rc;
    if (!o.block(h).have) return fail(NXC_ERR_STATE, o.unset);
    return NXC_OK;
}

// nxc_X_ages_enable: sets x records x (na + 2) zeroed records, or none (na == 0); the arguments are
// checked (check_ages_args) before the block there is is touched
int ages_enable(nxc_handle *h, const AgesOwner &o, int64_t S, int64_t na, double t0, double a_lo,
                double a_hi)
{
    return guarded([&]() -> int {
        if (int rc = ages_need_set(h, o)) return rc;
        const int64_t records = o.records ? o.records(h) : S;
        if (na != 0) {
            const std::string why = check_ages_args(o.subject, records, na, t0, a_lo, a_hi);
            if (!why.empty()) return fail(NXC_ERR_ARG, why.c_str());
        }
        HIPCHK(hipSetDevice(h->device));
        AgeBlock &b = o.block(h);
        int rc = b.release();
        if (rc || na == 0) return rc;
        b.K = AgeK{(int)na, t0, a_lo, ages_inv_da(na, a_lo, a_hi)};
        b.records = records;
        b.sets = o.sets;
        const size_t bytes = b.bytes();
        if ((rc = b.d.ensure(bytes))) return rc;
        HIPCHK(hipMemsetAsync(b.d, 0, bytes, h->stream));
        HIPCHK(stream_sync(h));
        b.have = true;
        return NXC_OK;
    });
}

// nxc_X_ages_download: sums[sets][records][na + 2][2], the device's own order; nxc_X_ages_upload:
// the block replaced by such sums (totals added on the host)
int ages_copy(nxc_handle *h, const AgesOwner &o, double *sums, hipMemcpyKind kind)
{
    return guarded([&]() -> int {
        if (int rc = ages_need_enable(h, o)) return rc;
        if (!sums) return fail(NXC_ERR_ARG, "bad arguments");
        HIPCHK(hipSetDevice(h->device));
        AgeBlock &b = o.block(h);
        const bool down = kind == hipMemcpyDeviceToHost;
        HIPCHK(hipMemcpyAsync(down ? sums : b.d.get(), down ? b.d.get() : sums, b.bytes(), kind,
                              h->stream));
        HIPCHK(stream_sync(h));
        return NXC_OK;
    });
}

// out[ne][n_rec][2] (host) = a resident block of n_rec records of `planes` planes contracted with
// K[planes][ne] (host), k_ages_apply over record runs x epoch chunks cut to the device's LDS
// (ages_apply_plan).  Called inside guarded(), after the state checks of the entry.
int ages_block_apply(nxc_handle *h, size_t n_rec, int64_t planes, const double *d_block, int64_t ne,
                     const double *K, double *out)
{
    const std::string why = check_ages_apply(planes, ne, K);
    if (!why.empty()) return fail(NXC_ERR_ARG, why.c_str());
    if (!out) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    int lds_per_block = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    AgesPlan plan;
    if (!ages_apply_plan(planes, ne, (size_t)std::max(lds_per_block, 0), &plan))
        return fail(NXC_ERR_ARG, "age cube: one pixel's planes and one column of K exceed the "
                                 "LDS of a workgroup");
    const int64_t runs = ((int64_t)n_rec + plan.run - 1) / plan.run;
    const int64_t chunks = (ne + plan.chunk - 1) / plan.chunk;
    if (chunks > NXC_AGES_MAX_CHUNKS)
        return fail(NXC_ERR_ARG, "age cube: more than 65535 epoch chunks in one call");
    const size_t k_bytes = (size_t)planes * (size_t)ne * sizeof(double);
    const size_t out_bytes = (size_t)ne * n_rec * 2 * sizeof(double);
    Dev<double> d_K, d_out;
    int rc;
    if ((rc = d_K.ensure(k_bytes)) || (rc = d_out.ensure(out_bytes))) return rc;
    HIPCHK(hipMemcpyAsync(d_K, K, k_bytes, hipMemcpyHostToDevice, h->stream));
    const AgesApplyK A = {(int)planes, (int)plan.stride, (int)plan.run, (int)plan.chunk, (int)ne,
                          (int64_t)n_rec};
    if ((rc = prep_kernel(k_ages_apply, plan.bytes)) || (rc = begin_timed(h))) return rc;
    hipLaunchKernelGGL(k_ages_apply, dim3((unsigned)runs, (unsigned)chunks), dim3(NXC_AGES_APPLY_BLOCK),
                       plan.bytes, h->stream, A, reinterpret_cast<const double2 *>(d_block),
                       d_K.get(), reinterpret_cast<double2 *>(d_out.get()));
    HIPCHK(hipGetLastError());
    if ((rc = end_timed(h))) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

// nxc_X_ages_apply: out[sets][ne][records][2] (host) = each set of the resident block contracted
// with K[na + 2][ne] (host) (ages_block_apply), the shell map's plane A first
int ages_apply(nxc_handle *h, const AgesOwner &o, int64_t ne, const double *K, double *out)
{
    return guarded([&]() -> int {
        if (int rc = ages_need_enable(h, o)) return rc;
        if (o.out_first && !out) return fail(NXC_ERR_ARG, "bad arguments");
        const AgeBlock &b = o.block(h);
        const size_t R = (size_t)b.records;
        const int64_t planes = (int64_t)b.K.na + 2;
        for (size_t set = 0; set < (size_t)b.sets; set++)
            if (int rc = ages_block_apply(h, R, planes, b.d.get() + set * R * (size_t)planes * 2, ne, K,
                                          out + set * (size_t)ne * R * 2))
                return rc;
        return NXC_OK;
    });
}

// What every accepted call does, samples or none
int begin_sample_pass(nxc_handle *h, const SampleConsumer &c)
{
    HIPCHK(hipSetDevice(h->device));
    if (c.clears_ctr) HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
    return NXC_OK;
}

// nxc_X_accumulate / nxc_X_accumulate_f32: samples in host memory, 64-bit or as save() keeps them
// (32-bit), go to the handle's staging buffer first
template <typename T>
int accumulate_columns(nxc_handle *h, const SampleConsumer &c, int64_t p, const T *x, const T *y,
                       const T *z, const T *vy, const T *frac, const T *vx = nullptr,
                       const T *vz = nullptr, const T *time = nullptr)
{
    return guarded([&]() -> int {
        if (!h || !c.have(h)) return fail(NXC_ERR_STATE, c.unset);
        if (p < 0 || (p && (!x || !y || !z || (c.needs_vy && !vy) || !frac ||
                            (c.needs_vxz && (!vx || !vz)) || (c.needs_time && !time))))
            return fail(NXC_ERR_ARG, "bad arguments");
        int rc = begin_sample_pass(h, c);
        if (rc || p == 0 || (c.idle && c.idle(h))) return rc;
        const T *cols[N_SAMPLE_COLS] = {x, y, z, c.needs_vy ? vy : nullptr, frac,
                                        c.needs_vxz ? vx : nullptr, c.needs_vxz ? vz : nullptr,
                                        c.needs_time ? time : nullptr};
        Samples s;
        rc = samples_upload(h, h->d_samples, p, cols, nullptr, &s);
        return rc ? rc : c.run(h, s);
    });
}

// nxc_X_accumulate_rows: rows [first, first + count) of a store, read where they are
int accumulate_rows(nxc_handle *h, const SampleConsumer &c, const nxc_rows *r, int64_t first, int64_t count)
{
    return guarded([&]() -> int {
        if (!h || !c.have(h)) return fail(NXC_ERR_STATE, c.unset);
        Samples s;
        int rc = samples_from_rows(h, r, first, count, 0, &s);
        if (rc || (rc = begin_sample_pass(h, c)) || count == 0 || (c.idle && c.idle(h))) return rc;
        return c.run(h, s);
    });
}

// n {first, second} fp64 pairs of the device (see image_add_pairs), split into the outputs that
// are not null
template <typename T>
int download_pairs(nxc_handle *h, const double *d_pairs, size_t n, double *first, T *second)
{
    std::vector<double> both(2 * n);
    HIPCHK(hipMemcpyAsync(both.data(), d_pairs, both.size() * sizeof(double), hipMemcpyDeviceToHost,
                          h->stream));
    HIPCHK(stream_sync(h));
    for (size_t q = 0; q < n; q++) {
        if (first) first[q] = both[2 * q];
        if (second) second[q] = (T)both[2 * q + 1];         // counts: integer-valued, < 2^53
    }
    return NXC_OK;
}

// ---- LOSResultFitted -------------------------------------------------------------------------
int fit_check(nxc_handle *h, const nxc_pairs *p)
{
    if (!h || !h->have_fit) return fail(NXC_ERR_STATE, "nxc_fit_set has not been called");
    if (!h->have_fit_src) return fail(NXC_ERR_STATE, "no fit source: call nxc_fit_source*");
    if (!p || p->device != h->device || p->n < 0 || p->n > p->cap)
        return fail(NXC_ERR_ARG, "bad pair list");
    HIPCHK(hipSetDevice(h->device));
    return NXC_OK;
}

FitK fit_consts(const nxc_handle *h, const nxc_pairs *p, int64_t n_packets)
{
    FitK F{};
    F.S = h->fit_S;
    F.n_pairs = p ? p->n : 0;
    F.cap = p ? p->cap : 0;
    F.n_rows = h->fit_src.n;
    F.n_packets = n_packets;
    F.index_shift = h->fit_src.shift;
    F.mode = h->fit_mode;
    return F;
}

// device scratch of the fit's small buffers: [blob | 4 counters]
int fit_aux(nxc_handle *h, size_t blob_bytes, unsigned char **blob, unsigned long long **ctr)
{
    const size_t o_ctr = (blob_bytes + 255) & ~size_t(255);
    int rc = h->d_fit_aux.ensure(o_ctr + 256);
    if (rc) return rc;
    *blob = h->d_fit_aux;
    *ctr = reinterpret_cast<unsigned long long *>(h->d_fit_aux + o_ctr);
    return NXC_OK;
}

double *fit_pos(nxc_handle *h) { return h->d_fit_spec; }
double *fit_ratio(nxc_handle *h) { return h->d_fit_spec + 3 * h->fit_S; }
double *fit_weight(nxc_handle *h) { return h->d_fit_spec + 4 * h->fit_S; }
double *fit_rad(nxc_handle *h) { return h->d_fit_spec + 5 * h->fit_S; }
unsigned char *fit_mask(nxc_handle *h) { return reinterpret_cast<unsigned char *>(h->d_fit_spec + 6 * h->fit_S); }

// per-packet arrays of n packets: num | den | mult (f64) | cnt | lengths (u32)
double *fit_num(nxc_handle *h, int64_t n) { return reinterpret_cast<double *>(h->d_fit_pk.get()); }
double *fit_den(nxc_handle *h, int64_t n) { return fit_num(h, n) + n; }
double *fit_mult(nxc_handle *h, int64_t n) { return fit_num(h, n) + 2 * n; }
unsigned *fit_cnt(nxc_handle *h, int64_t n) { return reinterpret_cast<unsigned *>(fit_num(h, n) + 3 * n); }
unsigned *fit_len(nxc_handle *h, int64_t n) { return fit_cnt(h, n) + n; }

int64_t fit_grid(const nxc_handle *h, int64_t work, int per_cu)
{
    return std::max<int64_t>(1, std::min<int64_t>((int64_t)h->n_cu * per_cu, (work + NXC_BLOCK - 1) / NXC_BLOCK));
}

// host columns go to a buffer of their own: the source outlives the image and line-of-sight calls,
// which stage theirs in d_samples
template <typename T>
int fit_source_columns(nxc_handle *h, int64_t P, const T *x, const T *y, const T *z, const T *vy,
                       const T *frac, const int64_t *index)
{
    if (!h || !h->have_fit) return fail(NXC_ERR_STATE, "nxc_fit_set has not been called");
    if (P < 0 || (P && (!x || !y || !z || !vy || !frac || !index))) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    h->have_fit_src = false;
    h->fit_np = -1;
    const T *cols[N_SAMPLE_COLS] = {x, y, z, vy, frac, nullptr, nullptr};
    int rc = samples_upload(h, h->d_fit_smp, P, cols, index, &h->fit_src);
    h->have_fit_src = rc == NXC_OK;
    return rc;
}

template <typename T, typename I>
int fit_packets_run(nxc_handle *h, const nxc_pairs *p, int64_t n_packets, unsigned long long *ctr)
{
    const Samples &s = h->fit_src;
    const FitK F = fit_consts(h, p, n_packets);
    if (F.n_pairs > 0) {
        hipLaunchKernelGGL((k_fit_packets<T, I>), dim3((unsigned)fit_grid(h, F.n_pairs, 8)), dim3(NXC_BLOCK), 0,
                           h->stream, F, p->d, fit_pos(h), fit_ratio(h), fit_weight(h), fit_mask(h),
                           s.col<T>(0), s.col<T>(1), s.col<T>(2), s.idx<I>(),
                           fit_num(h, n_packets), fit_den(h, n_packets), fit_cnt(h, n_packets), ctr);
        HIPCHK(hipGetLastError());
    }
    return NXC_OK;
}

template <typename T, typename I>
int fit_radiance_run(nxc_handle *h, const nxc_pairs *p, const LosK &K, size_t stage_bytes,
                     const unsigned char *d_blob, unsigned long long *ctr)
{
    const Samples &s = h->fit_src;
    const FitK F = fit_consts(h, p, h->fit_np);
    if (F.n_pairs == 0) return NXC_OK;
    size_t lds = (stage_bytes + 31) & ~size_t(31);
    // the per-spectrum sums of a workgroup in LDS while they leave room for two workgroups per CU
    const int lds_sums = lds + (size_t)F.S * 8 <= 64 * 1024 ? 1 : 0;
    if (lds_sums) lds += (size_t)F.S * 8;
    int rc;
    if ((rc = prep_kernel(k_fit_radiance<T, I>, lds))) return rc;
    hipLaunchKernelGGL((k_fit_radiance<T, I>), dim3((unsigned)fit_grid(h, F.n_pairs, 2)), dim3(NXC_BLOCK), lds,
                       h->stream, K, d_blob, (int64_t)stage_bytes, F, lds_sums, p->d, fit_pos(h),
                       fit_mult(h, h->fit_np), s.col<T>(0), s.col<T>(1), s.col<T>(2), s.col<T>(3),
                       s.col<T>(4), s.idx<I>(), fit_rad(h), ctr, ctr + 1);
    HIPCHK(hipGetLastError());
    return NXC_OK;
}

// Stable compaction of n rows in tiles of NXC_BLOCK: the tiles, and the bytes of its device
// scratch [tile offsets (i64) | tile counts (u32)]
int64_t row_tiles(int64_t n) { return (n + NXC_BLOCK - 1) / NXC_BLOCK; }
size_t tile_scratch_bytes(int64_t n) { return ((size_t)row_tiles(n) * 12 + 7) & ~size_t(7); }

// The kept rows of n, in their order, in a new, finished store (`what`: its producer, for failures).
// (*count)(tile counts) launches the pass that counts every tile's kept rows; without one all n
// rows are kept.  The exclusive sums are formed here; write(tile offsets, store) launches the pass
// that places the rows, and whatever the producer wants behind it on the stream, which is waited for.
template <class Count, class Write>
int compact_rows(nxc_handle *h, int64_t n, bool f32, void *d_scratch, const Count *count, Write write,
                 nxc_rows **out, const char *what)
{
    const int64_t tiles = row_tiles(n);
    long long *tile_off = static_cast<long long *>(d_scratch), total = count ? 0 : n;
    unsigned *tile_n = reinterpret_cast<unsigned *>(tile_off + tiles);
    std::vector<long long> offs((size_t)tiles);
    for (int64_t t = 0; t < tiles; t++) offs[(size_t)t] = (long long)t * NXC_BLOCK;
    if (count && tiles) {
        std::vector<unsigned> kept((size_t)tiles);
        (*count)(tile_n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(kept.data(), tile_n, (size_t)tiles * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(stream_sync(h));
        for (int64_t t = 0; t < tiles; t++) { offs[(size_t)t] = total; total += kept[(size_t)t]; }
    }
    if (int rc = new_rows(h, total, f32, out, what)) return rc;
    hipError_t e = hipSuccess;
    if (tiles) e = hipMemcpyAsync(tile_off, offs.data(), (size_t)tiles * 8, hipMemcpyHostToDevice, h->stream);
    if (tiles && e == hipSuccess) e = write(tile_off, *out);
    if (e == hipSuccess) e = stream_sync(h);          // offs must outlive its copy; the store is final
    if (e != hipSuccess) {
        nxc_rows_free(h, *out);
        *out = nullptr;
        return fail_hip(what, e);
    }
    return NXC_OK;
}

template <typename T, typename I>
int fit_rows_run(nxc_handle *h, int compress, nxc_rows **out, int64_t *lengths_out)
{
    const Samples &s = h->fit_src;
    const int64_t n = s.n, np = h->fit_np;
    const unsigned tiles = (unsigned)row_tiles(n);
    FitK F = fit_consts(h, nullptr, np);
    F.compress = compress ? 1 : 0;
    int rc = h->d_fit_aux.ensure(tile_scratch_bytes(n));
    if (rc) return rc;
    const I *index = s.idx<I>();
    if (np) HIPCHK(hipMemsetAsync(fit_len(h, np), 0, (size_t)np * 4, h->stream));
    std::vector<unsigned> len((size_t)np);
    auto count = [&](unsigned *tile_n) {
        hipLaunchKernelGGL((k_fit_rows_count<T, I>), dim3(tiles), dim3(NXC_BLOCK), 0, h->stream, F,
                           s.col<T>(4), index, fit_mult(h, np), tile_n, fit_len(h, np));
    };
    auto write = [&](const long long *tile_off, nxc_rows *r) {
        hipLaunchKernelGGL((k_fit_rows_write<T, I>), dim3(tiles), dim3(NXC_BLOCK), 0, h->stream, F,
                           static_cast<const T *>(s.col0), s.stride, index, fit_mult(h, np), tile_off,
                           static_cast<T *>(r->d_cols), (int64_t)r->total, static_cast<I *>(r->d_index));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || !np) return e;
        return hipMemcpyAsync(len.data(), fit_len(h, np), (size_t)np * 4, hipMemcpyDeviceToHost, h->stream);
    };
    if ((rc = compact_rows(h, n, sizeof(T) == 4, h->d_fit_aux, &count, write, out, "fitted rows"))) return rc;
    if (lengths_out)
        for (int64_t i = 0; i < np; i++) lengths_out[i] = len[i];
    return NXC_OK;
}

// The adaptive-step launch over the resident packets (nxc_integrate_var and its resident form):
// finals [8][n] and stored steps [n] in the scratch, which is sized for `extra_bytes` more
// (args_ok: what the caller found of its own arguments).
int var_launch(nxc_handle *h, double resolution, double outeredge, int64_t max_steps,
               bool args_ok, size_t extra_bytes, double **d_final_out, double **d_hs_out)
{
    int rc = need_forces(h);
    if (rc) return rc;
    const int64_t n = h->n_packets;
    if (n < 1) return fail(NXC_ERR_STATE, "no resident packets (nxc_packets_upload)");
    if (!(resolution > 0) || !args_ok || max_steps < 1) return fail(NXC_ERR_ARG, "bad arguments");
    if (h->have_bodies)
        return fail(NXC_ERR_STATE, "nxc_integrate_var: moons need the constant-step driver");
    if (h->have_bounce)
        return fail(NXC_ERR_STATE, "nxc_integrate_var: surface re-emission needs the constant-step "
                                   "driver (nxc_set_bounce(h, NULL) for perfect sticking)");
    const size_t col = (size_t)n * sizeof(double);
    if ((rc = scratch_for(h, 9 * col + extra_bytes))) return rc;
    double *d_final = h->d_scratch, *d_hs = d_final + 8 * n;
    // the adaptive driver's queue: slow packets with much time left first (nxc_kernels.hpp:
    // flight_key); once per resident set
#ifdef NXC_VAR_TRACE      /* experiment: the packets as uploaded are the queue */
    if (std::getenv("NXC_TEST_VAR_NO_ORDER")) { h->have_order = false; } else
#endif
    if (h->order_key != 2 && (rc = order_on_device(h, -1.0, nullptr, 0, true))) return rc;
    HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
    const bool full = h->F.grav && h->F.rad && h->F.loss == LOSS_PHOTO;
    // Two launch forms of the same arithmetic (nxc_kernels.hpp: k_var), by packets per lane: under
    // 24 (4.7e6 packets: the launch is mostly tail) with clock-rotated wave priorities and a merged
    // tail, above it plain (highest throughput).
    const double per_lane = (double)n / ((double)h->n_cu * BLOCK_PERSIST);
    bool fair = per_lane < NXC_VAR_FAIR_PACKETS_PER_LANE;
    if (const char *t = std::getenv("NXC_TEST_VAR_VARIANT"))          // tests: both forms at any size
        fair = t[0] == 'f';                                           // "fair" / "plain"
    const auto kernel = fair ? (full ? k_var<true, true> : k_var<false, true>)
                             : (full ? k_var<true, false> : k_var<false, false>);
    const size_t lds = persist_lds(h->force_bytes);
    int grid = 1, block = BLOCK_PERSIST;
    if ((rc = prepare_persistent_launch(h, kernel, &block, lds, n, &grid))) return rc;
#ifdef NXC_VAR_ONE_WG_PER_CU          /* experiment: with -DNXC_BLOCK_PERSIST_N=512, two waves per SIMD */
    if (grid > h->n_cu) grid = h->n_cu;
#endif
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, h->stream, h->F, h->d_blob,
                       (int64_t)h->force_bytes, n, h->have_order ? h->d_queue : h->d_packets,
                       h->have_order ? h->d_order : (const unsigned *)nullptr, resolution, outeredge,
                       (long long)max_steps, d_final, d_hs, h->d_ctr);
    HIPCHK(hipGetLastError());
    if ((rc = end_timed(h))) return rc;
    *d_final_out = d_final;
    *d_hs_out = d_hs;
    return NXC_OK;
}

// Behind the finals and steps in the scratch, what nxc_var_rows_build needs of it:
// [tile scratch | kept [n] u8]
size_t var_rows_scratch(int64_t n) { return tile_scratch_bytes(n) + (size_t)n; }

template <typename T, typename I>
int var_rows_run(nxc_handle *h, int compress, nxc_rows **out, uint8_t *kept_out)
{
    const int64_t n = h->var_n;
    const unsigned tiles = (unsigned)row_tiles(n);
    const double *fin = h->d_scratch;
    unsigned char *d_tiles = reinterpret_cast<unsigned char *>(h->d_scratch + 9 * n);
    unsigned char *d_kept = d_tiles + tile_scratch_bytes(n);
    auto count = [&](unsigned *tile_n) {
        hipLaunchKernelGGL(k_var_rows_count, dim3(tiles), dim3(NXC_BLOCK), 0, h->stream, n, fin + 7 * n, tile_n);
    };
    // (nothing kept: the pass still runs, for kept_out; it writes no row)
    auto write = [&](const long long *tile_off, nxc_rows *r) {
        hipLaunchKernelGGL((k_var_rows_write<T, I>), dim3(tiles), dim3(NXC_BLOCK), 0, h->stream, n, compress,
                           fin, tile_off, static_cast<T *>(r->d_cols), (int64_t)r->total,
                           static_cast<I *>(r->d_index), d_kept);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(h->ev1, h->stream);
        if (e != hipSuccess) return e;
        h->timed = true;
        return kept_out ? hipMemcpyAsync(kept_out, d_kept, (size_t)n, hipMemcpyDeviceToHost, h->stream) : e;
    };
    if (int rc = begin_timed(h)) return rc;
    return compact_rows(h, n, sizeof(T) == 4, d_tiles, compress ? &count : nullptr, write, out, "adaptive-step rows");
}

}  // namespace

// =============================================================================================
extern "C" {

int nxc_abi_version(void) { return NXC_ABI_VERSION; }

const char *nxc_last_error_string(void) { return g_error.c_str(); }

int nxc_device_count(int *count)
{
    if (!count) return fail(NXC_ERR_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(NXC_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return NXC_OK;
}

int nxc_create(int device, nxc_handle **out)
{
    return guarded([&]() -> int {
    if (!out) return fail(NXC_ERR_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    int rc = nxc_device_count(&n);
    if (rc) return rc;
    if (n < 1) return fail(NXC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(NXC_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    nxc_handle *h = new (std::nothrow) nxc_handle();
    if (!h) return fail(NXC_ERR_ARG, "out of host memory");
    h->device = device;
    h->n_cu = prop.multiProcessorCount;
    for (int i = 0; i < NXC_LOG_BINS; i++)          // the table nxc_log reads from the LDS header
        for (int c = 0; c < 3; c++) h->header.logtab[i][c] = NXC_LOG_TABLE_DATA[i][c];
    std::snprintf(h->name, sizeof h->name, "%s (%s, %d CUs)", prop.name, prop.gcnArchName,
                  prop.multiProcessorCount);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e == hipSuccess && (h->d_ctr.ensure(sizeof(DevCounters)) || h->d_reduce.ensure(64)))
        e = HipAlloc::last;
    if (e == hipSuccess) e = hipMemset(h->d_ctr, 0, sizeof(DevCounters));
    if (e != hipSuccess) {
        nxc_destroy(h);
        return fail(NXC_ERR_HIP, std::string("nxc_create: ") + hipGetErrorString(e));
    }
    {
        std::lock_guard<std::mutex> g(g_handles_lock);
        g_handles.push_back(h);
    }
    *out = h;
    return NXC_OK;
    });
}

int nxc_destroy(nxc_handle *h)
{
    if (!h) return NXC_OK;
    {
        std::lock_guard<std::mutex> g(g_handles_lock);
        g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), h), g_handles.end());
    }
    (void)hipSetDevice(h->device);
    if (h->stream) (void)stream_sync(h);          // bounded when a collective is still in flight
    g_coll_failure.clear();
    if (h->comm && g_rccl.ok) g_rccl.CommDestroy(h->comm);
    pool_flush(h);
    // the handle's device memory goes with the handle (every buffer frees itself); the streams and
    // events are destroyed after it, so they are taken out first
    const hipStream_t stream = h->stream, copy_stream = h->copy_stream, stream2 = h->stream2;
    hipEvent_t events[3 + 33] = {h->ev0, h->ev1, h->ev_pre_coll};
    std::copy(h->ev_piece, h->ev_piece + 33, events + 3);
    delete h;
    if (copy_stream) { (void)hipStreamSynchronize(copy_stream); (void)hipStreamDestroy(copy_stream); }
    if (stream2) { (void)hipStreamSynchronize(stream2); (void)hipStreamDestroy(stream2); }
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    if (stream) (void)hipStreamDestroy(stream);
    return NXC_OK;
}

int nxc_device_name(nxc_handle *h, char *buf, int buflen)
{
    if (!h || !buf || buflen < 1) return fail(NXC_ERR_ARG, "bad arguments");
    std::snprintf(buf, (size_t)buflen, "%s", h->name);
    return NXC_OK;
}

int nxc_device_bus_id(nxc_handle *h, char *buf, int buflen)
{
    if (!h || !buf || buflen < 16) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipDeviceGetPCIBusId(buf, buflen, h->device));
    return NXC_OK;
}

int nxc_mem_info(nxc_handle *h, uint64_t *free_bytes, uint64_t *total_bytes)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    f += pool_bytes(h);          // blocks kept from freed row stores are reused or given back on demand
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return NXC_OK;
}

int nxc_synchronize(nxc_handle *h)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(stream_sync(h));
    if (h->streamed_pending) {
        // the pipelined pass is the one launch whose kernel may give up by itself (a wave that has
        // waited three seconds for the next piece of its queue): say so instead of handing over a
        // partial image as if it were the result
        h->streamed_pending = false;
        DevCounters c;
        HIPCHK(hipMemcpy(&c, h->d_ctr, sizeof c, hipMemcpyDeviceToHost));
        if (c.unfinished != 0) {
            h->n_packets = 0;                  // the queue holds a partly ordered set: upload again
            char buf[400];
            std::snprintf(buf, sizeof buf,
                          "the pipelined pass gave up waiting for its queue (%llu packets not "
                          "integrated): the ordering kernels did not run beside the persistent "
                          "kernel (a profiler serialising kernels?); image and counters are partial "
                          "-- upload with nxc_packets_upload and run nxc_integrate_const_async",
                          (unsigned long long)c.unfinished);
            return fail(NXC_ERR_INCOMPLETE, buf);
        }
    }
    return NXC_OK;
}

int nxc_set_forces(nxc_handle *h, const nxc_forces *f)
{
    return guarded([&]() -> int {
    if (!h || !f) return fail(NXC_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    PackedLut lut;
    const double zero_one[2] = {0.0, 1.0}, zeros[2] = {0.0, 0.0};
    int rc;
    // (the launch groups of an Input.run set the same forces again and again: the packed table of
    // the last call is kept when its nodes are the same)
    const double *nv = f->radpres ? f->v_tab : zero_one, *na = f->radpres ? f->a_tab : zeros;
    const size_t nn = f->radpres ? (size_t)(f->n_tab > 0 ? f->n_tab : 0) : 2;
    if (f->radpres && (f->n_tab < 2 || !f->v_tab || !f->a_tab)) return fail(NXC_ERR_ARG, "radiation table missing");
    const bool same_table = h->have_forces && h->force_v.size() == nn && !h->force_lut.bytes.empty() &&
                            std::memcmp(h->force_v.data(), nv, nn * sizeof(double)) == 0 &&
                            std::memcmp(h->force_a.data(), na, nn * sizeof(double)) == 0;
    h->force_v.assign(nv, nv + nn);
    h->force_a.assign(na, na + nn);
    // 8 cells per node: a cell then rarely holds two nodes (0.5 % of the Na table's cells against
    // 2 % at 4), so the two-row probe of lut_interp hits and the divergent walk mostly stays out
    // of the step loop; 16 measured slower again in the image kernel (LDS footprint).
    h->force_cells_per_node = 8;
#ifdef NXC_EXPERIMENT_KNOBS
    if (const char *e = std::getenv("NXC_FORCE_CELLS")) h->force_cells_per_node = std::max(2, std::atoi(e));
#endif
    if (!same_table || h->force_lut_cells != h->force_cells_per_node) {
        rc = pack_lut(h->force_v.data(), h->force_a.data(), (int64_t)h->force_v.size(), lut,
                      "nxc_forces radiation table", h->force_cells_per_node);
        if (rc) { h->have_forces = false; return rc; }
        h->force_lut = std::move(lut);
        h->force_lut_cells = h->force_cells_per_node;
    }
    h->F.GM = f->GM;
    h->F.vrplanet = f->vrplanet;
    h->F.photo = f->photo;
    h->F.inv_lifetime = f->lifetime > 0 ? 1.0 / f->lifetime : 0.0;   // np.ones(n)/lifetime
    h->F.grav = f->gravity ? 1 : 0;
    h->F.rad = f->radpres ? 1 : 0;
    h->F.loss = f->lifetime > 0 ? LOSS_LIFETIME : (f->has_photo ? LOSS_PHOTO : LOSS_NONE);
    h->have_forces = true;
    return upload_blob(h, h->have_image);
    });
}

int nxc_set_image(nxc_handle *h, const nxc_image_desc *d)
{
    return guarded([&]() -> int {
    if (!h || !d) return fail(NXC_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    if (d->nx < 1 || d->nz < 1 || d->nx > 32768 || d->nz > 32768 || !d->xedges || !d->zedges)
        return fail(NXC_ERR_ARG, "image dims/edges invalid");
    if (d->quantity != 0 && d->quantity != 1) return fail(NXC_ERR_ARG, "quantity must be 0 or 1");
    const int nl = d->quantity == 1 ? d->n_lines : 0;
    if (nl < 0 || nl > NXC_MAX_LINES) return fail(NXC_ERR_ARG, "n_lines out of range");
    if (!(d->apix_cm2 > 0)) return fail(NXC_ERR_ARG, "apix_cm2 must be positive");
    if (!std::isfinite(d->vrplanet)) return fail(NXC_ERR_ARG, "vrplanet must be finite");
    for (int64_t k = 0; k < d->nx; k++)
        if (!(d->xedges[k + 1] > d->xedges[k])) return fail(NXC_ERR_ARG, "xedges not ascending");
    for (int64_t k = 0; k < d->nz; k++)
        if (!(d->zedges[k + 1] > d->zedges[k])) return fail(NXC_ERR_ARG, "zedges not ascending");

    std::vector<unsigned char> part;
    ImageK G{};
    std::memcpy(G.M, d->M, sizeof G.M);
    G.vrplanet = d->vrplanet;
    G.apix_cm2 = d->apix_cm2;
    G.quantity = d->quantity;
    G.downcast_f32 = d->downcast_f32 ? 1 : 0;
#ifdef NXC_EXPERIMENT_KNOBS
    if (const char *dbg = std::getenv("NXC_DEBUG_IMAGE")) G.dbg = std::atoi(dbg);
#endif
    G.x_is_x = (d->M[0] == 1.0 && d->M[1] == 0.0 && d->M[2] == 0.0 && d->M[3] == 0.0 &&
                d->M[6] == 0.0) ? 1 : 0;
    PackedLut luts[NXC_MAX_LINES];
    int rc;
    if ((rc = pack_lines(nl, d->line_v, d->line_g, d->line_n, luts))) return rc;
    h->have_image = false;
    h->img.have_mom = false;
    h->img.have_cube = false;
    h->img.ages.have = false;
    h->image_block = append_image_block(part, G, d->nx, d->nz, d->xedges, d->zedges, nl, luts);
    h->image_part = std::move(part);
    h->G = G;

    const size_t npix = (size_t)d->nx * (size_t)d->nz;
    if ((rc = h->img.image.ensure(2 * npix * sizeof(double)))) return rc;
    h->img.npix = npix;
    if ((rc = upload_blob(h, true))) return rc;
    HIPCHK(hipMemsetAsync(h->img.image, 0, 2 * npix * sizeof(double), h->stream));   // nxc_image_clear
    h->have_image = true;
    return NXC_OK;
    });
}

int nxc_set_bounce(nxc_handle *h, const nxc_bounce_desc *d)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (!d) {                       // back to perfect sticking
        h->have_bounce = false;
        return NXC_OK;
    }
    if (d->nx < 8 || d->ny < 8 || !d->tx || !d->ty || !d->coef || !(d->unit_km > 0) ||
        d->accomfactor < 0 || d->accomfactor > 1 || d->stickcoef < 0 || d->stickcoef > 1)
        return fail(NXC_ERR_ARG, "bad nxc_bounce_desc");
    // the spline is evaluated only with accommodation: without it the tables may be dummies
    if (d->accomfactor != 0) {
        const std::string why = check_bicubic_spline("nxc_bounce_desc: accommodated", d->nx, d->ny, d->tx,
                                                     d->ty, d->coef, nullptr);
        if (!why.empty()) return fail(NXC_ERR_ARG, why);
    }
    const size_t ncoef = (size_t)(d->nx - 4) * (size_t)(d->ny - 4);
    const size_t total = (size_t)d->nx + (size_t)d->ny + ncoef;
    int rc = h->d_bounce.ensure(total * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h->d_bounce, d->tx, (size_t)d->nx * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_bounce + d->nx, d->ty, (size_t)d->ny * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_bounce + d->nx + d->ny, d->coef, ncoef * 8, hipMemcpyHostToDevice, h->stream));
    BounceK &B = h->header.B;
    B.GM = d->GM; B.unit_km = d->unit_km; B.accom = d->accomfactor; B.stickcoef = d->stickcoef;
    B.A0 = d->A[0]; B.A1 = d->A[1]; B.A2 = d->A[2]; B.t0 = d->t0; B.t1 = d->t1;
    B.temp_dependent = d->temp_dependent == 2 ? 2 : (d->temp_dependent ? 1 : 0); B.nx = (int)d->nx; B.ny = (int)d->ny;
    B.seed = d->seed;
    B.tx = h->d_bounce; B.ty = h->d_bounce + d->nx; B.coef = h->d_bounce + d->nx + d->ny;
    h->have_bounce = true;
    if (h->d_blob)
        HIPCHK(hipMemcpyAsync(h->d_blob + offsetof(LdsHeader, B), &h->header.B, sizeof(BounceK),
                              hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_set_stick_map(nxc_handle *h, const nxc_stick_map_desc *d)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    BounceK &B = h->header.B;
    if (d) {
        const std::string why = check_stick_map(d);
        if (!why.empty()) return fail(NXC_ERR_ARG, why);
        const int64_t nlon = d->nlon, nlat = d->nlat, ncoef = nlon * (nlat ? nlat : 1);
        const size_t total = (size_t)(nlon + nlat + ncoef);
        // (a launch that reads the previous map has ended: every launch is followed by a sync or is
        // ordered before these copies on the handle's stream)
        int rc = h->d_stick_map.ensure(total * sizeof(double));
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(h->d_stick_map, d->lon, (size_t)nlon * 8, hipMemcpyHostToDevice, h->stream));
        if (nlat)
            HIPCHK(hipMemcpyAsync(h->d_stick_map + nlon, d->lat, (size_t)nlat * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_stick_map + nlon + nlat, d->coef, (size_t)ncoef * 8, hipMemcpyHostToDevice, h->stream));
        B.mlon = h->d_stick_map; B.mlat = h->d_stick_map + nlon; B.mcoef = h->d_stick_map + nlon + nlat;
        B.mlon_n = (int)nlon; B.mlat_n = (int)nlat;
        h->have_stick_map = true;
    } else {
        B.mlon = B.mlat = B.mcoef = nullptr;
        B.mlon_n = B.mlat_n = 0;
        h->have_stick_map = false;
    }
    if (h->d_blob)
        HIPCHK(hipMemcpyAsync(h->d_blob + offsetof(LdsHeader, B), &h->header.B, sizeof(BounceK),
                              hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_set_bodies(nxc_handle *h, const nxc_bodies_desc *d)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    BodyK &K = h->header.Bd;
    K = BodyK{};
    h->have_bodies = false;
    if (d && (d->n_moons != 0 || d->chx_on)) {
        if (d->n_moons < 0 || d->n_moons > NXC_MAX_MOONS)
            return fail(NXC_ERR_ARG, "nxc_bodies_desc: n_moons must be 0..4");
        for (int m = 0; m < d->n_moons; m++) {
            if (!(d->a[m] > 0) || !(d->radius[m] >= 0) || !std::isfinite(d->gm[m]) ||
                !std::isfinite(d->omega[m]) || !std::isfinite(d->phi[m]))
                return fail(NXC_ERR_ARG, "nxc_bodies_desc: bad moon parameters");
        }
        if (d->chx_on && (!(d->chx_width > 0) || !(d->chx_height > 0) || !(d->chx_k0 >= 0) ||
                          (d->chx_omega != 0 && !(d->chx_omega * d->chx_rho0 > 0))))
            return fail(NXC_ERR_ARG, "nxc_bodies_desc: bad torus parameters");
        if (!std::isfinite(d->t0)) return fail(NXC_ERR_ARG, "nxc_bodies_desc: bad t0");
        h->bodies = *d;
        K.n_moons = d->n_moons;
        for (int m = 0; m < d->n_moons; m++) {
            K.gm[m] = d->gm[m];
            K.rad2[m] = d->radius[m] * d->radius[m];
            K.a[m] = d->a[m];
        }
        K.chx_on = d->chx_on ? 1 : 0;
        if (K.chx_on) {
            K.chx_k0 = d->chx_k0; K.chx_rho0 = d->chx_rho0;
            K.chx_inv_w = 1.0 / d->chx_width; K.chx_inv_h = 1.0 / d->chx_height;
            K.chx_vel = d->chx_omega != 0 ? 1 : 0;
            K.chx_omega = d->chx_omega;
            K.chx_inv_v0 = K.chx_vel ? 1.0 / (d->chx_omega * d->chx_rho0) : 0.0;
        }
        h->have_bodies = true;
    }
    if (h->d_blob)
        HIPCHK(hipMemcpyAsync(h->d_blob + offsetof(LdsHeader, Bd), &h->header.Bd, sizeof(BodyK),
                              hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_set_first_index(nxc_handle *h, int64_t first_index)
{
    if (!h || first_index < 0) return fail(NXC_ERR_ARG, "bad arguments");
    h->first_id = first_index;
    return NXC_OK;
}

int nxc_image_clear(nxc_handle *h)
{
    if (!h || !h->have_image) return fail(NXC_ERR_STATE, "nxc_set_image has not been called");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemsetAsync(h->img.image, 0, 2 * h->img.npix * sizeof(double), h->stream));
    if (h->img.have_mom)
        HIPCHK(hipMemsetAsync(h->img.mom, 0, 4 * h->img.npix * sizeof(double), h->stream));
    if (h->img.have_cube)
        HIPCHK(hipMemsetAsync(h->img.cube, 0, cube_bytes(h->img.npix, h->img.cubeK), h->stream));
    if (h->img.ages.have)
        HIPCHK(hipMemsetAsync(h->img.ages.d, 0, h->img.ages.bytes(), h->stream));
    return NXC_OK;
}

int nxc_image_mode(nxc_handle *h, int mode, int tile_pixels, int64_t slab_samples)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (mode < 0 || mode > 2) return fail(NXC_ERR_ARG, "mode is 0 (by size), 1 (atomics) or 2 (tiles)");
    if (tile_pixels < 0 || tile_pixels > NXC_TILE_PIXELS)
        return fail(NXC_ERR_ARG, "tile_pixels is 0 (default) or at most 8192");
    if (slab_samples < 0 || slab_samples > (int64_t(1) << 31))
        return fail(NXC_ERR_ARG, "slab_samples is 0 (default) or at most 2^31");
    h->image_mode = mode;
    h->tile_pixels = tile_pixels ? tile_pixels : NXC_TILE_PIXELS;
    h->tile_slab = slab_samples ? slab_samples : int64_t(1) << 28;
    return NXC_OK;
    });
}

int nxc_image_download(nxc_handle *h, double *image, uint64_t *counts)
{
    return guarded([&]() -> int {
    if (!h || !h->have_image) return fail(NXC_ERR_STATE, "nxc_set_image has not been called");
    HIPCHK(hipSetDevice(h->device));
    return download_pairs(h, h->img.image, h->img.npix, image, counts);
    });
}

#ifdef NXC_STAMPS
extern "C" int nxc_debug_stamps(nxc_handle *h, unsigned long long out[8])
{
    DevCounters c;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(&c, h->d_ctr, sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; k++) out[k] = c.stamp[k];
    return NXC_OK;
}
#endif

int nxc_counters_get(nxc_handle *h, nxc_counters *out)
{
    if (!h || !out) return fail(NXC_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(h->device));
    DevCounters c;
    HIPCHK(hipMemcpyAsync(&c, h->d_ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    out->particle_steps = c.particle_steps;
    out->samples = c.samples;
    out->samples_binned = c.samples_binned;
    out->nonfinite = c.nonfinite;
    out->bad_step = c.bad_step;
    out->neg_frac = c.neg_frac;
    out->unfinished = c.unfinished;
    out->wave_trips = c.wave_trips;
    return NXC_OK;
}

int nxc_last_kernel_ms(nxc_handle *h, float *ms)
{
    if (!h || !ms) return fail(NXC_ERR_ARG, "null argument");
    if (!h->timed) return fail(NXC_ERR_STATE, "no timed launch yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return NXC_OK;
}

int nxc_state(nxc_handle *h, int64_t n, const double *x, const double *y, const double *z,
              const double *vy, double *ax, double *ay, double *az, double *ioniz)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    if (n < 0 || (n && (!x || !y || !z || !vy || !ax || !ay || !az || !ioniz)))
        return fail(NXC_ERR_ARG, "bad arguments");
    if (h->have_bodies) return fail(NXC_ERR_STATE, "nxc_state: not available with moons set");
    if (n == 0) return NXC_OK;
    const size_t bytes = (size_t)n * sizeof(double);
    if ((rc = scratch_for(h, 8 * bytes)))
        return rc;
    double *d = h->d_scratch;
    const double *src[4] = {x, y, z, vy};
    for (int c = 0; c < 4; c++)
        HIPCHK(hipMemcpyAsync(d + c * n, src[c], bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = prep_kernel(k_state, h->force_bytes))) return rc;
    hipLaunchKernelGGL(k_state, dim3(flat_grid(h, n, NXC_BLOCK)), dim3(NXC_BLOCK), h->force_bytes,
                       h->stream, h->F, h->d_blob, (int64_t)h->force_bytes, n, d, d + n, d + 2 * n,
                       d + 3 * n, d + 4 * n, d + 5 * n, d + 6 * n, d + 7 * n);
    HIPCHK(hipGetLastError());
    double *dst[4] = {ax, ay, az, ioniz};
    for (int c = 0; c < 4; c++)
        HIPCHK(hipMemcpyAsync(dst[c], d + (4 + c) * n, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_rk5_step(nxc_handle *h, int64_t n, const double *soa_in, const double *hstep,
                 double *soa_out, double *delta_out)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    if (n < 0 || (n && (!soa_in || !hstep || !soa_out))) return fail(NXC_ERR_ARG, "bad arguments");
    if (h->have_bodies) return fail(NXC_ERR_STATE, "nxc_rk5_step: not available with moons set");
    if (n == 0) return NXC_OK;
    const size_t col = (size_t)n * sizeof(double);
    if ((rc = scratch_for(h, 25 * col)))
        return rc;
    double *d_in = h->d_scratch, *d_h = d_in + 8 * n, *d_out = d_h + n, *d_delta = d_out + 8 * n;
    HIPCHK(hipMemcpyAsync(d_in, soa_in, 8 * col, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_h, hstep, col, hipMemcpyHostToDevice, h->stream));
    const int grid = flat_grid(h, n, NXC_BLOCK);
    if (delta_out) {
        if ((rc = prep_kernel(k_rk5_step<true>, h->force_bytes))) return rc;
        hipLaunchKernelGGL(k_rk5_step<true>, dim3(grid), dim3(NXC_BLOCK), h->force_bytes,
                           h->stream, h->F, h->d_blob, (int64_t)h->force_bytes, n, d_in, d_h,
                           d_out, d_delta);
    } else {
        if ((rc = prep_kernel(k_rk5_step<false>, h->force_bytes))) return rc;
        hipLaunchKernelGGL(k_rk5_step<false>, dim3(grid), dim3(NXC_BLOCK), h->force_bytes,
                           h->stream, h->F, h->d_blob, (int64_t)h->force_bytes, n, d_in, d_h,
                           d_out, d_delta);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(soa_out, d_out, 8 * col, hipMemcpyDeviceToHost, h->stream));
    if (delta_out)
        HIPCHK(hipMemcpyAsync(delta_out, d_delta, 8 * col, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

// Counting sort of `n` packets (columns `stride` apart, starting at `soa`) by decreasing |v|^2, or
// by decreasing lifetime (d_lifetimes), entirely on `st`: histogram -> device scan -> scatter of
// the packets themselves into the queue out_queue[n][8] (one 64-byte record per packet) with
// out_order[n] = base + local packet index.
// scale > 0: the bin scale; scale <= 0: taken on the device from *d_max (k_speed_max ran before).
// beside_persistent: the launches may have to run next to a persistent kernel that fills every
// CU's LDS, so the histogram uses global atomics instead of LDS bins.
static int order_async(nxc_handle *h, hipStream_t st, const double *soa, int64_t stride, int64_t n,
                       const long long *d_lifetimes, double scale, unsigned long long *d_max,
                       unsigned long long *d_hist, unsigned *out_order, double *out_queue,
                       bool beside_persistent, unsigned base = 0, bool flight_key = false)
{
    const size_t hb = (size_t)NXC_ORDER_BINS * sizeof(unsigned long long);
    const int grid = flat_grid(h, n, NXC_BLOCK);
    const unsigned long long *mx = scale > 0 ? (const unsigned long long *)nullptr : d_max;
    HIPCHK(hipMemsetAsync(d_hist, 0, hb, st));
#define NXC_ORDER_LAUNCH(KERNEL, ...)                                                           \
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(NXC_BLOCK), 0, st, soa, d_lifetimes, stride, n,  \
                       scale, mx, __VA_ARGS__)
    if (d_lifetimes) NXC_ORDER_LAUNCH((k_order_hist<1, true>), d_hist);
    else if (flight_key) NXC_ORDER_LAUNCH((k_order_hist<2, true>), d_hist);
    else if (beside_persistent) NXC_ORDER_LAUNCH((k_order_hist<0, false>), d_hist);
    else NXC_ORDER_LAUNCH((k_order_hist<0, true>), d_hist);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(64), 0, st, d_hist);
    HIPCHK(hipGetLastError());
    if (d_lifetimes) NXC_ORDER_LAUNCH(k_order_scatter<1>, d_hist, out_order, base, out_queue);
    else if (flight_key) NXC_ORDER_LAUNCH(k_order_scatter<2>, d_hist, out_order, base, out_queue);
    else NXC_ORDER_LAUNCH(k_order_scatter<0>, d_hist, out_order, base, out_queue);
#undef NXC_ORDER_LAUNCH
    HIPCHK(hipGetLastError());
    return NXC_OK;
}

// Queue order of the resident packets.  k2max: upper bound of |v|^2 when the caller knows it (the
// sampler does), negative = find the largest finite |v|^2 on the device.  d_lifetimes != null:
// sort by those step counts instead (exact lifetimes from a counting pass; max_steps = their
// upper bound).
static int order_on_device(nxc_handle *h, double k2max, const long long *d_lifetimes,
                           int64_t max_steps, bool flight_key)
{
    const int64_t n = h->n_packets;
    const bool by_steps = d_lifetimes != nullptr;
    h->order_key = by_steps ? 1 : flight_key ? 2 : 0;
    if (by_steps) {
        if (n < 2 || n >= (int64_t)0xffffffffll || max_steps < 1) return NXC_OK;   // keep what there is
    } else {
        h->have_order = false;
        if (n < 2 || n >= (int64_t)0xffffffffll || k2max == 0 || std::isnan(k2max) ||
            (k2max > 0 && !std::isfinite(k2max)))
            return NXC_OK;
    }
    int rc = h->d_order.ensure((size_t)n * sizeof(unsigned));
    if (rc) return rc;
    const size_t hb = (size_t)NXC_ORDER_BINS * sizeof(unsigned long long);
    if ((rc = h->d_hist.ensure(hb + 64))) return rc;
    if ((rc = h->d_queue.ensure((size_t)8 * n * sizeof(double))))
        return rc;
    unsigned long long *d_max = h->d_hist + NXC_ORDER_BINS;
    double scale = by_steps ? (double)(NXC_ORDER_BINS - 1) / (double)max_steps
                            : (k2max > 0 ? (double)(NXC_ORDER_BINS - 1) / k2max : 0.0);
    if (!by_steps && !(k2max > 0)) {
        HIPCHK(hipMemsetAsync(d_max, 0, sizeof(unsigned long long), h->stream));
        if (flight_key)
            hipLaunchKernelGGL(k_speed_max<true>, dim3(flat_grid(h, n, NXC_BLOCK)), dim3(NXC_BLOCK), 0,
                               h->stream, (const double *)h->d_packets, n, n, d_max);
        else
            hipLaunchKernelGGL(k_speed_max<false>, dim3(flat_grid(h, n, NXC_BLOCK)), dim3(NXC_BLOCK), 0,
                               h->stream, (const double *)h->d_packets, n, n, d_max);
        HIPCHK(hipGetLastError());
    }
    h->have_order = false;
    if ((rc = order_async(h, h->stream, h->d_packets, n, n, d_lifetimes, scale, d_max, h->d_hist,
                          h->d_order, h->d_queue, false, 0, flight_key)))
        return rc;
    HIPCHK(stream_sync(h));
    h->have_order = true;
    return NXC_OK;
}

int nxc_packets_upload(nxc_handle *h, int64_t n, const double *soa0)
{
    return guarded([&]() -> int {
    if (!h || n < 0 || (n && !soa0)) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)8 * n * sizeof(double);
    int rc = h->d_packets.ensure(bytes);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpyAsync(h->d_packets, soa0, bytes, hipMemcpyHostToDevice, h->stream));
    h->n_packets = n;
    h->var_n = -1;
    h->first_id = 0;
    h->rows_total = -1;
    // Queue order for the persistent kernels (longest-lived first): counting sort of the packet
    // indices by decreasing |v|^2 on the device, bounded by the largest launch speed found there.
    if ((rc = order_on_device(h, -1.0, nullptr, 0))) return rc;
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}
int nxc_packets_upload_pieces(nxc_handle *h, int32_t n_pieces, const int64_t *counts,
                              const double *const *soa)
{
    return guarded([&]() -> int {
    if (!h || n_pieces < 1 || !counts || !soa) return fail(NXC_ERR_ARG, "bad arguments");
    int64_t n = 0;
    for (int p = 0; p < n_pieces; p++) {
        if (counts[p] < 0 || (counts[p] && !soa[p])) return fail(NXC_ERR_ARG, "bad piece");
        n += counts[p];
    }
    HIPCHK(hipSetDevice(h->device));
    int rc = h->d_packets.ensure((size_t)8 * n * sizeof(double));
    if (rc) return rc;
    // piece p's column c goes behind the same column of the pieces before it: the resident set is
    // the concatenation, without the host ever building it
    int64_t at = 0;
    for (int p = 0; p < n_pieces; p++) {
        for (int c = 0; c < 8 && counts[p]; c++)
            HIPCHK(hipMemcpyAsync(h->d_packets + c * n + at, soa[p] + c * counts[p],
                                  (size_t)counts[p] * sizeof(double), hipMemcpyHostToDevice, h->stream));
        at += counts[p];
    }
    h->n_packets = n;
    h->var_n = -1;
    h->first_id = 0;
    h->rows_total = -1;
    if ((rc = order_on_device(h, -1.0, nullptr, 0))) return rc;
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

// (what the descriptor must satisfy, where its tables go and what the launch derives from them:
// plan_source, nxc_desc_check.hpp)
int nxc_packets_sample(nxc_handle *h, const nxc_source_desc *d, int64_t n, double *soa_out)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "bad arguments");
    const SourcePlan plan = plan_source(d, n);
    if (!plan.why.empty()) return fail(NXC_ERR_ARG, plan.why);
    HIPCHK(hipSetDevice(h->device));
    const int64_t total = plan.stride, offset = plan.offset;
    const size_t bytes = (size_t)8 * total * sizeof(double);
    if (offset > 0 && (h->d_packets.cap < bytes || h->n_packets != total))
        return fail(NXC_ERR_STATE, "nxc_packets_sample: pieces of a set must start with dest_offset 0");
    int rc = h->d_packets.ensure(bytes);
    if (rc) return rc;
    if (plan.total &&
        (rc = h->d_source.ensure(plan.total * sizeof(double))))
        return rc;
    for (const TableCopy &c : plan.copy) {
        if (!c.count) continue;
        HIPCHK(hipMemcpyAsync(h->d_source + c.at, c.from, c.count * 8, hipMemcpyHostToDevice, h->stream));
        if (c.from == plan.pcg_maps.data()) HIPCHK(stream_sync(h));      // the table is the plan's
    }
    const auto table = [&](SourceTable t) { return h->d_source + plan.copy[t].at; };
    const auto rows = [&](SourceTable t) { return (int)plan.copy[t].count; };
    const bool map2d = d->spatial_type == 2;
    SourceK K{};
    K.endtime = d->endtime; K.exobase = d->exobase; K.sinlat0 = d->sinlat0; K.sinlat1 = d->sinlat1;
    K.lon0 = d->lon0; K.lon1 = d->lon1; K.vprob = d->vprob; K.vwidth = d->vwidth;
    K.unit_km = d->unit_km; K.sinalt0 = d->sinalt0; K.sinalt1 = d->sinalt1; K.az0 = d->az0;
    K.az1 = d->az1; K.random_time = d->random_time; K.speed_type = d->speed_type;
    K.angular_type = d->angular_type; K.is_planet = d->is_planet; K.seed = d->seed;
    K.first_index = d->first_index;
    K.spatial_type = d->spatial_type; K.n_speed = rows(ST_SPEED_V);
    K.map_nlon = d->spatial_type != 0 ? (int)d->map_nlon : 0;
    K.map_nlat = d->spatial_type == 1 || map2d ? (int)d->map_nlat : 0;
    if (map2d) { K.map_lon0 = d->map_lon0; K.map_s0 = d->map_s0; K.map_s1 = d->map_s1; }
    K.map_dlon = plan.map_dlon; K.map_ds = plan.map_ds; K.map_max = plan.map_max;
    K.max_trials = plan.max_trials;
    K.speed_cdf = table(ST_SPEED_CDF); K.speed_v = table(ST_SPEED_V);
    K.map = table(ST_MAP); K.map_cdf = table(ST_MAP_CDF);
    K.generator = d->generator;
    if (d->generator == 1) {
        K.pcg.state = ((u128)d->pcg_state[0] << 64) | d->pcg_state[1];
        K.pcg.row0 = d->pcg_row0;
        K.pcg.maps = reinterpret_cast<const nxc_u128 *>(table(ST_PCG));
    }
    K.stride = total; K.offset = offset;
    if (plan.law == NXC_LAW_THERMAL) {
        K.t0 = d->t0; K.t1 = d->t1;
        K.spl.tx = table(ST_TX); K.spl.ty = table(ST_TY); K.spl.coef = table(ST_COEF);
        K.spl.nx = rows(ST_TX); K.spl.ny = rows(ST_TY);
    }
    if (plan.law == NXC_LAW_NODES) {
        K.node_speed_cdf = table(ST_NODE_SPEED_CDF); K.node_speed_v = table(ST_NODE_SPEED_V);
        K.node_alt_cdf = table(ST_NODE_ALT_CDF); K.node_alt = table(ST_NODE_ALT);
        K.node_az_cdf = table(ST_NODE_AZ_CDF); K.node_az = table(ST_NODE_AZ);
        K.n_node_speed = rows(ST_NODE_SPEED_V); K.n_node_alt = rows(ST_NODE_ALT);
        K.n_node_az = rows(ST_NODE_AZ);
    }
    HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
    if ((rc = begin_timed(h))) return rc;
    const auto kernel = plan.law == NXC_LAW_NODES ? k_sample<NXC_LAW_NODES>
                        : (plan.law == NXC_LAW_THERMAL ? k_sample<NXC_LAW_THERMAL> : k_sample<NXC_LAW_PLAIN>);
    hipLaunchKernelGGL(kernel, dim3(flat_grid(h, n, NXC_BLOCK)), dim3(NXC_BLOCK), 0, h->stream, K, n,
                       h->d_packets, h->d_ctr);
    HIPCHK(hipGetLastError());
    if ((rc = end_timed(h))) return rc;
    DevCounters c;
    HIPCHK(hipMemcpyAsync(&c, h->d_ctr, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    if (c.unfinished) {
        h->n_packets = 0;            // never-accepted candidates must not pass for packets
        h->have_order = false;
        return fail(NXC_ERR_ARG, "nxc_packets_sample: " + std::to_string(c.unfinished) +
                                 " packets found no launch point in the density map (is it "
                                 "almost everywhere zero?)");
    }
    h->n_packets = total;
    h->var_n = -1;
    h->rows_total = -1;
    if (offset == 0) h->first_id = d->first_index;
    h->have_order = false;
    if (soa_out)        // this piece's eight columns
        HIPCHK(hipMemcpy2DAsync(soa_out, (size_t)n * 8, h->d_packets + offset, (size_t)total * 8,
                                (size_t)n * 8, 8, hipMemcpyDeviceToHost, h->stream));
    if (offset + n < total) {        // more pieces to come: the queue order waits for the last
        HIPCHK(stream_sync(h));
        return NXC_OK;
    }
    if ((rc = order_on_device(h, plan.k2max, nullptr, 0))) return rc;
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_integrate_const_async(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                              uint32_t flags)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    if (h->n_packets < 1) return fail(NXC_ERR_STATE, "no resident packets (nxc_packets_upload)");
    if (!(step > 0) || n_iter < 0) return fail(NXC_ERR_ARG, "step must be > 0, n_iter >= 0");
    const bool image = (flags & NXC_RUN_IMAGE) != 0;
    if (image && !h->have_image) return fail(NXC_ERR_STATE, "NXC_RUN_IMAGE without nxc_set_image");
    if ((rc = speed_order_for_const(h))) return rc;
    return launch_const(h, step, n_iter, outeredge, image, nullptr, nullptr);
    });
}

// Upload and integrate in one pipelined pass (the integrate call including the
// host-to-device copy of X0).  ONE launch of the persistent integrator starts at once and consumes
// a queue that is still being filled: the packets cross PCIe in pieces (copy stream); each piece is
// put into queue order by small kernels on a second stream (global-atomic histogram, one-wave
// scan: no host round trip and no LDS, since they run next to the persistent kernel whose block
// owns the CU's LDS) and then published (k_publish / wait_published in nxc_kernels.hpp).  The
// kernel's waves only ever wait for the first piece: a piece uploads in a fraction of the time it
// takes to integrate.  (Cutting the PASS into one launch per piece does not pipeline: a 12-wave
// workgroup keeps its CU until its last wave ends, so no CU is free for the next launch before
// the previous one is over -- measured: 62 ms against 56 for upload-then-integrate.)
int nxc_integrate_const_streamed(nxc_handle *h, int64_t n, const double *soa0, int32_t pieces,
                                 double step, int64_t n_iter, double outeredge, uint32_t flags)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    if (n < 1 || !soa0 || pieces < 1 || pieces > 32) return fail(NXC_ERR_ARG, "bad arguments (1..32 pieces)");
    if (!(step > 0) || n_iter < 0) return fail(NXC_ERR_ARG, "step must be > 0, n_iter >= 0");
    const bool image = (flags & NXC_RUN_IMAGE) != 0;
    if (image && !h->have_image) return fail(NXC_ERR_STATE, "NXC_RUN_IMAGE without nxc_set_image");
    if (n >= (int64_t)0xffffffffll) return fail(NXC_ERR_ARG, "too many packets for one resident set");
    if (h->have_bodies || h->have_bounce)
        return fail(NXC_ERR_STATE, "the streamed pass covers the plain force models; with moons or "
                                   "surface re-emission upload first (nxc_packets_upload)");
    if ((int64_t)pieces > n) pieces = (int32_t)n;
    const size_t per_piece = NXC_ORDER_BINS + 8;                    // bins, then the largest |v|^2
    if ((rc = h->d_packets.ensure((size_t)8 * n * 8))) return rc;
    if ((rc = h->d_queue.ensure((size_t)8 * n * 8))) return rc;
    if ((rc = h->d_order.ensure((size_t)n * sizeof(unsigned)))) return rc;
    if ((rc = h->d_piece_hist.ensure((32 * per_piece + 8) * sizeof(unsigned long long)))) return rc;
    for (int e = 0; e <= 32; e++)
        if (!h->ev_piece[e]) HIPCHK(hipEventCreateWithFlags(&h->ev_piece[e], hipEventDisableTiming));
    unsigned long long *d_avail = h->d_piece_hist + 32 * per_piece;
    h->n_packets = n;
    h->var_n = -1;
    h->first_id = 0;
    h->rows_total = -1;
    h->have_order = false;

    if ((rc = upload_step(h, step))) return rc;
    HIPCHK(hipMemsetAsync(h->d_ctr, 0, sizeof(DevCounters), h->stream));
    HIPCHK(hipMemsetAsync(d_avail, 0, sizeof(unsigned long long), h->stream));
    // everything queued on the handle's stream so far (image clear, tables, the zeroed word) first
    HIPCHK(hipEventRecord(h->ev_piece[32], h->stream));
    HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_piece[32], 0));
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->ev_piece[32], 0));
    FusedJob job;
    job.soa = h->d_queue; job.order = h->d_order; job.avail = d_avail;
    if ((rc = launch_fused(h, image, 0, n_iter, outeredge, job))) return rc;
    // from here on the kernel is waiting for pieces: whatever happens, something must be published
    auto give_up = [&](int code) {
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, h->stream2, d_avail, ~0ull);
        (void)hipStreamSynchronize(h->stream2);
        (void)stream_sync(h);
        h->n_packets = 0;
        return code;
    };
    // piece boundaries: a small first piece (enough to occupy every lane a few times over) lets
    // the integrator start after a fraction of a millisecond of copying; the rest in equal parts
    std::vector<int64_t> bound((size_t)pieces + 1, n);
    bound[0] = 0;
    if (pieces > 1) {
        int64_t first = std::max<int64_t>(n / (4 * (int64_t)pieces), (int64_t)h->n_cu * BLOCK_PERSIST * 2);
        first = std::min(first, n / pieces);
        for (int p = 1; p < pieces; p++) bound[(size_t)p] = first + (n - first) * (p - 1) / (pieces - 1);
    }
    // fault injection for the tests of the give-up path: the last piece is never published
    const bool withhold = std::getenv("NXC_TEST_WITHHOLD_LAST_PIECE") != nullptr;
    for (int p = 0; p < pieces; p++) {
        const int64_t p0 = bound[(size_t)p], len = bound[(size_t)p + 1] - p0;
        if (len <= 0) continue;
        if (withhold && p == pieces - 1 && pieces > 1) break;
        hipError_t e = hipSuccess;
        for (int c = 0; c < 8 && e == hipSuccess; c++)
            e = hipMemcpyAsync(h->d_packets + c * n + p0, soa0 + c * n + p0, (size_t)len * 8,
                               hipMemcpyHostToDevice, h->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(h->ev_piece[p], h->copy_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream2, h->ev_piece[p], 0);
        unsigned long long *hist = h->d_piece_hist + (size_t)p * per_piece, *d_max = hist + NXC_ORDER_BINS;
        if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, sizeof(unsigned long long), h->stream2);
        if (e != hipSuccess)
            return give_up(fail_hip("streamed upload", e));
        hipLaunchKernelGGL(k_speed_max<false>, dim3(flat_grid(h, len, NXC_BLOCK)), dim3(NXC_BLOCK), 0,
                           h->stream2, (const double *)(h->d_packets + p0), n, len, d_max);
        if ((rc = order_async(h, h->stream2, h->d_packets + p0, n, len, nullptr, 0.0, d_max, hist,
                              h->d_order + p0, h->d_queue + 8 * p0, true, (unsigned)p0)))
            return give_up(rc);
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, h->stream2, d_avail,
                           (unsigned long long)(p0 + len));
        if (hipGetLastError() != hipSuccess) return give_up(fail(NXC_ERR_HIP, "streamed upload: launch failed"));
    }
    h->have_order = true;            // pieces sorted one by one: still a valid queue order
    h->order_key = 0;
    h->streamed_pending = true;
    // the handle's stream continues after the ordering stream as well
    HIPCHK(hipEventRecord(h->ev_piece[32], h->stream2));
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_piece[32], 0));
    return NXC_OK;
    });
}

int nxc_integrate_const(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                        uint32_t flags, double *traj_out, int64_t nrec, double *final_out,
                        int64_t *steps_out)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    const int64_t n = h->n_packets;
    if (n < 1) return fail(NXC_ERR_STATE, "no resident packets (nxc_packets_upload)");
    if (!(step > 0) || n_iter < 0) return fail(NXC_ERR_ARG, "step must be > 0, n_iter >= 0");
    const bool image = (flags & NXC_RUN_IMAGE) != 0;
    if (image && !h->have_image) return fail(NXC_ERR_STATE, "NXC_RUN_IMAGE without nxc_set_image");
    if (traj_out && nrec < n_iter + 1) return fail(NXC_ERR_ARG, "nrec must be >= n_iter + 1");
    if ((rc = speed_order_for_const(h))) return rc;

    const size_t col = (size_t)n * sizeof(double);
    double *d_final = nullptr;
    long long *d_steps = nullptr;
    if (!traj_out) {
        if (final_out) {
            if ((rc = scratch_for(h, 8 * col)))
                return rc;
            d_final = h->d_scratch;
        }
        if (steps_out) {
            if ((rc = h->d_steps.ensure((size_t)n * sizeof(long long))))
                return rc;
            d_steps = h->d_steps;
        }
        if ((rc = launch_const(h, step, n_iter, outeredge, image, d_final, d_steps))) return rc;
    } else {
        // the dense `results` array of the reference (Output.py:376,419): pass 1 (persistent
        // integrator, + image) -> row offsets -> pass 2 writes the live records -> k_rows_densify
        // lays them out [column][record][packet] with the death record and the zero padding
        const size_t tbytes = (size_t)8 * (size_t)nrec * col;
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        if (tbytes > free_b && pool_bytes(h)) {
            pool_flush(h);
            HIPCHK(hipMemGetInfo(&free_b, &total_b));
        }
        if (tbytes > free_b)
            return fail(NXC_ERR_ARG, "trajectory buffer does not fit in device memory; run fewer "
                                     "packets per call (the reference chunks too, Input.py:219-222)");
        long long total = 0;
        if ((rc = count_rows(h, step, n_iter, outeredge, image, nullptr, &total))) return rc;
        // the caller's counters are those of pass 1 (work, samples); pass 2 re-does the steps
        DevCounters pass1;
        HIPCHK(hipMemcpyAsync(&pass1, h->d_ctr, sizeof pass1, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(stream_sync(h));
        d_final = h->d_scratch;
        d_steps = h->d_steps;
        if ((rc = write_records(h, false, tbytes))) return rc;
        h->rows_total = -1;
        const double *d_rec = static_cast<const double *>(h->d_rec.get());
        Dev<double> d_traj;
        hipError_t e = d_traj.ensure(tbytes) ? HipAlloc::last : hipSuccess;
        if (e == hipSuccess) {
            const dim3 grid((unsigned)((n + NXC_BLOCK - 1) / NXC_BLOCK),
                            (unsigned)((nrec + NXC_DENSIFY_RECORDS - 1) / NXC_DENSIFY_RECORDS));
            hipLaunchKernelGGL(k_rows_densify, grid, dim3(NXC_BLOCK), 0, h->stream, d_rec,
                               (const long long *)h->d_offsets, (const double *)d_final,
                               (const long long *)d_steps, n, nrec, d_traj.get());
            e = hipGetLastError();
        }
        DevCounters pass2;
        if (e == hipSuccess)
            e = hipMemcpyAsync(&pass2, h->d_ctr, sizeof pass2, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(traj_out, d_traj, tbytes, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = stream_sync(h);
        if (e == hipSuccess) {
            pass1.unfinished += pass2.unfinished;        // rows the two passes disagree on
            e = hipMemcpyAsync(h->d_ctr, &pass1, sizeof pass1, hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) e = stream_sync(h);
        }
        if (e != hipSuccess)
            return fail_hip("trajectory run", e);
    }
    if (final_out)
        HIPCHK(hipMemcpyAsync(final_out, d_final, 8 * col, hipMemcpyDeviceToHost, h->stream));
    if (steps_out)
        HIPCHK(hipMemcpyAsync(steps_out, d_steps, (size_t)n * sizeof(long long),
                              hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_integrate_const_rows(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                             int64_t *lengths_out, int64_t *total_out)
{
    return guarded([&]() -> int {
    int rc = need_forces(h);
    if (rc) return rc;
    if (h->n_packets < 1) return fail(NXC_ERR_STATE, "no resident packets (nxc_packets_upload)");
    if (!(step > 0) || n_iter < 0 || !total_out) return fail(NXC_ERR_ARG, "bad arguments");
    if ((rc = speed_order_for_const(h))) return rc;
    long long total = 0;
    if ((rc = count_rows(h, step, n_iter, outeredge, false, lengths_out, &total))) return rc;
    *total_out = total;
    return NXC_OK;
    });
}

int nxc_rows_build(nxc_handle *h, int narrow, nxc_rows **out)
{
    return guarded([&]() -> int {
    if (!out) return fail(NXC_ERR_ARG, "out is null");
    if (!h || h->rows_total < 0 || h->rows_n != h->n_packets)
        return fail(NXC_ERR_STATE, "nxc_rows_build needs a preceding nxc_integrate_const_rows");
    return rows_build(h, narrow != 0, out);
    });
}

int nxc_rows_info(const nxc_rows *r, int64_t *total, int32_t *is_f32)
{
    if (!r) return fail(NXC_ERR_ARG, "null argument");
    if (total) *total = r->total;
    if (is_f32) *is_f32 = r->f32 ? 1 : 0;
    return NXC_OK;
}

int nxc_rows_free(nxc_handle *h, nxc_rows *r)
{
    if (!r) return NXC_OK;
    (void)hipSetDevice(r->device);
    if (h && h->stream) (void)stream_sync(h);
    if (h && h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    if (h && h->device == r->device) {
        pool_give(h, r->d_cols, r->cols_cap);
        pool_give(h, r->d_index, r->index_cap);
    } else {
        if (r->d_cols) (void)hipFree(r->d_cols);
        if (r->d_index) (void)hipFree(r->d_index);
    }
    delete r;
    return NXC_OK;
}

int nxc_rows_download(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count,
                      void *cols_out, void *index_out)
{
    return guarded([&]() -> int {
    int rc = rows_check(h, r, first, count);
    if (rc) return rc;
    if (count == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    // a finished store is immutable (nxc_rows_build synchronises before it returns), so the copy
    // goes on its own stream and may be issued from a second host thread (a file writer) while
    // the handle's thread launches the next run
    hipStream_t st = h->copy_stream;
    const size_t vsz = r->f32 ? 4 : 8, isz = r->f32 ? 4 : 8;
    if (cols_out)          // nine strided column pieces -> [9][count]
        HIPCHK(hipMemcpy2DAsync(cols_out, (size_t)count * vsz,
                                static_cast<const char *>(r->d_cols) + (size_t)first * vsz,
                                (size_t)r->total * vsz, (size_t)count * vsz, 9,
                                hipMemcpyDeviceToHost, st));
    if (index_out)
        HIPCHK(hipMemcpyAsync(index_out, static_cast<const char *>(r->d_index) + (size_t)first * isz,
                              (size_t)count * isz, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return NXC_OK;
    });
}

int nxc_image_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    return accumulate_rows(h, IMAGE_SAMPLES, r, first, count);
}

int nxc_los_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                            const nxc_rows *r, int64_t first, int64_t count, int64_t index_shift,
                            int64_t n_index,
                            double *radiance, int64_t *npackets, uint8_t *included,
                            int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
    int rc = los_check(h, d, S, sc, count, radiance, npackets, included, n_index, used_cap,
                       used_pairs, n_used);
    if (rc) return rc;
    Samples s;
    if ((rc = samples_from_rows(h, r, first, count, index_shift, &s))) return rc;
    return los_run<LOS_PLAIN>(h, d, S, sc, s, n_index, radiance, npackets, included, used_cap,
                              used_pairs, n_used);
    });
}

int nxc_los_profile_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                    const nxc_rows *r, int64_t first, int64_t count,
                                    int64_t index_shift, int64_t n_index, double *radiance,
                                    int64_t *npackets, uint8_t *included, int64_t used_cap,
                                    int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
    int rc = los_profile_check(h, S);
    if (rc) return rc;
    rc = los_check(h, d, S, sc, count, radiance, npackets, included, n_index, used_cap, used_pairs,
                   n_used);
    if (rc) return rc;
    Samples s;
    if ((rc = samples_from_rows(h, r, first, count, index_shift, &s))) return rc;
    return los_run<LOS_PROFILE>(h, d, S, sc, s, n_index, radiance, npackets, included, used_cap,
                                used_pairs, n_used);
    });
}

int nxc_los_ages_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                 const nxc_rows *r, int64_t first, int64_t count,
                                 int64_t index_shift, int64_t n_index, double *radiance,
                                 int64_t *npackets, uint8_t *included, int64_t used_cap,
                                 int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
    int rc = los_ages_check(h, S);
    if (rc) return rc;
    rc = los_check(h, d, S, sc, count, radiance, npackets, included, n_index, used_cap, used_pairs,
                   n_used);
    if (rc) return rc;
    Samples s;
    if ((rc = samples_from_rows(h, r, first, count, index_shift, &s))) return rc;
    return los_run<LOS_AGES>(h, d, S, sc, s, n_index, radiance, npackets, included, used_cap,
                             used_pairs, n_used);
    });
}

int nxc_density_set(nxc_handle *h, const nxc_density_desc *d)
{
    return guarded([&]() -> int {
    if (!h || !d) return fail(NXC_ERR_ARG, "null argument");
    const int64_t Q = d->n_points;
    if (!(d->dr > 0.0) || !std::isfinite(d->dr) || !(d->h >= d->dr * (1.0 + std::ldexp(1.0, -20))) ||
        !std::isfinite(d->h) || Q < 0 || Q > INT32_MAX || (Q && !d->points) || !d->cell_start)
        return fail(NXC_ERR_ARG, "bad nxc_density_desc");
    int64_t ncells = 1;
    for (int a = 0; a < 3; a++) {
        if (d->dims[a] < 1 || d->dims[a] > (int64_t(1) << 24) || !std::isfinite(d->origin[a]))
            return fail(NXC_ERR_ARG, "bad nxc_density_desc grid");
        ncells *= d->dims[a];
        if (ncells > (int64_t(1) << 24)) return fail(NXC_ERR_ARG, "more than 2^24 density cells");
    }
    // the kernel reads points cell_start[c] .. cell_start[c + 1] - 1: the starts must be a
    // non-decreasing walk from 0 to Q
    const int32_t *cs = d->cell_start;
    if (cs[0] != 0 || cs[ncells] != Q) return fail(NXC_ERR_ARG, "cell starts do not span the points");
    for (int64_t c = 0; c < ncells; c++)
        if (cs[c + 1] < cs[c]) return fail(NXC_ERR_ARG, "cell starts are not sorted");
    HIPCHK(hipSetDevice(h->device));
    h->have_density = false;
    h->have_dens_mom = false;
    if (int rc = spectrum_free(h)) return rc;      // up to gigabytes: not kept for a set that may never enable one
    if (int rc = h->dens_ages.release()) return rc; // likewise
    std::vector<double> pts((size_t)Q * 4, 0.0);
    for (int64_t j = 0; j < Q; j++)
        for (int a = 0; a < 3; a++) pts[4 * j + a] = d->points[3 * j + a];
    int rc;
    if ((rc = h->d_dens_pts.ensure(pts.size() * 8)) ||
        (rc = h->d_dens_cell.ensure((size_t)(ncells + 1) * 4)) ||
        (rc = h->d_dens_acc.ensure((size_t)Q * 16)))
        return rc;
    if (Q) HIPCHK(hipMemcpyAsync(h->d_dens_pts, pts.data(), pts.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_dens_cell, cs, (size_t)(ncells + 1) * 4, hipMemcpyHostToDevice, h->stream));
    if (Q) HIPCHK(hipMemsetAsync(h->d_dens_acc, 0, (size_t)Q * 16, h->stream));
    HIPCHK(stream_sync(h));
    DensityK K{};
    for (int a = 0; a < 3; a++) {
        K.o[a] = d->origin[a];
        K.n[a] = (int)d->dims[a];
    }
    K.inv_h = 1.0 / d->h;
    K.r_cell = d->dr / d->h + 1e-6;
    K.dr2 = d->dr * d->dr;
    h->dens = K;
    h->dens_q = Q;
    h->have_density = true;
    return NXC_OK;
    });
}

int nxc_density_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                           const double *z, const double *frac)
{
    return accumulate_columns<double>(h, DENSITY_SAMPLES, p, x, y, z, nullptr, frac);
}

int nxc_density_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                               const float *z, const float *frac)
{
    return accumulate_columns<float>(h, DENSITY_SAMPLES, p, x, y, z, nullptr, frac);
}

int nxc_density_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    return accumulate_rows(h, DENSITY_SAMPLES, r, first, count);
}

int nxc_density_download(nxc_handle *h, double *sum_frac, double *count)
{
    return guarded([&]() -> int {
    if (!h || !h->have_density) return fail(NXC_ERR_STATE, "nxc_density_set has not been called");
    if (h->dens_q && (!sum_frac || !count)) return fail(NXC_ERR_ARG, "bad arguments");
    if (h->dens_q == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    return download_pairs(h, h->d_dens_acc, (size_t)h->dens_q, sum_frac, count);
    });
}

int nxc_density_moments_enable(nxc_handle *h, int on)
{
    return guarded([&]() -> int {
    if (!h || !h->have_density) return fail(NXC_ERR_STATE, DENSITY_SAMPLES.unset);
    HIPCHK(hipSetDevice(h->device));
    h->have_dens_mom = false;
    if (!on) return NXC_OK;
    const size_t bytes = (size_t)h->dens_q * NXC_MOMENT_PLANES * 16;
    int rc = h->d_dens_mom.ensure(bytes);
    if (rc) return rc;
    if (bytes) HIPCHK(hipMemsetAsync(h->d_dens_mom, 0, bytes, h->stream));
    HIPCHK(stream_sync(h));
    h->have_dens_mom = true;
    return NXC_OK;
    });
}

int nxc_density_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                   const double *z, const double *vx, const double *vy,
                                   const double *vz, const double *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<double>(h, MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_density_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                       const float *z, const float *vx, const float *vy,
                                       const float *vz, const float *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<float>(h, MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_density_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_rows(h, MOMENT_SAMPLES, r, first, count);
}

int nxc_density_moments_download(nxc_handle *h, double *sums)
{
    return guarded([&]() -> int {
    if (!h || !h->have_density) return fail(NXC_ERR_STATE, DENSITY_SAMPLES.unset);
    if (!h->have_dens_mom) return fail(NXC_ERR_STATE, MOMENT_SAMPLES.unset);
    const size_t Q = (size_t)h->dens_q;
    if (Q && !sums) return fail(NXC_ERR_ARG, "bad arguments");
    if (Q == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> planes(Q * NXC_MOMENT_PLANES * 2);
    HIPCHK(hipMemcpyAsync(planes.data(), h->d_dens_mom, planes.size() * sizeof(double),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    for (size_t q = 0; q < Q; q++)
        for (size_t k = 0; k < NXC_MOMENT_PLANES; k++) {
            sums[10 * q + 2 * k] = planes[2 * (k * Q + q)];
            sums[10 * q + 2 * k + 1] = planes[2 * (k * Q + q) + 1];
        }
    return NXC_OK;
    });
}

int nxc_density_spectrum_enable(nxc_handle *h, const nxc_density_spectrum_desc *d)
{
    return guarded([&]() -> int {
    if (!h || !h->have_density) return fail(NXC_ERR_STATE, DENSITY_SAMPLES.unset);
    const size_t Q = (size_t)h->dens_q;
    const bool on = d && d->nv != 0;
    if (on) {          // before anything is freed or allocated
        const std::string why = check_spectrum_args(h->dens_q, d->n_frames, d->nv, d->s_lo, d->s_hi,
                                                    d->cos_half, d->all_sky, d->frames);
        if (!why.empty()) return fail(NXC_ERR_ARG, why.c_str());
    }
    HIPCHK(hipSetDevice(h->device));
    if (int rc = spectrum_free(h)) return rc;
    if (!on) return NXC_OK;
    h->dens_spec = SpectrumK{(int)d->nv, d->all_sky != 0 ? 1 : 0, d->s_lo,
                             spectrum_inv_ds(d->nv, d->s_lo, d->s_hi), d->cos_half};
    const size_t bytes = spectrum_bytes(Q, h->dens_spec);
    int rc;
    if ((rc = h->d_dens_spec.ensure(bytes)) || (rc = h->d_dens_frames.ensure(Q * 8 * sizeof(double))))
        return rc;
    if (Q) {
        HIPCHK(hipMemsetAsync(h->d_dens_spec, 0, bytes, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_dens_frames, d->frames, Q * 8 * sizeof(double), hipMemcpyHostToDevice,
                              h->stream));
    }
    HIPCHK(stream_sync(h));
    h->have_dens_spec = true;
    return NXC_OK;
    });
}

int nxc_density_spectrum_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                    const double *z, const double *vx, const double *vy,
                                    const double *vz, const double *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<double>(h, SPECTRUM_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_density_spectrum_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                        const float *z, const float *vx, const float *vy,
                                        const float *vz, const float *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<float>(h, SPECTRUM_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_density_spectrum_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_rows(h, SPECTRUM_SAMPLES, r, first, count);
}

int nxc_density_spectrum_download(nxc_handle *h, double *sums)
{
    return guarded([&]() -> int {
    if (!h || !h->have_density) return fail(NXC_ERR_STATE, DENSITY_SAMPLES.unset);
    if (!h->have_dens_spec) return fail(NXC_ERR_STATE, SPECTRUM_SAMPLES.unset);
    if (h->dens_q && !sums) return fail(NXC_ERR_ARG, "bad arguments");
    if (h->dens_q == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(sums, h->d_dens_spec, spectrum_bytes((size_t)h->dens_q, h->dens_spec),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_density_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi)
{
    return ages_enable(h, DENSITY_AGES, 0, na, t0, a_lo, a_hi);
}

int nxc_density_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                                const double *y, const double *z, const double *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<double>(h, DENSITY_AGES_SAMPLES, p, x, y, z, nullptr, frac, nullptr,
                                      nullptr, time);
}

int nxc_density_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                    const float *y, const float *z, const float *frac)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_columns<float>(h, DENSITY_AGES_SAMPLES, p, x, y, z, nullptr, frac, nullptr,
                                     nullptr, time);
}

int nxc_density_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = moments_need_set(h)) return rc;
    return accumulate_rows(h, DENSITY_AGES_SAMPLES, r, first, count);
}

int nxc_density_ages_download(nxc_handle *h, double *sums)
{
    return ages_copy(h, DENSITY_AGES, sums, hipMemcpyDeviceToHost);
}

int nxc_density_ages_upload(nxc_handle *h, const double *sums)
{
    return ages_copy(h, DENSITY_AGES, const_cast<double *>(sums), hipMemcpyHostToDevice);
}

int nxc_density_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out)
{
    return ages_apply(h, DENSITY_AGES, ne, K, out);
}

// ---- CameraImage ---------------------------------------------------------------------------------
int nxc_camera_set(nxc_handle *h, const nxc_camera_desc *d)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    const std::string why = check_camera_desc(d);
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    HIPCHK(hipSetDevice(h->device));
    const int nl = d->quantity == 1 ? d->n_lines : 0;
    std::vector<unsigned char> blob((size_t)NXC_HEADER_BYTES, 0);
    LdsHeader hdr = h->header;                 // nxc_log's table; the image's own G is replaced
    ImageK G{};
    std::memcpy(G.M, d->C, sizeof G.M);       // the basis, where the image keeps its rotation
    G.vrplanet = d->vrplanet;
    G.apix_cm2 = 1.0;                          // the per-sample area divides in camera_located
    G.quantity = d->quantity;
    PackedLut luts[NXC_MAX_LINES];
    int rc;
    if ((rc = pack_lines(nl, d->line_v, d->line_g, d->line_n, luts))) return rc;
    place_image_block(append_image_block(blob, G, d->nx, d->nz, d->uedges, d->vedges, nl, luts),
                      NXC_HEADER_BYTES, G);
    if (blob.size() > 160 * 1024)
        return fail(NXC_ERR_ARG, "nxc_camera_desc: tables and edges exceed the 160 KiB LDS of a gfx950 CU");
    hdr.G = G;
    std::memcpy(blob.data(), &hdr, sizeof(LdsHeader));

    CameraK K{};
    for (int a = 0; a < 3; a++) K.o[a] = d->o[a];
    K.area = d->pix_area_cm2;

    h->have_camera = false;
    h->cam_px.have_mom = false;
    h->cam_px.have_cube = false;
    h->cam_px.ages.have = false;
    const size_t npix = (size_t)d->nx * (size_t)d->nz;
    if ((rc = h->d_blob_cam.ensure(blob.size())) ||
        (rc = h->cam_px.image.ensure(2 * npix * sizeof(double))))
        return rc;
    HIPCHK(hipMemcpyAsync(h->d_blob_cam, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->cam_px.image, 0, 2 * npix * sizeof(double), h->stream));
    HIPCHK(stream_sync(h));                    // blob is a local
    h->cam = K;
    h->cam_bytes = blob.size();
    h->cam_px.npix = npix;
    h->have_camera = true;
    return NXC_OK;
    });
}

int nxc_camera_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                          const double *z, const double *vy, const double *frac)
{
    return accumulate_columns(h, CAMERA_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_camera_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                              const float *z, const float *vy, const float *frac)
{
    return accumulate_columns(h, CAMERA_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_camera_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    return accumulate_rows(h, CAMERA_SAMPLES, r, first, count);
}

int nxc_camera_download(nxc_handle *h, double *image, uint64_t *counts)
{
    return guarded([&]() -> int {
    if (!h || !h->have_camera) return fail(NXC_ERR_STATE, "nxc_camera_set has not been called");
    HIPCHK(hipSetDevice(h->device));
    return download_pairs(h, h->cam_px.image, h->cam_px.npix, image, counts);
    });
}

int nxc_camera_moments_enable(nxc_handle *h, int on)
{
    return pixel_moments_enable(h, CAMERA_SAMPLES, on);
}

int nxc_camera_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                  const double *z, const double *vx, const double *vy,
                                  const double *vz, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<double>(h, CAMERA_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_camera_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                      const float *z, const float *vx, const float *vy,
                                      const float *vz, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<float>(h, CAMERA_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_camera_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_rows(h, CAMERA_MOMENT_SAMPLES, r, first, count);
}

int nxc_camera_moments_download(nxc_handle *h, double *sums)
{
    return pixel_moments_download(h, CAMERA_SAMPLES, CAMERA_MOMENT_SAMPLES, sums);
}

int nxc_camera_cube_enable(nxc_handle *h, int64_t nv, double v_lo, double v_hi)
{
    return pixel_cube_enable(h, CAMERA_SAMPLES, nv, v_lo, v_hi);
}

int nxc_camera_cube_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                               const double *z, const double *vx, const double *vy,
                               const double *vz, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<double>(h, CAMERA_CUBE_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_camera_cube_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                   const float *z, const float *vx, const float *vy,
                                   const float *vz, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<float>(h, CAMERA_CUBE_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_camera_cube_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_rows(h, CAMERA_CUBE_SAMPLES, r, first, count);
}

int nxc_camera_cube_download(nxc_handle *h, double *sums)
{
    return pixel_cube_download(h, CAMERA_SAMPLES, CAMERA_CUBE_SAMPLES, sums);
}

int nxc_camera_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi)
{
    return ages_enable(h, CAMERA_AGES, 0, na, t0, a_lo, a_hi);
}

int nxc_camera_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                               const double *y, const double *z, const double *vy, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<double>(h, CAMERA_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_camera_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                   const float *y, const float *z, const float *vy, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_columns<float>(h, CAMERA_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_camera_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, CAMERA_SAMPLES)) return rc;
    return accumulate_rows(h, CAMERA_AGES_SAMPLES, r, first, count);
}

int nxc_camera_ages_download(nxc_handle *h, double *sums)
{
    return ages_copy(h, CAMERA_AGES, sums, hipMemcpyDeviceToHost);
}

int nxc_camera_ages_upload(nxc_handle *h, const double *sums)
{
    return ages_copy(h, CAMERA_AGES, const_cast<double *>(sums), hipMemcpyHostToDevice);
}

int nxc_camera_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out)
{
    return ages_apply(h, CAMERA_AGES, ne, K, out);
}

// ---- ShellMap --------------------------------------------------------------------------------------
int nxc_shell_set(nxc_handle *h, const nxc_shell_desc *d)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    std::string why = check_shell_desc(d);
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    HIPCHK(hipSetDevice(h->device));
    const int nl = d->quantity == 1 ? d->n_lines : 0;
    std::vector<unsigned char> blob((size_t)NXC_HEADER_BYTES, 0);
    LdsHeader hdr = h->header;                 // nxc_log's table; the image's own G is replaced
    ImageK G{};
    G.vrplanet = d->vrplanet;
    G.apix_cm2 = 1.0;                          // image_weight's last division is exact
    G.quantity = d->quantity;
    PackedLut luts[NXC_MAX_LINES];
    int rc;
    if ((rc = pack_lines(nl, d->line_v, d->line_g, d->line_n, luts))) return rc;
    place_image_block(append_image_block(blob, G, d->nlon, d->nlat, d->lon_edges, d->mu_edges, nl, luts),
                      NXC_HEADER_BYTES, G);
    why = check_shell_blob(blob.size());
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    hdr.G = G;
    std::memcpy(blob.data(), &hdr, sizeof(LdsHeader));

    ShellK K{};
    K.nalt = (int)d->nalt;
    K.r_lo = d->r_lo;
    K.inv_dr = shell_inv_dr(d->nalt, d->r_lo, d->r_hi);
    K.plane = (int64_t)shell_plane_doubles(d->nlon, d->nlat, d->nalt);
    K.replicas = (int)shell_replicas(d->nlon * d->nlat);
    K.pairs = 2 * d->nlon * d->nlat;

    h->have_shell = false;
    h->have_shell_mom = false;                 // the moments go with the map they were enabled on
    if ((rc = h->d_shell_mom.release())) return rc;
    if ((rc = h->shell_ages.release())) return rc;  // likewise the ages
    const size_t cells = (size_t)d->nlon * (size_t)d->nlat;
    const size_t pair_bytes = (size_t)K.replicas * 2 * cells * sizeof(double);
    const size_t plane_bytes = 2 * (size_t)K.plane * sizeof(double);
    if ((rc = h->d_blob_shell.ensure(blob.size())) ||
        (rc = h->shell_px.image.ensure(pair_bytes)) ||
        (rc = h->d_shell_planes.ensure(plane_bytes)))
        return rc;
    HIPCHK(hipMemcpyAsync(h->d_blob_shell, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->shell_px.image, 0, pair_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->d_shell_planes, 0, plane_bytes, h->stream));
    HIPCHK(stream_sync(h));                    // blob is a local
    h->shell = K;
    h->shell_bytes = blob.size();
    h->shell_px.npix = cells;
    h->have_shell = true;
    return NXC_OK;
    });
}

int nxc_shell_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                         const double *z, const double *vy, const double *frac)
{
    return accumulate_columns(h, SHELL_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_shell_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                             const float *z, const float *vy, const float *frac)
{
    return accumulate_columns(h, SHELL_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_shell_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    return accumulate_rows(h, SHELL_SAMPLES, r, first, count);
}

int nxc_shell_download(nxc_handle *h, double *column, uint64_t *counts, double *sums)
{
    return guarded([&]() -> int {
    if (!h || !h->have_shell) return fail(NXC_ERR_STATE, SHELL_SAMPLES.unset);
    HIPCHK(hipSetDevice(h->device));
    if (sums) {
        HIPCHK(hipMemcpyAsync(sums, h->d_shell_planes, 2 * (size_t)h->shell.plane * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
        HIPCHK(stream_sync(h));
    }
    if (!column && !counts) return NXC_OK;
    // the copies of the pair array, summed in their order (the counts are integers below 2^53)
    const size_t cells = h->shell_px.npix, copies = (size_t)h->shell.replicas;
    std::vector<double> all(copies * 2 * cells);
    HIPCHK(hipMemcpyAsync(all.data(), h->shell_px.image, all.size() * sizeof(double),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    for (size_t q = 0; q < cells; q++) {
        double c = 0.0, n = 0.0;
        for (size_t r = 0; r < copies; r++) {
            c += all[2 * (r * cells + q)];
            n += all[2 * (r * cells + q) + 1];
        }
        if (column) column[q] = c;
        if (counts) counts[q] = (uint64_t)n;
    }
    return NXC_OK;
    });
}

// ---- ShellMap moments ------------------------------------------------------------------------------
int nxc_shell_moments_enable(nxc_handle *h, int on)
{
    return guarded([&]() -> int {
    const ShellMomentsRefusal r = check_shell_moments_enable(shell_moments_state(h));
    if (r.code != NXC_OK) return fail(r.code, r.why);
    HIPCHK(hipSetDevice(h->device));
    h->have_shell_mom = false;
    int rc = h->d_shell_mom.release();
    if (rc || !on) return rc;
    const size_t bytes = shell_moments_bytes(h->shell.plane);
    if ((rc = h->d_shell_mom.ensure(bytes))) return rc;
    HIPCHK(hipMemsetAsync(h->d_shell_mom, 0, bytes, h->stream));
    HIPCHK(stream_sync(h));
    h->have_shell_mom = true;
    return NXC_OK;
    });
}

int nxc_shell_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                 const double *z, const double *vx, const double *vy,
                                 const double *vz, const double *frac)
{
    if (int rc = shell_moments_ready(h)) return rc;
    return accumulate_columns<double>(h, SHELL_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_shell_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                     const float *z, const float *vx, const float *vy,
                                     const float *vz, const float *frac)
{
    if (int rc = shell_moments_ready(h)) return rc;
    return accumulate_columns<float>(h, SHELL_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_shell_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = shell_moments_ready(h)) return rc;
    return accumulate_rows(h, SHELL_MOMENT_SAMPLES, r, first, count);
}

int nxc_shell_moments_download(nxc_handle *h, double *sums)
{
    return guarded([&]() -> int {
    const ShellMomentsRefusal r = check_shell_moments_download(shell_moments_state(h), sums);
    if (r.code != NXC_OK) return fail(r.code, r.why);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(sums, h->d_shell_mom, shell_moments_bytes(h->shell.plane),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

// ---- ShellMap ages ---------------------------------------------------------------------------------
int nxc_shell_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi)
{
    return ages_enable(h, SHELL_AGES, 0, na, t0, a_lo, a_hi);
}

int nxc_shell_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                              const double *y, const double *z, const double *vy, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, SHELL_SAMPLES)) return rc;
    return accumulate_columns<double>(h, SHELL_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_shell_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                  const float *y, const float *z, const float *vy, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, SHELL_SAMPLES)) return rc;
    return accumulate_columns<float>(h, SHELL_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_shell_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, SHELL_SAMPLES)) return rc;
    return accumulate_rows(h, SHELL_AGES_SAMPLES, r, first, count);
}

int nxc_shell_ages_download(nxc_handle *h, double *sums)
{
    return ages_copy(h, SHELL_AGES, sums, hipMemcpyDeviceToHost);
}

int nxc_shell_ages_upload(nxc_handle *h, const double *sums)
{
    return ages_copy(h, SHELL_AGES, const_cast<double *>(sums), hipMemcpyHostToDevice);
}

int nxc_shell_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out)
{
    return ages_apply(h, SHELL_AGES, ne, K, out);
}

// ---- source maps ---------------------------------------------------------------------------------
namespace {
size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

void set_axis(const double *e, int64_t n, double &lo, double &hi, double &inv)
{
    lo = e[0];
    hi = e[n];
    inv = (double)n / (hi - lo);
}

// the dynamic LDS of k_smap_points and k_smap_prep (nxc_source_map_check.hpp; nxc_source_map_set
// has held both to NXC_SMAP_LDS_BYTES)
size_t smap_points_lds(const SmapK &K)
{
    return smap_points_lds_bytes(K.tile, K.nvel, K.nalt, K.naz, K.nseg_max);
}

size_t smap_prep_lds(const SmapK &K) { return smap_prep_lds_bytes(K.nvel, K.nalt, K.naz, K.nlon, K.nlat); }
}  // namespace

int nxc_source_map_set(nxc_handle *h, const nxc_source_map_desc *d)
{
    return guarded([&]() -> int {
    if (!h || !d) return fail(NXC_ERR_ARG, "null argument");
    // the grid, the tables, the segment lists and the LDS of both kernels (nxc_source_map_check.hpp)
    int64_t nseg_max = 0;
    const std::string why = check_source_map_desc(d, &nseg_max);
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    const int64_t nlon = d->nlon, nlat = d->nlat;
    const int64_t tpr = (nlon + d->tile - 1) / d->tile, ntiles = tpr * nlat, ncells = nlon * nlat;
    SmapK K{};
    K.r_km = d->r_km;
    K.nlon = (int)nlon; K.nlat = (int)nlat;
    K.nvel = (int)d->nvel; K.nalt = (int)d->nalt; K.naz = (int)d->naz;
    K.tile = (int)d->tile; K.tiles_per_row = (int)tpr; K.nseg_max = (int)nseg_max;
    set_axis(d->alt_edges, d->nalt, K.alt_lo, K.alt_hi, K.alt_inv);
    set_axis(d->az_edges, d->naz, K.az_lo, K.az_hi, K.az_inv);
    set_axis(d->lon_edges, nlon, K.lon_lo, K.lon_hi, K.lon_inv);
    set_axis(d->lat_edges, nlat, K.lat_lo, K.lat_hi, K.lat_inv);
    HIPCHK(hipSetDevice(h->device));
    h->have_smap = false;
    const int64_t npoints = ncells, stride = smap_stride(K);
    const size_t grid_bytes = align256(8 * (size_t)(2 * nlat + nlon + nlat)) +
                              align256(4 * (size_t)(ntiles + 1)) + 8 * (size_t)std::max<int64_t>(d->n_seg, 1);
    std::vector<unsigned char> grid(grid_bytes, 0);
    double *g = reinterpret_cast<double *>(grid.data());
    std::copy(d->point_lon, d->point_lon + nlon, g);
    std::copy(d->point_lat, d->point_lat + nlat, g + nlon);
    std::copy(d->point_cos, d->point_cos + nlat, g + nlon + nlat);
    std::copy(d->threshold, d->threshold + nlat, g + nlon + 2 * nlat);
    const size_t off_segoff = align256(8 * (size_t)(2 * nlat + nlon + nlat));
    const size_t off_seg = off_segoff + align256(4 * (size_t)(ntiles + 1));
    std::copy(d->seg_off, d->seg_off + ntiles + 1, reinterpret_cast<int32_t *>(grid.data() + off_segoff));
    if (d->n_seg)
        std::copy(d->seg, d->seg + 2 * d->n_seg, reinterpret_cast<int32_t *>(grid.data() + off_seg));
    const size_t acc_bytes = 8 * (size_t)npoints * (size_t)(stride + 1);
    int rc;
    if ((rc = h->d_smap_grid.ensure(grid_bytes)) ||
        (rc = h->d_smap_acc.ensure(acc_bytes)))
        return rc;
    HIPCHK(hipMemcpyAsync(h->d_smap_grid, grid.data(), grid_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_smap_acc, 0, acc_bytes, h->stream));
    HIPCHK(stream_sync(h));
    h->smap_edges.clear();
    for (auto [e, n] : {std::pair<const double *, int64_t>{d->alt_edges, d->nalt}, {d->az_edges, d->naz},
                        {d->lon_edges, nlon}, {d->lat_edges, nlat}})
        h->smap_edges.insert(h->smap_edges.end(), e, e + n + 1);
    h->smap = K;
    h->smap_ntiles = ntiles;
    h->smap_ncells = ncells;
    h->have_smap = true;
    return NXC_OK;
    });
}

int nxc_source_map_accumulate(nxc_handle *h, int64_t n, const double *lat, const double *lon,
                              const double *v, const double *alt, const double *az,
                              const double *frac, const int32_t *cell_start,
                              const double *vel_edges, int32_t available, double factor,
                              double *small)
{
    return guarded([&]() -> int {
    if (!h || !h->have_smap) return fail(NXC_ERR_STATE, "nxc_source_map_set has not been called");
    SmapK K = h->smap;
    if (n < 0 || n > INT32_MAX || !cell_start || !small ||
        (n && (!lat || !lon || !v || !alt || !az || !frac)) || !std::isfinite(factor))
        return fail(NXC_ERR_ARG, "bad arguments");
    if (!smap_linspace_ok(vel_edges, K.nvel))
        return fail(NXC_ERR_ARG, "speed edges must be finite and increasing");
    const int64_t nc = h->smap_ncells;
    if (cell_start[0] != 0 || cell_start[nc] > n)
        return fail(NXC_ERR_ARG, "cell starts do not lie within the packets");
    for (int64_t c = 0; c < nc; c++)
        if (cell_start[c + 1] < cell_start[c]) return fail(NXC_ERR_ARG, "cell starts are not sorted");
    set_axis(vel_edges, K.nvel, K.vel_lo, K.vel_hi, K.vel_inv);
    K.available = available ? 1 : 0;
    HIPCHK(hipSetDevice(h->device));
    const int nh = K.nvel + K.nalt + K.naz;
    const size_t col = align256(8 * (size_t)std::max<int64_t>(n, 1));
    const size_t geo_b = align256(32 * (size_t)std::max<int64_t>(n, 1));
    const size_t bins_b = align256(16 * (size_t)std::max<int64_t>(n, 1));
    const size_t cs_b = align256(4 * (size_t)(nc + 1));
    const size_t ne = (size_t)(K.nvel + 1) + h->smap_edges.size();
    const size_t edges_b = align256(8 * ne);
    const size_t small_b = align256(8 * (size_t)(nh + K.nvel));
    const size_t part_b = 8 * (size_t)h->smap_ntiles * K.nvel;
    int rc = h->d_smap_pk.ensure(6 * col + geo_b + bins_b + cs_b + edges_b + small_b + part_b);
    if (rc) return rc;
    unsigned char *base = h->d_smap_pk;
    double *dcol = reinterpret_cast<double *>(base);
    double4 *geo = reinterpret_cast<double4 *>(base + 6 * col);
    int4 *bins = reinterpret_cast<int4 *>(base + 6 * col + geo_b);
    int *dcs = reinterpret_cast<int *>(base + 6 * col + geo_b + bins_b);
    double *dedges = reinterpret_cast<double *>(base + 6 * col + geo_b + bins_b + cs_b);
    double *dsmall = reinterpret_cast<double *>(base + 6 * col + geo_b + bins_b + cs_b + edges_b);
    double *dpart = reinterpret_cast<double *>(base + 6 * col + geo_b + bins_b + cs_b + edges_b + small_b);
    const double *src[6] = {lat, lon, v, alt, az, frac};
    if (n)
        for (int c = 0; c < 6; c++)
            HIPCHK(hipMemcpyAsync(reinterpret_cast<unsigned char *>(dcol) + c * col, src[c], 8 * (size_t)n,
                                  hipMemcpyHostToDevice, h->stream));
    std::vector<double> edges(ne);
    std::copy(vel_edges, vel_edges + K.nvel + 1, edges.begin());
    std::copy(h->smap_edges.begin(), h->smap_edges.end(), edges.begin() + K.nvel + 1);
    HIPCHK(hipMemcpyAsync(dedges, edges.data(), 8 * ne, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dcs, cell_start, 4 * (size_t)(nc + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(dsmall, 0, 8 * (size_t)(nh + K.nvel), h->stream));
    const int64_t npoints = (int64_t)K.nlon * K.nlat;
    double *acc = h->d_smap_acc, *hist2d = h->d_smap_acc + npoints * smap_stride(K);
    const unsigned char *gb = h->d_smap_grid;
    const int nlon = K.nlon, nlat = K.nlat;
    const size_t off_segoff = align256(8 * (size_t)(2 * nlat + nlon + nlat));
    const size_t off_seg = off_segoff + align256(4 * (size_t)(h->smap_ntiles + 1));
    const double *pt_lon = reinterpret_cast<const double *>(gb);
    const int *seg_off = reinterpret_cast<const int *>(gb + off_segoff);
    const int2 *seg = reinterpret_cast<const int2 *>(gb + off_seg);
    if ((rc = begin_timed(h))) return rc;
    if (n) {
        const size_t lds = smap_prep_lds(K);      // 8 * (ne + nh), within NXC_SMAP_LDS_BYTES since set
        const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + NXC_BLOCK - 1) / NXC_BLOCK,
                                                                    (int64_t)h->n_cu * 8));
        hipLaunchKernelGGL(k_smap_prep, dim3((unsigned)grid), dim3(NXC_BLOCK), lds, h->stream, K, (int)n,
                           dcol, reinterpret_cast<const double *>(reinterpret_cast<unsigned char *>(dcol) + col),
                           reinterpret_cast<const double *>(reinterpret_cast<unsigned char *>(dcol) + 2 * col),
                           reinterpret_cast<const double *>(reinterpret_cast<unsigned char *>(dcol) + 3 * col),
                           reinterpret_cast<const double *>(reinterpret_cast<unsigned char *>(dcol) + 4 * col),
                           reinterpret_cast<const double *>(reinterpret_cast<unsigned char *>(dcol) + 5 * col),
                           dedges, geo, bins, dsmall, hist2d);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_smap_points, dim3((unsigned)h->smap_ntiles), dim3(NXC_BLOCK), smap_points_lds(K),
                       h->stream, K, geo, bins, dcs, seg, seg_off, pt_lon, pt_lon + nlon,
                       pt_lon + nlon + nlat, pt_lon + nlon + 2 * nlat, factor, acc, dpart);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_smap_gridsum, dim3((unsigned)K.nvel), dim3(NXC_BLOCK), 8 * NXC_BLOCK, h->stream,
                       (int)h->smap_ntiles,
                       K.nvel, dpart, dsmall + nh);
    HIPCHK(hipGetLastError());
    if ((rc = end_timed(h))) return rc;
    HIPCHK(hipMemcpyAsync(small, dsmall, 8 * (size_t)(nh + K.nvel), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_source_map_download(nxc_handle *h, double *map, double *hist2d)
{
    return guarded([&]() -> int {
    if (!h || !h->have_smap) return fail(NXC_ERR_STATE, "nxc_source_map_set has not been called");
    if (!map || !hist2d) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const int64_t npoints = (int64_t)h->smap.nlon * h->smap.nlat;
    const size_t mb = 8 * (size_t)npoints * smap_stride(h->smap);
    HIPCHK(hipMemcpyAsync(map, h->d_smap_acc, mb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(hist2d, h->d_smap_acc + npoints * smap_stride(h->smap), 8 * (size_t)npoints,
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_pairs_create(nxc_handle *h, int64_t capacity, nxc_pairs **out)
{
    return guarded([&]() -> int {
    if (!h || !out) return fail(NXC_ERR_ARG, "null argument");
    *out = nullptr;
    if (capacity < 1) return fail(NXC_ERR_ARG, "a pair list needs a capacity >= 1");
    HIPCHK(hipSetDevice(h->device));
    nxc_pairs *p = new (std::nothrow) nxc_pairs();
    if (!p) return fail(NXC_ERR_ARG, "out of host memory");
    p->device = h->device;
    p->cap = capacity;
    if (p->d.ensure((size_t)capacity * 16)) {
        delete p;
        return fail(NXC_ERR_NOMEM, "pair list of " + std::to_string(capacity) + " pairs");
    }
    *out = p;
    return NXC_OK;
    });
}

int nxc_pairs_free(nxc_handle *h, nxc_pairs *p)
{
    if (!p) return NXC_OK;
    (void)hipSetDevice(p->device);
    if (h && h->stream) (void)stream_sync(h);
    if (h && h->los_pairs == p) h->los_pairs = nullptr;
    delete p;
    return NXC_OK;
}

int nxc_pairs_count(const nxc_pairs *p, int64_t *n)
{
    if (!p || !n) return fail(NXC_ERR_ARG, "null argument");
    *n = p->n;
    return NXC_OK;
}

int nxc_pairs_download(nxc_handle *h, const nxc_pairs *p, int64_t *spectrum, int64_t *row)
{
    return guarded([&]() -> int {
    if (!h || !p) return fail(NXC_ERR_ARG, "null argument");
    if (p->device != h->device) return fail(NXC_ERR_ARG, "the pair list lives on another device");
    if (p->n == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    if (spectrum) HIPCHK(hipMemcpyAsync(spectrum, p->d, (size_t)p->n * 8, hipMemcpyDeviceToHost, h->stream));
    if (row) HIPCHK(hipMemcpyAsync(row, p->d + p->cap, (size_t)p->n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_los_set_pairs(nxc_handle *h, nxc_pairs *p)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (p && p->device != h->device) return fail(NXC_ERR_ARG, "the pair list lives on another device");
    h->los_pairs = p;
    return NXC_OK;
}

int nxc_fit_set(nxc_handle *h, const nxc_fit_desc *d)
{
    return guarded([&]() -> int {
    if (!h || !d) return fail(NXC_ERR_ARG, "null argument");
    const int64_t S = d->n_spectra;
    if (S < 1 || d->weight_mode < 0 || d->weight_mode > 3 || !d->position || !d->ratio || !d->mask ||
        (d->weight_mode == 3 && !d->weight))
        return fail(NXC_ERR_ARG, "bad nxc_fit_desc");
    HIPCHK(hipSetDevice(h->device));
    h->have_fit = false;
    h->have_fit_src = false;
    h->fit_np = -1;
    int rc = h->d_fit_spec.ensure((size_t)S * 6 * 8 + (size_t)S);
    if (rc) return rc;
    h->fit_S = S;
    std::vector<double> w((size_t)S, 1.0);
    if (d->weight_mode == 3) w.assign(d->weight, d->weight + S);
    HIPCHK(hipMemcpyAsync(fit_pos(h), d->position, (size_t)S * 24, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(fit_ratio(h), d->ratio, (size_t)S * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(fit_weight(h), w.data(), (size_t)S * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(fit_rad(h), 0, (size_t)S * 8, h->stream));
    HIPCHK(hipMemcpyAsync(fit_mask(h), d->mask, (size_t)S, hipMemcpyHostToDevice, h->stream));
    HIPCHK(stream_sync(h));
    h->fit_mode = d->weight_mode;
    h->have_fit = true;
    return NXC_OK;
    });
}

int nxc_fit_source_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count, int64_t index_shift)
{
    return guarded([&]() -> int {
    if (!h || !h->have_fit) return fail(NXC_ERR_STATE, "nxc_fit_set has not been called");
    Samples s;
    int rc = samples_from_rows(h, r, first, count, index_shift, &s);
    if (rc) return rc;
    h->fit_src = s;
    h->have_fit_src = true;
    h->fit_np = -1;
    return NXC_OK;
    });
}

int nxc_fit_source(nxc_handle *h, int64_t P, const double *x, const double *y, const double *z,
                   const double *vy, const double *frac, const int64_t *index)
{
    return guarded([&]() -> int { return fit_source_columns(h, P, x, y, z, vy, frac, index); });
}

int nxc_fit_source_f32(nxc_handle *h, int64_t P, const float *x, const float *y, const float *z,
                       const float *vy, const float *frac, const int64_t *index)
{
    return guarded([&]() -> int { return fit_source_columns(h, P, x, y, z, vy, frac, index); });
}

int nxc_fit_packets(nxc_handle *h, const nxc_pairs *p, int64_t n_packets, double *num, double *den,
                    int32_t *cnt, double *mult, double *stats)
{
    return guarded([&]() -> int {
    int rc = fit_check(h, p);
    if (rc) return rc;
    if (n_packets < 0 || n_packets > INT32_MAX) return fail(NXC_ERR_ARG, "bad packet count");
    h->fit_np = -1;
    if ((rc = h->d_fit_pk.ensure((size_t)n_packets * 32 + 16)))
        return rc;
    unsigned char *blob;
    unsigned long long *ctr;
    if ((rc = fit_aux(h, 16, &blob, &ctr))) return rc;
    double *d_stats = reinterpret_cast<double *>(blob);
    HIPCHK(hipMemsetAsync(h->d_fit_pk, 0, (size_t)n_packets * 28, h->stream));   // num, den, mult, cnt
    HIPCHK(hipMemsetAsync(blob, 0, 256 + 64, h->stream));                         // stats, counters
    if ((rc = begin_timed(h))) return rc;
    rc = with_sample_types(h->fit_src, [&](auto t, auto i) {
        return fit_packets_run<decltype(t), decltype(i)>(h, p, n_packets, ctr);
    });
    if (rc) return rc;
    if (n_packets) {
        hipLaunchKernelGGL(k_fit_norm, dim3(1), dim3(NXC_FIT_NORM_THREADS), 0, h->stream, n_packets,
                           fit_num(h, n_packets), fit_den(h, n_packets), fit_mult(h, n_packets), d_stats);
        HIPCHK(hipGetLastError());
    }
    if ((rc = end_timed(h))) return rc;
    unsigned long long bad = 0;
    double st[2] = {0.0, 0.0};
    HIPCHK(hipMemcpyAsync(&bad, ctr, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st, d_stats, 16, hipMemcpyDeviceToHost, h->stream));
    const size_t n8 = (size_t)n_packets * 8;
    if (num && n_packets) HIPCHK(hipMemcpyAsync(num, fit_num(h, n_packets), n8, hipMemcpyDeviceToHost, h->stream));
    if (den && n_packets) HIPCHK(hipMemcpyAsync(den, fit_den(h, n_packets), n8, hipMemcpyDeviceToHost, h->stream));
    if (mult && n_packets) HIPCHK(hipMemcpyAsync(mult, fit_mult(h, n_packets), n8, hipMemcpyDeviceToHost, h->stream));
    if (cnt && n_packets)
        HIPCHK(hipMemcpyAsync(cnt, fit_cnt(h, n_packets), (size_t)n_packets * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; }
    if (bad) return fail(NXC_ERR_ARG, std::to_string(bad) + " pairs name a spectrum, row or packet outside the fit");
    h->fit_np = n_packets;
    return NXC_OK;
    });
}

int nxc_fit_radiance(nxc_handle *h, const nxc_pairs *p, const nxc_los_desc *d)
{
    return guarded([&]() -> int {
    int rc = fit_check(h, p);
    if (rc) return rc;
    if (h->fit_np < 0) return fail(NXC_ERR_STATE, "nxc_fit_radiance needs a preceding nxc_fit_packets");
    if (!d || d->n_lines < 0 || d->n_lines > NXC_MAX_LINES || d->n_ladder < 1 || !d->ladder)
        return fail(NXC_ERR_ARG, "bad nxc_los_desc");
    std::vector<unsigned char> blob;
    LosK K{};
    if ((rc = los_tables(h, d, K, blob))) return rc;
    if (((blob.size() + 31) & ~size_t(31)) > 160 * 1024) return fail(NXC_ERR_ARG, "g-value tables exceed the LDS");
    unsigned char *d_blob;
    unsigned long long *ctr;
    if ((rc = fit_aux(h, blob.size(), &d_blob, &ctr))) return rc;
    HIPCHK(hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(ctr, 0, 16, h->stream));
    if ((rc = begin_timed(h))) return rc;
    rc = with_sample_types(h->fit_src, [&](auto t, auto i) {
        return fit_radiance_run<decltype(t), decltype(i)>(h, p, K, blob.size(), d_blob, ctr);
    });
    if (rc) return rc;
    if ((rc = end_timed(h))) return rc;
    unsigned long long c[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(c, ctr, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    if (c[0]) return fail(NXC_ERR_ARG, std::to_string(c[0]) + " pairs name a spectrum, row or packet outside the fit");
    if (c[1]) return fail(NXC_ERR_ARG, std::to_string(c[1]) + " fitted pair weights are not finite");
    return NXC_OK;
    });
}

int nxc_fit_rows(nxc_handle *h, int compress, nxc_rows **out, int64_t *lengths_out)
{
    return guarded([&]() -> int {
    if (!out) return fail(NXC_ERR_ARG, "out is null");
    *out = nullptr;
    if (!h || !h->have_fit) return fail(NXC_ERR_STATE, "nxc_fit_set has not been called");
    if (!h->have_fit_src || !h->fit_src.store) return fail(NXC_ERR_STATE, "nxc_fit_rows needs a row-store source");
    if (h->fit_np < 0) return fail(NXC_ERR_STATE, "nxc_fit_rows needs a preceding nxc_fit_packets");
    HIPCHK(hipSetDevice(h->device));
    // a store's types: (float, int) or (double, long long)
    if (h->fit_src.f32) return fit_rows_run<float, int>(h, compress, out, lengths_out);
    return fit_rows_run<double, long long>(h, compress, out, lengths_out);
    });
}

int nxc_fit_download(nxc_handle *h, double *radiance)
{
    return guarded([&]() -> int {
    if (!h || !h->have_fit) return fail(NXC_ERR_STATE, "nxc_fit_set has not been called");
    if (!radiance) return fail(NXC_ERR_ARG, "radiance is null");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(radiance, fit_rad(h), (size_t)h->fit_S * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_rows_fetch(nxc_handle *h, double *rows_out)
{
    return guarded([&]() -> int { return rows_fetch(h, rows_out, false); });
}

int nxc_rows_fetch_f32(nxc_handle *h, float *rows_out)
{
    return guarded([&]() -> int { return rows_fetch(h, rows_out, true); });
}

int nxc_integrate_var(nxc_handle *h, double resolution, double outeredge, int64_t max_steps,
                      double *final_out, double *hstore_out)
{
    return guarded([&]() -> int {
    double *d_final = nullptr, *d_hs = nullptr;
    int rc = var_launch(h, resolution, outeredge, max_steps, final_out != nullptr, 0, &d_final, &d_hs);
    if (rc) return rc;
    const size_t col = (size_t)h->n_packets * sizeof(double);
    HIPCHK(hipMemcpyAsync(final_out, d_final, 8 * col, hipMemcpyDeviceToHost, h->stream));
    if (hstore_out)
        HIPCHK(hipMemcpyAsync(hstore_out, d_hs, col, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_integrate_var_resident(nxc_handle *h, double resolution, double outeredge, int64_t max_steps,
                               double *hstore_out)
{
    return guarded([&]() -> int {
    double *d_final = nullptr, *d_hs = nullptr;
    const size_t extra = h && h->n_packets > 0 ? var_rows_scratch(h->n_packets) : 0;
    int rc = var_launch(h, resolution, outeredge, max_steps, true, extra, &d_final, &d_hs);
    if (rc) return rc;
    h->rows_total = -1;                      // a counted constant-step run's finals are gone
    if (hstore_out)
        HIPCHK(hipMemcpyAsync(hstore_out, d_hs, (size_t)h->n_packets * sizeof(double),
                              hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    h->var_n = h->n_packets;
    return NXC_OK;
    });
}

int nxc_var_rows_build(nxc_handle *h, int narrow, int compress, nxc_rows **out, uint8_t *kept_out)
{
    return guarded([&]() -> int {
    if (!out) return fail(NXC_ERR_ARG, "out is null");
    *out = nullptr;
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (h->var_n < 1 || h->var_n != h->n_packets)
        return fail(NXC_ERR_STATE, "nxc_var_rows_build needs a preceding nxc_integrate_var_resident "
                                   "on the resident packets");
    if (narrow && h->var_n > (int64_t)INT32_MAX)
        return fail(NXC_ERR_ARG, "more packets than a 32-bit index column numbers");
    HIPCHK(hipSetDevice(h->device));
    if (narrow) return var_rows_run<float, int>(h, compress, out, kept_out);
    return var_rows_run<double, long long>(h, compress, out, kept_out);
    });
}

#ifdef NXC_VAR_TRACE
extern "C" int nxc_debug_var_trace(nxc_handle *h, unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_var_trace), sizeof(unsigned long long) * 8 * 4096) == hipSuccess ? 0 : -1;
}
#endif

int nxc_image_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                         const double *z, const double *vy, const double *frac)
{
    return accumulate_columns(h, IMAGE_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_image_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                             const float *z, const float *vy, const float *frac)
{
    return accumulate_columns(h, IMAGE_SAMPLES, p, x, y, z, vy, frac);
}

int nxc_image_moments_enable(nxc_handle *h, int on)
{
    return pixel_moments_enable(h, IMAGE_SAMPLES, on);
}

int nxc_image_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                 const double *z, const double *vx, const double *vy,
                                 const double *vz, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<double>(h, IMAGE_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_image_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                     const float *z, const float *vx, const float *vy,
                                     const float *vz, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<float>(h, IMAGE_MOMENT_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_image_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_rows(h, IMAGE_MOMENT_SAMPLES, r, first, count);
}

int nxc_image_moments_download(nxc_handle *h, double *sums)
{
    return pixel_moments_download(h, IMAGE_SAMPLES, IMAGE_MOMENT_SAMPLES, sums);
}

int nxc_image_cube_enable(nxc_handle *h, int64_t nv, double v_lo, double v_hi)
{
    return pixel_cube_enable(h, IMAGE_SAMPLES, nv, v_lo, v_hi);
}

int nxc_image_cube_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                              const double *z, const double *vx, const double *vy,
                              const double *vz, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<double>(h, IMAGE_CUBE_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_image_cube_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                  const float *z, const float *vx, const float *vy,
                                  const float *vz, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<float>(h, IMAGE_CUBE_SAMPLES, p, x, y, z, vy, frac, vx, vz);
}

int nxc_image_cube_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_rows(h, IMAGE_CUBE_SAMPLES, r, first, count);
}

int nxc_image_cube_download(nxc_handle *h, double *sums)
{
    return pixel_cube_download(h, IMAGE_SAMPLES, IMAGE_CUBE_SAMPLES, sums);
}

int nxc_image_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi)
{
    return ages_enable(h, IMAGE_AGES, 0, na, t0, a_lo, a_hi);
}

int nxc_image_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                               const double *y, const double *z, const double *vy, const double *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<double>(h, IMAGE_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_image_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                   const float *y, const float *z, const float *vy, const float *frac)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_columns<float>(h, IMAGE_AGES_SAMPLES, p, x, y, z, vy, frac, nullptr, nullptr, time);
}

int nxc_image_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count)
{
    if (int rc = pixel_moments_need_set(h, IMAGE_SAMPLES)) return rc;
    return accumulate_rows(h, IMAGE_AGES_SAMPLES, r, first, count);
}

int nxc_image_ages_download(nxc_handle *h, double *sums)
{
    return ages_copy(h, IMAGE_AGES, sums, hipMemcpyDeviceToHost);
}

int nxc_image_ages_upload(nxc_handle *h, const double *sums)
{
    return ages_copy(h, IMAGE_AGES, const_cast<double *>(sums), hipMemcpyHostToDevice);
}

int nxc_image_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out)
{
    return ages_apply(h, IMAGE_AGES, ne, K, out);
}

int nxc_los_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                       int64_t P, const double *x, const double *y, const double *z,
                       const double *vy, const double *frac, const int64_t *index,
                       int64_t n_index, double *radiance, int64_t *npackets, uint8_t *included,
                       int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_PLAIN>(h, d, S, sc, P, x, y, z, decltype(x)(nullptr), vy,
                                         decltype(x)(nullptr), frac, decltype(x)(nullptr), index,
                                         n_index, radiance, npackets, included, used_cap, used_pairs,
                                         n_used);
    });
}

int nxc_los_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                           int64_t P, const float *x, const float *y, const float *z,
                           const float *vy, const float *frac, const int64_t *index,
                           int64_t n_index, double *radiance, int64_t *npackets, uint8_t *included,
                           int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_PLAIN>(h, d, S, sc, P, x, y, z, decltype(x)(nullptr), vy,
                                         decltype(x)(nullptr), frac, decltype(x)(nullptr), index,
                                         n_index, radiance, npackets, included, used_cap, used_pairs,
                                         n_used);
    });
}

int nxc_los_profile_enable(nxc_handle *h, int64_t S, int64_t nv, double v_lo, double v_hi)
{
    return guarded([&]() -> int { return los_profile_enable(h, S, nv, v_lo, v_hi); });
}

int nxc_los_profile_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                               int64_t P, const double *x, const double *y, const double *z,
                               const double *vx, const double *vy, const double *vz,
                               const double *frac, const int64_t *index, int64_t n_index,
                               double *radiance, int64_t *npackets, uint8_t *included,
                               int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_PROFILE>(h, d, S, sc, P, x, y, z, vx, vy, vz, frac,
                                           decltype(x)(nullptr), index, n_index, radiance, npackets,
                                           included, used_cap, used_pairs, n_used);
    });
}

int nxc_los_profile_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                   int64_t P, const float *x, const float *y, const float *z,
                                   const float *vx, const float *vy, const float *vz,
                                   const float *frac, const int64_t *index, int64_t n_index,
                                   double *radiance, int64_t *npackets, uint8_t *included,
                                   int64_t used_cap, int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_PROFILE>(h, d, S, sc, P, x, y, z, vx, vy, vz, frac,
                                           decltype(x)(nullptr), index, n_index, radiance, npackets,
                                           included, used_cap, used_pairs, n_used);
    });
}

int nxc_los_profile_download(nxc_handle *h, double *sums, double *moments)
{
    return guarded([&]() -> int { return los_profile_download(h, sums, moments); });
}

int nxc_los_ages_enable(nxc_handle *h, int64_t S, int64_t na, double t0, double a_lo, double a_hi)
{
    return ages_enable(h, LOS_AGES_BLOCK, S, na, t0, a_lo, a_hi);
}

int nxc_los_ages_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                            int64_t P, const double *time, const double *x, const double *y,
                            const double *z, const double *vy, const double *frac,
                            const int64_t *index, int64_t n_index, double *radiance,
                            int64_t *npackets, uint8_t *included, int64_t used_cap,
                            int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_AGES>(h, d, S, sc, P, x, y, z, decltype(x)(nullptr), vy,
                                        decltype(x)(nullptr), frac, time, index, n_index, radiance,
                                        npackets, included, used_cap, used_pairs, n_used);
    });
}

int nxc_los_ages_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                int64_t P, const float *time, const float *x, const float *y,
                                const float *z, const float *vy, const float *frac,
                                const int64_t *index, int64_t n_index, double *radiance,
                                int64_t *npackets, uint8_t *included, int64_t used_cap,
                                int64_t *used_pairs, int64_t *n_used)
{
    return guarded([&]() -> int {
        return los_accumulate<LOS_AGES>(h, d, S, sc, P, x, y, z, decltype(x)(nullptr), vy,
                                        decltype(x)(nullptr), frac, time, index, n_index, radiance,
                                        npackets, included, used_cap, used_pairs, n_used);
    });
}

int nxc_los_ages_download(nxc_handle *h, double *sums)
{
    return ages_copy(h, LOS_AGES_BLOCK, sums, hipMemcpyDeviceToHost);
}

// ---- RCCL -------------------------------------------------------------------------------------
int nxc_comm_unique_id(uint8_t id[NXC_UNIQUE_ID_BYTES])
{
    static_assert(sizeof(ncclUniqueId) == NXC_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id) return fail(NXC_ERR_ARG, "id is null");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    std::memcpy(id, &u, sizeof u);
    return NXC_OK;
}

int nxc_comm_init(nxc_handle *h, const uint8_t id[NXC_UNIQUE_ID_BYTES], int rank, int nranks)
{
    if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(NXC_ERR_ARG, "bad arguments");
    int rc = rccl_load();
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (h->comm) { g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    const ncclResult_t r = g_rccl.CommInitRank(&h->comm, nranks, u, rank);
    if (r != ncclSuccess) {
        h->comm = nullptr;
        if (r == ncclInvalidUsage || r == ncclInvalidArgument)
            // what RCCL reports when two ranks of the communicator sit on one device
            return fail(NXC_ERR_ARG, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r) +
                                     " -- every rank needs its own GPU (one process per device)");
        return fail(NXC_ERR_RCCL, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
    }
    h->rank = rank;
    h->nranks = nranks;
    h->coll_pending = false;
    h->abort_requested.store(false);
    if (const char *t = std::getenv("NXC_COLLECTIVE_TIMEOUT_S")) {
        const double v = std::atof(t);
        if (v > 0.0) h->coll_timeout_s = v;
    }
    return NXC_OK;
}

int nxc_comm_destroy(nxc_handle *h)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (h->comm && g_rccl.ok) {
        HIPCHK(hipSetDevice(h->device));
        NCCLCHK(g_rccl.CommDestroy(h->comm));
    }
    h->comm = nullptr;
    h->nranks = 1;
    h->rank = 0;
    return NXC_OK;
}

int nxc_comm_set_timeout(nxc_handle *h, double seconds)
{
    if (!h || !(seconds > 0.0)) return fail(NXC_ERR_ARG, "bad arguments");
    h->coll_timeout_s = seconds;
    return NXC_OK;
}

// In front of a collective: the event that separates this process's own queued work from it.
static int mark_collective(nxc_handle *h)
{
    if (!h->coll_pending) {
        if (!h->ev_pre_coll) HIPCHK(hipEventCreateWithFlags(&h->ev_pre_coll, hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ev_pre_coll, h->stream));
    }
    h->coll_pending = true;
    return NXC_OK;
}

int nxc_comm_request_abort(nxc_handle *h)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    h->abort_requested.store(true);
    return NXC_OK;
}

int nxc_comm_test_stall(nxc_handle *h, double seconds)
{
    if (!h || !(seconds >= 0.0) || seconds > 30.0) return fail(NXC_ERR_ARG, "bad arguments");
    if (!h->comm) return fail(NXC_ERR_STATE, "nxc_comm_init has not been called");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = mark_collective(h)) return rc;
    hipLaunchKernelGGL(k_stall, dim3(1), dim3(64), 0, h->stream,
                       (unsigned long long)(seconds * 1e8), (unsigned long long *)nullptr);
    HIPCHK(hipGetLastError());
    return NXC_OK;
}

// A rank that has been told of a peer's failure does not enter another collective.
static int refuse_after_abort_request(nxc_handle *h)
{
    if (!h->abort_requested.load()) return NXC_OK;
    if (h->comm && g_rccl.ok) (void)g_rccl.CommAbort(h->comm);
    h->comm = nullptr;
    h->nranks = 1;
    h->rank = 0;
    h->coll_pending = false;
    return fail(NXC_ERR_RCCL, "a peer rank reported a failure; the communicator was aborted");
}

int nxc_comm_abort(nxc_handle *h)
{
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    if (h->comm && g_rccl.ok) {
        (void)hipSetDevice(h->device);
        (void)g_rccl.CommAbort(h->comm);
    }
    h->comm = nullptr;
    h->nranks = 1;
    h->rank = 0;
    h->coll_pending = false;
    return NXC_OK;
}

int nxc_image_allreduce(nxc_handle *h)
{
    if (!h || !h->have_image) return fail(NXC_ERR_STATE, "nxc_set_image has not been called");
    if (!h->comm) return fail(NXC_ERR_STATE, "nxc_comm_init has not been called");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = refuse_after_abort_request(h)) return rc;
    // one collective: weights and (integer-valued fp64) counts are interleaved in one array
    if (int rc = mark_collective(h)) return rc;
    NCCLCHK(g_rccl.AllReduce(h->img.image, h->img.image, 2 * h->img.npix, ncclFloat64, ncclSum, h->comm,
                             h->stream));
    return NXC_OK;
}

// In-place all-reduce of n host doubles (n small: scalars of the bench, the S radiances + S
// packet counts of a set of lines of sight): staged through device scratch on the handle's stream.
static int allreduce_host(nxc_handle *h, double *values, int64_t n, ncclRedOp_t op)
{
    if (!h || !values || n < 1) return fail(NXC_ERR_ARG, "bad arguments");
    if (!h->comm) return fail(NXC_ERR_STATE, "nxc_comm_init has not been called");
    HIPCHK(hipSetDevice(h->device));
    double *d = h->d_reduce;
    if (n > 1) {
        int rc = h->d_reduce_n.ensure((size_t)n * 8);
        if (rc) return rc;
        d = h->d_reduce_n;
    }
    if (int rc = refuse_after_abort_request(h)) return rc;
    if (int rc = mark_collective(h)) return rc;
    HIPCHK(hipMemcpyAsync(d, values, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    NCCLCHK(g_rccl.AllReduce(d, d, (size_t)n, ncclFloat64, op, h->comm, h->stream));
    HIPCHK(hipMemcpyAsync(values, d, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
}

int nxc_allreduce_max_f64(nxc_handle *h, double *value) { return allreduce_host(h, value, 1, ncclMax); }

int nxc_allreduce_sum_f64(nxc_handle *h, double *value) { return allreduce_host(h, value, 1, ncclSum); }

int nxc_allreduce_f64(nxc_handle *h, double *values, int64_t n)
{
    return allreduce_host(h, values, n, ncclSum);
}

int nxc_barrier(nxc_handle *h)
{
    double v = 0.0;
    return nxc_allreduce_max_f64(h, &v);
}

int nxc_stream_copy_gbs(nxc_handle *h, int64_t bytes, int reps, double *gbs)
{
    return guarded([&]() -> int {
    if (!h || !gbs || bytes < (1 << 20) || reps < 1) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n16 = bytes / 16;
    Dev<char> buf;
    if (int rc = buf.ensure((size_t)n16 * 32)) return rc;
    hipError_t e = hipMemsetAsync(buf, 1, (size_t)n16 * 32, h->stream);
    float best = 0.f;
    hipEvent_t a = nullptr, b = nullptr;
    if (e == hipSuccess) e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    for (int r = 0; r <= reps && e == hipSuccess; r++) {         // first round warms up
        e = hipEventRecord(a, h->stream);
        const int64_t per_block = (int64_t)NXC_BLOCK * NXC_COPY_UNROLL;
        hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)((n16 + per_block - 1) / per_block)),
                           dim3(NXC_BLOCK), 0, h->stream,
                           reinterpret_cast<const nxc_v2d *>(buf.get()),
                           reinterpret_cast<nxc_v2d *>(buf + (size_t)n16 * 16), n16);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(b, h->stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        if (r > 0 && e == hipSuccess && (best == 0.f || ms < best)) best = ms;
    }
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (e != hipSuccess) return fail_hip("stream copy", e);
    *gbs = 2.0 * (double)n16 * 16.0 / ((double)best * 1e-3) / 1e9;      // bytes read + written
    return NXC_OK;
    });
}

int nxc_shader_clock_mhz(nxc_handle *h, double *mhz)
{
    return guarded([&]() -> int {
    if (!h || !mhz) return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const int blocks = h->n_cu, waves = blocks * (BLOCK_PERSIST / 64);
    int rc = scratch_for(h,
                    (size_t)waves * 3 * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *d = reinterpret_cast<unsigned long long *>(h->d_scratch.get());
    std::vector<unsigned long long> got((size_t)waves * 3);
    for (int round = 0; round < 2; round++) {                    // the first brings the clock up
        hipLaunchKernelGGL(k_clock, dim3(blocks), dim3(BLOCK_PERSIST), 0, h->stream, d,
                           round ? 40000 : 400000, 1.0);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(got.data(), d, got.size() * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    std::vector<double> f;
    for (int w = 0; w < waves; w++)
        if (got[3 * (size_t)w + 1] > 0)
            f.push_back((double)got[3 * (size_t)w] / (double)got[3 * (size_t)w + 1] * 100.0);
    if (f.empty()) return fail(NXC_ERR_HIP, "no clock stamps came back");
    std::nth_element(f.begin(), f.begin() + f.size() / 2, f.end());
    *mhz = f[f.size() / 2];
    return NXC_OK;
    });
}

int nxc_pcg64_uniforms(nxc_handle *h, const uint64_t state[2], const uint64_t inc[2], int64_t n,
                       int64_t row0, int64_t count, int32_t nvec, double *out)
{
    return guarded([&]() -> int {
    if (!h || !state || !inc || !out || n < 1 || row0 < 0 || count < 1 || row0 + count > n ||
        nvec < 1 || nvec > NXC_PCG_VECS || n >= ((int64_t)1 << (NXC_PCG_BITS - 1)) || !(inc[1] & 1ull))
        return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    const std::vector<u128> maps = pcg_tables(((u128)inc[0] << 64) | inc[1], n);
    const size_t map_bytes = maps.size() * sizeof(u128), out_bytes = (size_t)nvec * count * 8;
    int rc = scratch_for(h, map_bytes + out_bytes);
    if (rc) return rc;
    unsigned char *base = reinterpret_cast<unsigned char *>(h->d_scratch.get());
    HIPCHK(hipMemcpyAsync(base, maps.data(), map_bytes, hipMemcpyHostToDevice, h->stream));
    PcgK P{};
    P.state = ((u128)state[0] << 64) | state[1];
    P.row0 = row0;
    P.maps = reinterpret_cast<const nxc_u128 *>(base);
    hipLaunchKernelGGL(k_pcg_uniforms, dim3(flat_grid(h, count, NXC_BLOCK)), dim3(NXC_BLOCK), 0,
                       h->stream, P, (int)nvec, count, reinterpret_cast<double *>(base + map_bytes));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, base + map_bytes, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

int nxc_math_batch(nxc_handle *h, int which, int64_t n, const double *in, const double *in2,
                   double *out)
{
    return guarded([&]() -> int {
    if (!h || n < 0 || (n && (!in || !out)) || which < 0 || which > 4 || (which == 4 && !in2))
        return fail(NXC_ERR_ARG, "bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (n == 0) return NXC_OK;
    const size_t col = (size_t)n * sizeof(double);
    int rc = scratch_for(h, 3 * col);
    if (rc) return rc;
    double *d = h->d_scratch;
    HIPCHK(hipMemcpyAsync(d, in, col, hipMemcpyHostToDevice, h->stream));
    if (in2) HIPCHK(hipMemcpyAsync(d + n, in2, col, hipMemcpyHostToDevice, h->stream));
    if (!h->d_blob && (rc = upload_blob(h, h->have_image))) return rc;   // the header with nxc_log's table
    hipLaunchKernelGGL(k_math, dim3(flat_grid(h, n, 256)), dim3(256), NXC_HEADER_BYTES, h->stream,
                       h->d_blob, which, n, d, d + n, d + 2 * n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d + 2 * n, col, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

}  // extern "C"

// ---- moon-centred frame ------------------------------------------------------------------------
namespace {

FrameK frame_kernel_args(const nxc_frame_desc *d)
{
    return FrameK{d->omega, d->M[0], d->M[1], d->M[2], d->U[0], d->U[1], d->U[2], d->scale};
}

// k_frame_rows over n rows of the columns C, timed (nxc_last_kernel_ms).  16 bytes a thread and
// column where every column that is used starts on a 16-byte boundary.
template <typename T, typename I>
int launch_frame(nxc_handle *h, const FrameK &F, const FrameCols &C, int64_t n)
{
    auto aligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    bool wide = aligned(C.idx_in) && aligned(C.idx_out);
    for (int c = 0; c < 9; c++) wide = wide && aligned(C.in[c]) && aligned(C.out[c]);
    const int64_t V = 16 / (int64_t)sizeof(T);
    const int64_t threads = wide ? n / V + V : n;
    int rc;
    if ((rc = begin_timed(h))) return rc;
    hipLaunchKernelGGL((k_frame_rows<T, I>), dim3((unsigned)flat_grid(h, threads, NXC_BLOCK)),
                       dim3(NXC_BLOCK), 0, h->stream, F, C, (long long)n, wide ? 1 : 0);
    HIPCHK(hipGetLastError());
    return end_timed(h);
}

// nxc_frame_columns / _f32: the seven columns up, one pass, the six moved ones back
template <typename T, typename I>
int frame_columns(nxc_handle *h, const nxc_frame_desc *d, int64_t p, const T *const in[7], T *out)
{
    return guarded([&]() -> int {
    if (!h) return fail(NXC_ERR_ARG, "null handle");
    std::string why = check_frame_desc(d);
    const void *cols[8] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6], out};
    if (why.empty()) why = check_frame_columns(p, cols);
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    if (p == 0) return NXC_OK;
    HIPCHK(hipSetDevice(h->device));
    // device scratch: 7 columns in | 6 columns out, each 256-byte aligned
    const size_t bytes = (size_t)p * sizeof(T), col = (bytes + 255) & ~size_t(255);
    int rc = scratch_for(h, 13 * col);
    if (rc) return rc;
    unsigned char *base = reinterpret_cast<unsigned char *>(h->d_scratch.get());
    FrameCols C{};
    for (int c = 0; c < 7; c++) {
        HIPCHK(hipMemcpyAsync(base + (size_t)c * col, in[c], bytes, hipMemcpyHostToDevice, h->stream));
        C.in[c] = base + (size_t)c * col;
    }
    for (int c = 1; c < 7; c++) C.out[c] = base + (size_t)(6 + c) * col;
    if ((rc = launch_frame<T, I>(h, frame_kernel_args(d), C, p))) return rc;
    HIPCHK(hipMemcpy2DAsync(out, bytes, base + 7 * col, col, bytes, 6, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(stream_sync(h));
    return NXC_OK;
    });
}

}  // namespace

extern "C" {

int nxc_frame_rows(nxc_handle *h, const nxc_frame_desc *d, const nxc_rows *src, int64_t first,
                   int64_t count, nxc_rows **out)
{
    return guarded([&]() -> int {
    if (!out) return fail(NXC_ERR_ARG, "out is null");
    *out = nullptr;
    if (!h || !src) return fail(NXC_ERR_ARG, "null argument");
    std::string why = check_frame_desc(d);
    if (why.empty()) why = check_frame_range(src->total, first, count);
    if (!why.empty()) return fail(NXC_ERR_ARG, why);
    int rc = rows_check(h, src, first, count);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    nxc_rows *r = nullptr;
    if ((rc = new_rows(h, count, src->f32, &r, "frame rows"))) return rc;
    if (count > 0) {
        const size_t vsz = src->f32 ? 4 : 8;
        FrameCols C{};
        for (int c = 0; c < 9; c++) {
            C.in[c] = static_cast<const char *>(src->d_cols) + ((size_t)c * src->total + first) * vsz;
            C.out[c] = static_cast<char *>(r->d_cols) + (size_t)c * count * vsz;
        }
        C.idx_in = static_cast<const char *>(src->d_index) + (size_t)first * vsz;
        C.idx_out = r->d_index;
        const FrameK F = frame_kernel_args(d);
        rc = src->f32 ? launch_frame<float, int>(h, F, C, count)
                      : launch_frame<double, long long>(h, F, C, count);
        const hipError_t e = rc ? hipSuccess : stream_sync(h);
        if (rc || e != hipSuccess) {
            nxc_rows_free(h, r);
            return rc ? rc : fail_hip("frame rows", e);
        }
    }
    *out = r;
    return NXC_OK;
    });
}

int nxc_frame_columns(nxc_handle *h, const nxc_frame_desc *d, int64_t p, const double *t,
                      const double *x, const double *y, const double *z, const double *vx,
                      const double *vy, const double *vz, double *out)
{
    const double *const in[7] = {t, x, y, z, vx, vy, vz};
    return frame_columns<double, long long>(h, d, p, in, out);
}

int nxc_frame_columns_f32(nxc_handle *h, const nxc_frame_desc *d, int64_t p, const float *t,
                          const float *x, const float *y, const float *z, const float *vx,
                          const float *vy, const float *vz, float *out)
{
    const float *const in[7] = {t, x, y, z, vx, vy, vz};
    return frame_columns<float, int>(h, d, p, in, out);
}

}  // extern "C"
