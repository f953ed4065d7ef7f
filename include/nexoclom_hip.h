/* nexoclom_hip.h -- C ABI of libnexoclom_hip.so: nexoclom's particle_tracking + image hot path
 * on AMD MI355X (gfx950).
 *
 * The reference (mburger-stsci/nexoclom, pure Python/NumPy) has no FFI on this path; its "plugin
 * boundary" is a set of plain Python call sites.  Each entry point below replaces one of them and
 * is what a ctypes binding inside the reference would call (INTEGRATION.md shows the stubs).
 * Citations are paths under the reference tree's nexoclom/ directory.
 *
 *   nxc_state              state(x, output)                       particle_tracking/state.py:17-74
 *   nxc_rk5_step           rk5(output, X0, h)                     particle_tracking/rk5.py:21-54
 *   nxc_integrate_const    Output.constant_step_size_driver()     particle_tracking/Output.py:368-455
 *                          (+ optionally fused ModelImage.create_image of every stored step)
 *   nxc_integrate_const_rows / nxc_rows_fetch / nxc_rows_build
 *                          the same driver followed by save()'s   particle_tracking/Output.py:523-543
 *                          frac > 0 row filter and 32-bit cast;
 *                          the rows can stay on the device for
 *                          nxc_image_accumulate_rows /
 *                          nxc_los_accumulate_rows
 *   nxc_integrate_var      Output.variable_step_size_driver()     particle_tracking/Output.py:221-366
 *   nxc_image_accumulate   ModelImage.create_image()              data_simulation/ModelImage.py:229-274
 *                          + ModelResult.packet_weighting()       data_simulation/ModelResult.py:140-170
 *                          + Histogram2d()                        math/histogram.py:28-39
 *   nxc_image_allreduce    the per-output-file image sum          data_simulation/ModelImage.py:96-98
 *   nxc_los_accumulate     compute_iteration() inner work          data_simulation/compute_iteration.py:138-217
 *   nxc_set_bounce         bouncepackets() inside the drivers     particle_tracking/bouncepackets.py:5-100
 *   nxc_packets_sample     surface/speed/angular_distribution()   initial_state/source_distribution.py:37-283
 *   nxc_set_bodies         (extension) moons + plasma-torus loss  equations: particle_tracking/state.py:5-10
 *
 * Conventions
 *   - Every function returns 0 on success or a negative nxc_status; nothing is thrown across the
 *     boundary.  nxc_last_error_string() describes the last failure on the calling thread.
 *   - All array arguments are caller-owned HOST buffers, C-contiguous, fp64 unless stated; no
 *     pointer is retained after the call returns, except the table pointers inside nxc_forces /
 *     nxc_image_desc, which are copied to the device during nxc_set_forces / nxc_set_image.
 *   - Packet arrays are struct-of-arrays: soa[c*n + i], column c = 0..7 =
 *     t_remaining, x, y, z, vx, vy, vz, frac (the reference's (N,8) row layout, transposed);
 *     lengths in planet radii, times in seconds.
 *   - A handle owns one device, one HIP stream, its tables, a resident packet set and a resident
 *     image pair.  One host thread per handle; calls are synchronous unless named *_async.
 *   - The reference's asserts (Output.py:254,284,287,388-389; rk5.py:52) become counters
 *     (nxc_counters) that the Python shim turns back into AssertionError.
 */
#ifndef NEXOCLOM_HIP_H
#define NEXOCLOM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: nxc_source_desc grew (tabulated speeds, surface maps, generator), resident row stores
 * 3: bounded waits on collectives (nxc_comm_set_timeout / _abort / _request_abort), nxc_allreduce_f64,
 *    nxc_packets_upload_pieces, nxc_counters.wave_trips, NXC_ERR_NOMEM / NXC_ERR_INCOMPLETE */
#define NXC_ABI_VERSION 3
#define NXC_MAX_LINES 4

typedef enum {
    NXC_OK = 0,
    NXC_ERR_HIP = -1,        /* a HIP runtime call failed (message has the HIP error)   */
    NXC_ERR_ARG = -2,        /* invalid argument / missing prerequisite call            */
    NXC_ERR_NO_DEVICE = -3,  /* no gfx950-class device visible                          */
    NXC_ERR_RCCL = -4,       /* librccl missing or a collective failed                  */
    NXC_ERR_STATE = -5,      /* handle not in the state the call needs                  */
    NXC_ERR_NOMEM = -6,      /* device memory: an allocation failed or the result would
                                not fit (callers may split the work and call again)     */
    NXC_ERR_INCOMPLETE = -7, /* nxc_synchronize after nxc_integrate_const_streamed: the
                                kernel gave up waiting for its queue; results are partial */
    NXC_ERR_OVERFLOW = -8    /* a device pair list (nxc_pairs) was too small for the pairs
                                a pass found; nothing was truncated silently            */
} nxc_status;

/* Scalars and table consumed by state() (what Output.__init__ hangs on `output`,
 * particle_tracking/Output.py:105-128). */
typedef struct nxc_forces {
    double GM;          /* R^3/s^2; NEGATIVE as in the reference (solarsystem/SSObject.py:53)    */
    double vrplanet;    /* R/s, radial velocity of the planet w.r.t. the Sun                     */
    double photo;       /* 1/s, loss_info.photo (state.py:48-52); used when has_photo            */
    double lifetime;    /* s; > 0 selects the constant loss rate 1/lifetime (state.py:44-46)     */
    int32_t gravity;    /* inputs.forces.gravity                                                 */
    int32_t radpres;    /* inputs.forces.radpres                                                 */
    int32_t has_photo;  /* loss_info.photo is not None                                           */
    int32_t reserved;
    int64_t n_tab;      /* radiation-acceleration table length (>= 2)                            */
    const double *v_tab;/* R/s, strictly ascending  (radpres.velocity)                           */
    const double *a_tab;/* R/s^2                    (radpres.accel)                              */
} nxc_forces;

/* Everything create_image needs besides the packets (ModelImage.py:53-78,229-269). */
typedef struct nxc_image_desc {
    double M[9];          /* row-major sun->observer rotation (ModelImage.image_rotation)        */
    double vrplanet;      /* R/s, added to vy for the g-value lookup (ModelImage.py:242-243)     */
    double apix_cm2;      /* pixel area in cm^2; weights are divided by it (ModelImage.py:262)   */
    int32_t quantity;     /* 0 = column/density (w = frac), 1 = radiance/difrad                  */
    int32_t n_lines;      /* number of g-value tables summed for radiance (<= NXC_MAX_LINES)     */
    int32_t downcast_f32; /* 1: round x,y,z,vy,frac through float32 first, as the reference's
                             save()/restore() pair does (Output.py:528-543,555-570)              */
    int32_t reserved;
    int64_t nx, nz;       /* image dims (bins along x_obs, z_obs)                                */
    const double *xedges; /* nx+1 bin edges = np.linspace(lo, hi, nx+1)                          */
    const double *zedges; /* nz+1 bin edges                                                      */
    int64_t line_n[NXC_MAX_LINES];
    const double *line_v[NXC_MAX_LINES]; /* R/s ascending (gValue.velocity converted)            */
    const double *line_g[NXC_MAX_LINES]; /* 1/s           (gValue.g)                             */
} nxc_image_desc;

/* Work and assertion counters of the last integrate / image call on the handle. */
typedef struct nxc_counters {
    uint64_t particle_steps; /* rk5 steps taken = sum over iterations of active packets          */
    uint64_t samples;        /* packet samples offered to the image (frac > 0 records)           */
    uint64_t samples_binned; /* of those, inside the image range                                 */
    uint64_t nonfinite;      /* non-finite state / errmax / weight events; impacts without a finite
                                re-emission (on the polar axis, at rest inside the planet), whose
                                packets are absorbed where they are (nxc_set_bounce)              */
    uint64_t bad_step;       /* step size <= 0 or not finite (variable driver)                   */
    uint64_t neg_frac;       /* accepted step with frac < 0 (variable driver, Output.py:287)     */
    uint64_t unfinished;     /* packets stopped by max_steps before reaching their end time      */
    uint64_t wave_trips;     /* measurement, not a result: trips of a wave through the persistent
                                step loop (64 lanes each); particle_steps / (64 wave_trips) is the
                                share of lanes that held a live packet.  Depends on scheduling. */
} nxc_counters;

typedef struct nxc_handle nxc_handle;

/* ---- device / library ------------------------------------------------------------------------ */
int nxc_abi_version(void);
int nxc_device_count(int *count);
const char *nxc_last_error_string(void);
int nxc_create(int device, nxc_handle **out);
int nxc_destroy(nxc_handle *h);
int nxc_device_name(nxc_handle *h, char *buf, int buflen);
int nxc_device_bus_id(nxc_handle *h, char *buf, int buflen);  /* PCI bus id, e.g. "0000:05:00.0" */
int nxc_synchronize(nxc_handle *h);
int nxc_mem_info(nxc_handle *h, uint64_t *free_bytes, uint64_t *total_bytes);  /* device memory */

/* ---- set-up ---------------------------------------------------------------------------------- */
int nxc_set_forces(nxc_handle *h, const nxc_forces *f);
int nxc_set_image(nxc_handle *h, const nxc_image_desc *d);   /* also zeroes the resident image    */

/* ---- f-2: surface re-emission (particle_tracking/bouncepackets.py:39-100) --------------------------
 * With a bounce description set, a packet that ends a step inside the planet is moved back to its
 * impact point and re-emitted (isotropic rebound, energy accommodation to the local surface
 * temperature through the v(T, probability) spline, sticking loss) instead of being absorbed
 * (Output.py:398-402).  NULL restores perfect sticking.  Random numbers are Philox draws keyed
 * by (seed; first_index + packet row, bounce number): statistically the reference's process.
 * tx[nx], ty[ny], coef[(nx-4)*(ny-4)]: knots/coefficients of scipy's RectBivariateSpline
 * (SurfaceInteraction.py:56) in km/s; ignored when accomfactor == 0.
 * Sticking law (temp_dependent): 0 the constant stickcoef, 1 clip(A0 exp(A1 T) + A2, 0, 1) at the
 * local surface temperature, 2 the surface map of nxc_set_stick_map at the impact point (the
 * inputfiles' sticktype = surface map, which the reference documents and never wrote); frac is
 * multiplied by 1 - coefficient.  The two calls may come in either order; a launch with law 2 and
 * no map returns NXC_ERR_STATE and leaves the handle usable. */
typedef struct nxc_bounce_desc {
    double GM;            /* R^3/s^2 (negative), for the impact speed (bouncepackets.py:59)      */
    double unit_km;
    double accomfactor;   /* 0 = elastic rebound at the impact speed                            */
    double stickcoef;     /* constant sticking (used when temp_dependent == 0)                  */
    double A[3];          /* temperature-dependent sticking A0 exp(A1 T) + A2                   */
    double t0, t1;        /* surface temperature: t0 night, t0 + t1 |cos lon cos lat|^0.25 day  */
    int32_t temp_dependent; /* sticking law: 0 constant, 1 temperature, 2 surface map            */
    int32_t reserved;
    int64_t nx, ny;
    const double *tx, *ty, *coef;
    uint64_t seed;
} nxc_bounce_desc;

/* NULL: back to perfect sticking.  With accomfactor != 0 the spline is checked as for
 * nxc_packets_sample speed_type 3 (finite, non-decreasing knots that increase inside
 * [t[3], t[n-4]], finite coefficients: NXC_ERR_ARG otherwise, the handle's description unchanged);
 * with accomfactor == 0 it is never evaluated and zero-filled tables of 8 knots will do.
 * Re-emission belongs to the constant-step driver: nxc_integrate_var, nxc_integrate_const_streamed
 * and any launch with bodies set return NXC_ERR_STATE while a description is set. */
int nxc_set_bounce(nxc_handle *h, const nxc_bounce_desc *d);
int nxc_set_first_index(nxc_handle *h, int64_t first_index);  /* RNG counter of resident packet 0 */

/* Sticking coefficient from a surface map (sticking law 2 of nxc_bounce_desc): coef[nlon * nlat],
 * longitude-major, in [0, 1], on the nodes lon[nlon] (rad, strictly increasing within [0, 2 pi);
 * 0 at the sub-solar point, pi/2 at dusk: the solar-fixed longitude atan2(x, -y) of the impact)
 * and lat[nlat] (rad, strictly increasing within [-pi/2, pi/2]); nlat = 0: coef[nlon], a function
 * of longitude only.  At an impact the map is interpolated bilinearly: periodic in longitude (the
 * interval from lon[nlon-1] to lon[0] + 2 pi closes the circle), clamped to the end nodes in
 * latitude; with wl, wt the fractions of the cell (i, j),
 *   S = (S[i][j] (1 - wl) + S[i+1][j] wl) (1 - wt) + (S[i][j+1] (1 - wl) + S[i+1][j+1] wl) wt,
 * evaluated in that order, one rounding per operation.  The arrays are copied to the device.
 * NULL clears the map.  Fewer than 2 (or more than 65536) nodes on an axis, nodes out of order or
 * range, or a coefficient that is not a number in [0, 1]: NXC_ERR_ARG, the handle unchanged.
 * nxc_set_bounce(h, NULL) does not clear the map, and a map without law 2 is ignored. */
typedef struct nxc_stick_map_desc {
    int64_t nlon, nlat;
    const double *lon, *lat, *coef;
} nxc_stick_map_desc;
int nxc_set_stick_map(nxc_handle *h, const nxc_stick_map_desc *d);

/* ---- f-4 (tail): moons and plasma-torus loss ---------------------------------------------------
 * EXTENSION -- no reference implementation exists: particle_tracking/state.py:5-10 documents
 * the multi-body equations of motion, :56-70 holds the commented charge-exchange stub, and
 * Output.py:153-155 asserts 'Not set up' for planets with moons.  Parity is therefore against
 * oracle/ only ("parity unpinned"); tests/ add physics checks (Jacobi integral, limits).
 *   accel += sum_m gm[m] (r - r_m(t)) / |r - r_m(t)|^3
 *   loss  += chx_k0 exp(-((rho - chx_rho0)/chx_width)^2 - (z/chx_height)^2)
 *            [* |v - chx_omega z^ x r| / (chx_omega chx_rho0)   when chx_omega > 0]
 *   a packet within radius[m] of moon m after a step is absorbed.
 * Moon m moves on a circle of radius a[m] in the planet's equatorial (x, y) plane; its orbital
 * phase is phi[m] at t_remaining = 0 (geometry.phi: 0 = superior conjunction (+y), pi/2 = over
 * the dawn terminator (-x), docs/nexoclom/inputfiles.rst:72-77) and phi[m] - omega[m] t at
 * t_remaining = t:  r_m = a (-sin, cos, 0).  At stage n (Dormand-Prince node c_n) of step k the
 * phase is evaluated as theta_k + delta_n, theta_k = phi - omega (t0 - k h), delta_n = omega c_n h,
 * with sin/cos of the sum formed from the two sincos() pairs by the angle-addition formulas (that
 * is the definition; the oracles follow it to the bit).  Applies to nxc_integrate_const* only
 * (every packet starts at t_remaining = t0); nxc_state / nxc_rk5_step / nxc_integrate_var and surface
 * re-emission refuse to run while bodies are set.  NULL or n_moons == 0 && !chx_on clears. */
#define NXC_MAX_MOONS 4
typedef struct nxc_bodies_desc {
    int32_t n_moons;
    int32_t chx_on;
    double gm[NXC_MAX_MOONS];      /* R^3/s^2, negative like nxc_forces.GM */
    double radius[NXC_MAX_MOONS];  /* R */
    double a[NXC_MAX_MOONS];       /* R */
    double omega[NXC_MAX_MOONS];   /* rad/s */
    double phi[NXC_MAX_MOONS];     /* rad */
    double t0;                     /* s: t_remaining of every packet at the start of the run */
    double chx_k0;                 /* 1/s */
    double chx_rho0, chx_width, chx_height;   /* R */
    double chx_omega;              /* rad/s; 0 = no dependence on the relative speed */
} nxc_bodies_desc;

int nxc_set_bodies(nxc_handle *h, const nxc_bodies_desc *d);

/* ---- a-2: state() ---------------------------------------------------------------------------- */
int nxc_state(nxc_handle *h, int64_t n, const double *x, const double *y, const double *z,
              const double *vy, double *ax, double *ay, double *az, double *ioniz);

/* ---- a-1: rk5() -- one Dormand-Prince step, per-packet step size h[n] -------------------------
 * soa_out receives the 5th-order state; delta_out (nullable, [8][n]) the reference's
 * |h * sum_{i<6} (b5-b4)_i k_i| error estimate (rk5.py:38-46).
 * Arithmetic: the reference's operations in the reference's order, each rounded once, with two
 * documented departures of at most an ulp -- deterministic r^3 / exp / log (NumPy's own are 1-ulp
 * routines) and the terms of the tableau sums (rk5.py:33-35,41-43), which are fused multiply-adds
 * (one rounding where NumPy has two).  Against rk5.py itself: 1e-13 relative per step. */
int nxc_rk5_step(nxc_handle *h, int64_t n, const double *soa_in, const double *hstep,
                 double *soa_out, double *delta_out);

/* ---- resident packets / image (what a long run keeps in HBM) ----------------------------------- */
int nxc_packets_upload(nxc_handle *h, int64_t n, const double *soa0);
/* The same for a resident set that the host holds in pieces (the Outputs of one launch of
 * Input.run, each an [8][counts[p]] array): piece p's packets follow those of the pieces before it. */
int nxc_packets_upload_pieces(nxc_handle *h, int32_t n_pieces, const int64_t *counts,
                              const double *const *soa);
int nxc_image_clear(nxc_handle *h);
int nxc_image_download(nxc_handle *h, double *image /* nx*nz */, uint64_t *counts /* nx*nz */);
int nxc_counters_get(nxc_handle *h, nxc_counters *out);
int nxc_last_kernel_ms(nxc_handle *h, float *ms);  /* HIP-event time of the last integrate/image launch */

/* ---- f-4: initial states sampled on the device -----------------------------------------------------
 * Fills the resident packet set with n packets of the sources of
 * initial_state/source_distribution.py:37-283 using a counter-based generator (Philox-4x32-10
 * keyed by seed; counter = first_index + i), so shards on different GPUs draw disjoint,
 * reproducible packets.  soa_out (nullable) receives the [8][n] states.  Statistically equivalent
 * to the reference's NumPy sampler, not draw-for-draw.
 *   surface   spatial_type 0  uniform in sin(latitude) and longitude (:47-62)
 *             spatial_type 1  'surface spot' (:96-118): accept/reject on a density map tabulated
 *                             on linspace(0, 2 pi, map_nlon) x linspace(-pi/2, pi/2, map_nlat),
 *                             bilinear between nodes (math/randomdeviates.py:36-83); the device
 *                             runs the trials per packet instead of in rounds of n candidates
 *             spatial_type 2  'surface map' (:63-83), 2-D: the density that is bilinear between
 *                             the nodes map[map_nlon][map_nlat] on linspace(map_lon0, map_lon1) x
 *                             linspace(map_s0, map_s1) in (longitude, sin latitude) -- the law
 *                             random_deviates_2d accepts against -- drawn exactly from three
 *                             uniforms, without a loop: the cell from map_cdf (the cells' masses
 *                             (a + b) + (c + d) of their corner values, cumulated in the order
 *                             i_lon * (map_nlat - 1) + j_lat and divided by the total), then the
 *                             point within the cell by inverting two linear densities.  Every
 *                             packet gets a launch point (no `unfinished`)
 *             spatial_type 3  'surface map', 1-D (:73-77): latitude 0, longitude =
 *                             interp(u, map_cdf, map) with map the even longitude grid [map_nlon]
 *                             and map_cdf its cdf (math/randomdeviates.py:29-33)
 *   speed     speed_type 0/1  flat, gaussian (:141-147,169-171)
 *             speed_type 2    inverse CDF of a tabulated flux density (maxwellian, sputtering;
 *                             :148-168, math/randomdeviates.py:8-33): v = interp(u, speed_cdf,
 *                             speed_v), speed_cdf non-decreasing from 0 to 1
 *             speed_type 3    thermal: a Maxwellian flux at the launch point's surface temperature
 *                             ('maxwellian' at temperature 0, which the reference documents but
 *                             stops at, :165-168).  T = t0 on the night side, t0 + t1
 *                             sqrt(sqrt(|cos lon cos lat|)) within 90 degrees of the sub-solar
 *                             longitude (surface_temperature.py:4-19); v = max(S(T, u), 0) with S
 *                             the bicubic spline (tx[nx], ty[ny], coef[nx-4][ny-4], the
 *                             nxc_bounce_desc layout) of SurfaceInteraction.py:28-61, u the speed
 *                             uniform.  Speed bound of the queue: max |coef| (B-spline bases are
 *                             >= 0 and sum to 1)
 *             speed_type 4    per-node tables of a 2-D surface map (needs spatial_type 2): the
 *                             packet comes from one corner node c of its launch cell (i, j), drawn
 *                             with probability w_c A_c / sum w A -- w the bilinear hat weights at
 *                             the launch point's in-cell coordinates (tx, ty), A the node values
 *                             `map` -- so that the joint law is sum_c w_c A_c p_c and the launch
 *                             points keep the law of spatial_type 2.  Corners in the order (i, j),
 *                             (i, j+1), (i+1, j), (i+1, j+1) with weights (1-tx)(1-ty) a,
 *                             (1-tx) ty b, tx (1-ty) c, tx ty d: the first whose running sum
 *                             exceeds u_corner * total; if rounding leaves none, the last with a
 *                             positive weight; if total is not > 0 (a point on a zero edge), the
 *                             corner with the largest A.  u_corner is the second uniform of Philox
 *                             block 17.  Then v = interp(u, node_speed_cdf[c], node_speed_v), u the
 *                             speed uniform.  Speed bound of the queue: max |node_speed_v|
 *   direction angular_type 0  radial, 1 isotropic (:198-252)
 *             angular_type 2  per-node tables (needs spatial_type 2): altitude =
 *                             interp(u_alt, node_alt_cdf[c], node_alt) and azimuth = interp(u_az,
 *                             node_az_cdf[c], node_az) at the same corner node c as speed_type 4
 *                             (one corner serves all of a packet's per-node draws).  Goes with
 *                             speed_type 0, 1, 2 and 4; with thermal speeds (speed_type 3) it is
 *                             refused (NXC_ERR_ARG): no kernel holds both laws */
typedef struct nxc_source_desc {
    double endtime;        /* s                                                                 */
    double exobase;        /* R                                                                 */
    double sinlat0, sinlat1; /* sin of the latitude range                                       */
    double lon0, lon1;     /* rad; lon1 already += 2 pi when the range wraps                    */
    double vprob, vwidth;  /* km/s: flat = vprob +- vwidth (delv); gaussian = mean, sigma       */
    double unit_km;        /* planet radius                                                     */
    double sinalt0, sinalt1, az0, az1;   /* isotropic launch cone                               */
    int32_t random_time;   /* 1: t = u*endtime (variable-step runs, Output.py:138-139)          */
    int32_t speed_type;    /* 0 flat, 1 gaussian, 2 tabulated, 3 thermal, 4 per-node tables  */
    int32_t angular_type;  /* 0 radial, 1 isotropic, 2 per-node tables                       */
    int32_t is_planet;     /* longitude convention (source_distribution.py:13-28)               */
    uint64_t seed;
    int64_t first_index;
    int32_t spatial_type;  /* 0 uniform, 1 surface spot, 2 surface map, 3 1-D surface map       */
    int32_t reserved;
    int64_t n_speed;       /* speed_type 2: table length (>= 2)                                 */
    const double *speed_cdf;   /* [n_speed] non-decreasing, first 0, last 1                     */
    const double *speed_v;     /* [n_speed] km/s                                                */
    int64_t map_nlon, map_nlat;   /* spatial_type 1, 2: map dims (2..8192 each); 3: map_nlon    */
    const double *map;     /* [map_nlon][map_nlat], >= 0 (3: the longitude grid [map_nlon])     */
    /* generator 1: the reference's own seeded stream, numpy.random.default_rng(seed) = PCG64
     * (Output.py:92), reproduced on the device: the packets are rows pcg_row0 .. pcg_row0 + n - 1
     * of the pcg_n-packet vectors the reference would draw one after the other ([launch time,]
     * sin latitude, longitude, speed, [sin altitude, azimuth]); the uniforms are bit-identical
     * to Generator.random(pcg_n), the states equal the host sampler's to libm rounding.  Only
     * sources whose every draw is such a vector: spatial_type 0, speed_type 0 (flat) or 3
     * (thermal), any angular_type.  pcg_state / pcg_inc: PCG64(seed).state['state'] as {high,
     * low} words.                                                                                */
    int32_t generator;     /* 0 Philox-4x32-10 (counter-based, statistical parity), 1 PCG64     */
    int32_t reserved2;
    uint64_t pcg_state[2], pcg_inc[2];
    int64_t pcg_n, pcg_row0;
    /* dest_total > 0: the n packets are piece [dest_offset, dest_offset + n) of a resident set of
     * dest_total packets that several calls fill (pieces in ascending order, the first with
     * dest_offset 0; the set is usable once the last piece is in).  0: they are the whole set.    */
    int64_t dest_offset, dest_total;
    /* spatial_type 2: [(map_nlon - 1) * (map_nlat - 1)] cumulated cell masses, non-decreasing,
     * last = 1; spatial_type 3: [map_nlon] cdf of the longitude grid, from 0 to 1               */
    const double *map_cdf;
    double map_lon0, map_lon1;   /* spatial_type 2: first and last longitude node, rad          */
    double map_s0, map_s1;       /* spatial_type 2: first and last sin(latitude) node           */
    /* speed_type 3: night-side temperature t0 > 0 and sub-solar excess t1 >= 0, K; the v(T, p)
     * spline [km/s] as in nxc_bounce_desc: knots tx[nx], ty[ny] (non-decreasing, strictly
     * increasing between tx[3] .. tx[nx-4] and ty[3] .. ty[ny-4], nx, ny >= 8), finite
     * coefficients coef[(nx-4) * (ny-4)] row-major                                               */
    double t0, t1;
    int64_t nx, ny;
    const double *tx, *ty, *coef;
    /* speed_type 4 / angular_type 2: one cdf row per node of the 2-D map, [map_nlon * map_nlat][n]
     * row-major with the nodes lon-major (node = i_lon * map_nlat + j_lat), and the axis [n] all
     * rows share (n >= 2, finite).  A row is non-decreasing from 0 to 1; where the node's value in
     * `map` is 0 -- such a node is never drawn -- it may instead be the placeholder of all zeros.
     * Generator 0 only.  The tables are copied to device memory owned by the handle.             */
    int64_t n_node_speed;
    const double *node_speed_cdf, *node_speed_v;     /* speed_type 4; km/s                       */
    int64_t n_node_alt;
    const double *node_alt_cdf, *node_alt;           /* angular_type 2; rad above the horizon    */
    int64_t n_node_az;
    const double *node_az_cdf, *node_az;             /* angular_type 2; rad from north via east  */
} nxc_source_desc;

int nxc_packets_sample(nxc_handle *h, const nxc_source_desc *d, int64_t n, double *soa_out);

/* ---- a-3 (+ fused a-6..a-8): constant-step driver over the resident packets --------------------
 * Runs n_iter iterations of {rk5(step); impact r<1; escape r>outeredge; vanish frac<1e-10}
 * (Output.py:384-431) for every packet until it dies.
 *   flags & NXC_RUN_IMAGE : every stored record with frac > 0 -- the initial state and the state
 *                           after each iteration -- is binned into the resident image with the
 *                           nxc_set_image description (compress=True rule, Output.py:523-524).
 *   traj_out (nullable)   : host [8][nrec][n]; record 0 = initial state, record k = state after
 *                           iteration k, zeros once dead (the reference's `results`, transposed).
 *                           nrec must be >= n_iter+1 when given.
 *   final_out (nullable)  : host [8][n], state at the packet's last processed iteration.
 *   steps_out (nullable)  : host int64[n], iterations the packet was active.
 * The kernel is always the persistent lane-refill integrator.  With traj_out == NULL no trajectory
 * is ever materialised; with traj_out a second pass of the same kernel writes the live records
 * (see nxc_integrate_const_rows) and a layout kernel expands them into the dense array. */
#define NXC_RUN_IMAGE 1u
int nxc_integrate_const(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                        uint32_t flags, double *traj_out, int64_t nrec, double *final_out,
                        int64_t *steps_out);
/* The same trajectories in the form Output.save() keeps them (compress=True, Output.py:523-524):
 * only the records with frac > 0, packet-major (all records of packet 0 in step order, then packet
 * 1, ...), i.e. the row order of the reference's X frame after the frac > 0 filter.  A packet's
 * live records are a prefix of its step axis, so the zero padding of the dense [8][nrec][n] array
 * (typically > 90 % of it) is never materialised or transferred.
 *   nxc_integrate_const_rows : pass 1 (persistent kernel) counts the live records per packet;
 *                              lengths_out int64[n] (nullable), *total_out = their sum.
 *   nxc_rows_fetch           : pass 2 (the same persistent kernel, now writing: a lane owns its
 *                              packet for life, so record k goes to row offset[packet] + k)
 *                              re-integrates and delivers rows_out, host [9][total]: the 8 state
 *                              columns and lossfrac accumulated as (lossfrac + frac_before) -
 *                              frac_after per step (Output.py:420-421), starting from 0 (the
 *                              reference's starts from uninitialised memory, Output.py:378).  Must
 *                              follow nxc_integrate_const_rows on the same resident packets. */
int nxc_integrate_const_rows(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                             int64_t *lengths_out, int64_t *total_out);
int nxc_rows_fetch(nxc_handle *h, double *rows_out);
/* The same rows narrowed to float32 on the device, host [9][total] floats: what save()'s down-cast
 * (Output.py:528-543, which every reference Output ends in, Output.py:202) makes of them, at half
 * the device-to-host bytes. */
int nxc_rows_fetch_f32(nxc_handle *h, float *rows_out);
/* The same rows kept ON THE DEVICE (pass 2 of the protocol above, in place of nxc_rows_fetch): an
 * nxc_rows store holds the nine columns [9][total] plus the packet-index column (row -> number of
 * its packet in the resident set: the reference's X.Index, Output.py:438), as float32 / int32
 * when narrow != 0 (what save() stores, Output.py:528-543) or float64 / int64.  A store outlives
 * the packets it was built from; it is what the reference's per-Output file is to
 * ModelImage / LOSResult (ModelImage.py:85-98, LOSResult.py:264-266), minus the disk and the
 * host.  Stores are freed explicitly; a handle may own any number of them.
 *   nxc_rows_download          rows [first, first + count) -> cols_out host [9][count] (nullable)
 *                              and index_out host [count] (nullable), in the store's types; runs on
 *                              a stream of its own and may be called from a second host thread
 *                              (a file writer) while the handle's thread computes
 *   nxc_image_accumulate_rows  create_image over those rows (columns x, y, z, vy, frac), as
 *                              nxc_image_accumulate[_f32] without the host round trip
 *   nxc_los_accumulate_rows    compute_iteration over those rows, as nxc_los_accumulate[_f32];
 *                              index_shift is subtracted from the store's index column (the first
 *                              packet of the Output the rows belong to) before `included` is set */
typedef struct nxc_rows nxc_rows;
int nxc_rows_build(nxc_handle *h, int narrow, nxc_rows **out);
int nxc_rows_info(const nxc_rows *r, int64_t *total, int32_t *is_f32);
int nxc_rows_download(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count,
                      void *cols_out, void *index_out);
/* Frees the store.  Its two device blocks (when large) are kept by the handle for the next store of
 * about the same size -- hipFree / hipMalloc of tens of GB cost seconds -- and go back to the driver
 * when anything else needs the memory; nxc_mem_info counts them as free. */
int nxc_rows_free(nxc_handle *h, nxc_rows *r);
int nxc_image_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
/* Same launch without any host transfer or synchronisation (bench / pipelining). */
int nxc_integrate_const_async(nxc_handle *h, double step, int64_t n_iter, double outeredge,
                              uint32_t flags);

/* Upload + integrate as one pipelined pass ("incl. H2D of X0"): the n
 * packets of host array soa0 [8][n] are cut into `pieces` (1..32); piece p + 1 crosses PCIe and is
 * put into queue order while piece p is integrated.  Asynchronous like nxc_integrate_const_async
 * (soa0 must stay valid until nxc_synchronize); afterwards the packets are the resident set, the
 * image holds their samples and nxc_counters_get reports the pass.  Same results as
 * nxc_packets_upload + nxc_integrate_const_async (the order of the queue changes no packet).
 * Not with moons or surface re-emission set (NXC_ERR_STATE: upload first).
 * The persistent kernel waits for its pieces while small ordering kernels on a second stream
 * prepare them; where those cannot run beside it (a profiler in counter mode serialises kernels)
 * a wave gives up after three seconds of waiting, the launch ends with part of the packets
 * integrated (nxc_counters.unfinished counts the rest), and the nxc_synchronize that follows
 * returns NXC_ERR_INCOMPLETE: the image and counters are partial, the resident set is dropped, the
 * handle stays usable (nxc_packets_upload + nxc_integrate_const_async is the sequential form). */
int nxc_integrate_const_streamed(nxc_handle *h, int64_t n, const double *soa0, int32_t pieces,
                                 double step, int64_t n_iter, double outeredge, uint32_t flags);

/* ---- a-4: variable-step driver over the resident packets ---------------------------------------
 * final_out host [8][n]; hstore_out (nullable) host [n] = stored step_size column at exit.
 * One persistent launch; the queue is ordered by remaining time over launch speed.  Under 24
 * packets per lane (4.7e6 packets) the waves of a SIMD take turns at issue priority and, once the
 * queue is drained, sparse waves hand their live packets to one wave per SIMD; above it the plain
 * form: same arithmetic, same bits (the environment variable NXC_TEST_VAR_VARIANT = "fair" /
 * "plain" forces either, for tests).  Returns NXC_ERR_STATE, leaving the handle usable, while
 * bodies (nxc_set_bodies) or surface re-emission (nxc_set_bounce) are set: the reference has
 * neither in this driver (Output.py:312-315). */
int nxc_integrate_var(nxc_handle *h, double resolution, double outeredge, int64_t max_steps,
                      double *final_out, double *hstore_out);
/* The same launch (same checks, queue order and kernel) with the finals left ON THE DEVICE: [8][n]
 * fp64 and the stored step in the handle's scratch, where they stay until the next call that
 * uploads or samples packets, integrates, or takes the scratch (nxc_state, nxc_rk5_step, a
 * line-of-sight pass, ...).  Only hstore_out (nullable, host [n]) crosses to the host; the counters
 * come through nxc_counters_get.
 *   nxc_var_rows_build  the row store of that run, in nxc_rows_build's layout (every *_rows entry
 *                       point takes it): one row per kept packet, in packet order; the eight state
 *                       columns are the finals, lossfrac is 0 (this driver never accumulates it,
 *                       Output.py:328-329) and the index column is the packet's number in the
 *                       resident set.  compress != 0 keeps a packet iff its fp64 frac > 0 -- save()'s
 *                       filter on the 64-bit frame (Output.py:523-524), applied before narrowing: a
 *                       frac that underflows in float32 is kept; NaN, +-0 and negative ones are
 *                       dropped; compress == 0 keeps every packet.  narrow != 0 stores float32 /
 *                       int32 (round to nearest even, overflow to inf: numpy's astype), else
 *                       float64 / int64.  kept_out (nullable, host [n]): 1 where the packet has a
 *                       row.  A store of no rows is valid.  May be called more than once per run.
 *                       NXC_ERR_STATE, leaving the handle usable, unless the finals of an
 *                       nxc_integrate_var_resident over the current resident packets are still in
 *                       the scratch.  nxc_last_kernel_ms then spans its two passes. */
int nxc_integrate_var_resident(nxc_handle *h, double resolution, double outeredge,
                               int64_t max_steps, double *hstore_out);
int nxc_var_rows_build(nxc_handle *h, int narrow, int compress, nxc_rows **out, uint8_t *kept_out);

/* ---- a-6..a-8: image of p stored samples -------------------------------------------------------
 * Adds to the resident image pair (use nxc_image_clear / nxc_image_download around it). */
int nxc_image_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                         const double *z, const double *vy, const double *frac);
/* The same for samples in the 32-bit form Output.save() stores them in (Output.py:528-543): what
 * restore()'s up-cast (Output.py:555-570) followed by nxc_image_accumulate gives, bit for bit,
 * with half the host-to-device bytes and no 64-bit copy on the host. */
int nxc_image_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                             const float *z, const float *vy, const float *frac);
/* How the image calls above (and nxc_image_accumulate_rows) add their samples to the image:
 * mode 1 = one global atomic pair per binned sample (k_image); mode 2 = LDS-privatised tiles
 * (k_image_bin + k_image_tiles: the samples are filed by image tile first, a workgroup sums a tile
 * in LDS and hands it over once -- the replacement of np.histogram2d's bincount,
 * math/histogram.py:34, at HBM speed instead of atomic-request speed); mode 0 (default) = tiles for
 * 2^17 samples and more when the image fits them (up to 32 tiles of 8192 pixels: 512 x 512),
 * atomics otherwise.  Packet counts are identical either way, weight sums equal to the order of
 * fp64 additions.  tile_pixels: 0 = 8192; slab_samples: 0 = 2^28, the samples that go through the
 * two passes at a time (their chunk scratch is 10 bytes per sample at worst); smaller values of
 * both exist for tests (more tiles on a small image, several slabs of a small sample set). */
int nxc_image_mode(nxc_handle *h, int mode, int tile_pixels, int64_t slab_samples);

/* ---- f-1: spacecraft line-of-sight cones ----------------------------------------------------------
 * For each of S spectra (spacecraft position + boresight) sum weight/Apix over the stored samples
 * inside the view cone of half-angle dphi, in front of the planet cut-off, that the reference's
 * KD-tree ball pre-selection would have offered (compute_iteration.py:164-185), with the shadow test
 * at the line-of-sight foot point (:202-206).  All angles/trig values are computed by the caller
 * (NumPy) so that thresholds are the reference's own:
 *   sc            host [8][S]: x, y, z, xbore, ybore, zbore, dist_from_plan (1e30 if the LOS misses
 *                 the planet, :105-115), ladder length K_i (as a double)
 *   ladder        t_k = t_{k-1} (1 + sin dphi), t_0 = sin dphi, the longest of the S ladders (:164-167)
 *   cos_threshold smallest double c with arccos(c) <= dphi
 * Outputs: radiance[S] (fp64 sum), npackets[S], included[n_index] (nullable: set to 1 for every
 * packet index seen in a cone, :191), used_pairs (nullable, [2][used_cap]: spectrum, sample row of
 * every pair with weight > 0, :210) and *n_used (pairs found; may exceed used_cap). */
typedef struct nxc_los_desc {
    double dphi, sin_dphi, sin_2dphi, cos_threshold;
    double vrplanet;      /* R/s                                                                   */
    double unit_cm;       /* planet radius in cm: Apix = pi (d sin dphi)^2 unit_cm^2               */
    int32_t n_lines;      /* g-value tables summed (radiance is the only quantity the reference has
                             here, compute_iteration.py:198-213)                                   */
    int32_t reserved;
    int64_t line_n[NXC_MAX_LINES];
    const double *line_v[NXC_MAX_LINES];
    const double *line_g[NXC_MAX_LINES];
    int64_t n_ladder;
    const double *ladder;
} nxc_los_desc;

int nxc_los_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                       int64_t P, const double *x, const double *y, const double *z,
                       const double *vy, const double *frac, const int64_t *index,
                       int64_t n_index, double *radiance, int64_t *npackets, uint8_t *included,
                       int64_t used_cap, int64_t *used_pairs, int64_t *n_used);
/* The same for sample columns in the 32-bit form Output.save() stores (Output.py:528-543); the
 * device widens them exactly as restore() would (Output.py:555-570). */
int nxc_los_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                           int64_t P, const float *x, const float *y, const float *z,
                           const float *vy, const float *frac, const int64_t *index,
                           int64_t n_index, double *radiance, int64_t *npackets,
                           uint8_t *included, int64_t used_cap, int64_t *used_pairs,
                           int64_t *n_used);

int nxc_los_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                            const nxc_rows *r, int64_t first, int64_t count, int64_t index_shift,
                            int64_t n_index, double *radiance, int64_t *npackets,
                            uint8_t *included, int64_t used_cap, int64_t *used_pairs,
                            int64_t *n_used);

/* ---- ModelDensity: number density at points ------------------------------------------------------
 * data_simulation/ModelDensity.py:56-85: for each of Q query points, the frac sum and the number of
 * stored samples within dr of it, summed over any number of accumulate calls.  The points come
 * indexed (ModelDensity.DensityIndex): sorted by the cell of a uniform grid of edge h >= dr (1 +
 * 2^-20) with origin `origin` and dims[3] cells (at most 2^24 in all), cell (cx, cy, cz) =
 * floor((q - origin) * (1/h)) per axis, linear cell (cz * ny + cy) * nx + cx, its points
 * cell_start[c] .. cell_start[c + 1] - 1 of `points` (cell_start[0] = 0, cell_start[ncells] = Q).
 * A sample at p counts for point q iff, with d = q - p in fp64, (dx*dx + dy*dy) + dz*dz <= dr*dr
 * (KDTree.query_ball_point's set).
 *   nxc_density_set              copies the index to the device and zeroes the resident sums
 *   nxc_density_accumulate[_f32] adds P samples held on the host (x, y, z, frac; float32 ones are
 *                                widened exactly as restore() does, Output.py:555-570)
 *   nxc_density_accumulate_rows  adds rows [first, first + count) of a row store (x, y, z, frac)
 *   nxc_density_download         sum_frac[Q], count[Q], in the index's (sorted) point order */
typedef struct nxc_density_desc {
    double origin[3];
    double h;                 /* cell edge                                                        */
    double dr;                /* ball radius, same unit as the points                             */
    int64_t dims[3];          /* cells along x, y, z                                              */
    int64_t n_points;         /* Q (0 allowed: every accumulate is then a no-op)                  */
    const double *points;     /* host [Q][3], sorted by cell                                      */
    const int32_t *cell_start;/* host [dims[0] * dims[1] * dims[2] + 1]                           */
} nxc_density_desc;

int nxc_density_set(nxc_handle *h, const nxc_density_desc *d);
int nxc_density_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                           const double *z, const double *frac);
int nxc_density_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                               const float *z, const float *frac);
int nxc_density_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_density_download(nxc_handle *h, double *sum_frac, double *count);

/* Velocity moments at the same points (EXTENSION: the reference stops at the density).  Each sample
 * that counts for a point (the membership above) also adds, with f = frac and v = (vx, vy, vz)
 * widened to fp64 as p and frac are, one rounding per operation and no contraction,
 *     m1_a  = f * v_a             a  = x, y, z
 *     m2_ab = (f * v_a) * v_b     ab = xx, yy, zz, xy, xz, yz
 *     ff    = f * f
 * to ten sums per point, kept in that order: m1x m1y m1z m2xx m2yy m2zz m2xy m2xz m2yz ff.  Nothing is
 * filtered: a non-finite frac or velocity makes the sums of the points it counts for non-finite, as
 * a non-finite frac does to sum_frac.  The order of addition is not fixed (device atomics).
 *   nxc_density_moments_enable          after nxc_density_set: on != 0 allocates and zeroes the
 *                                       moment sums of the Q points just set, 0 switches them off;
 *                                       nxc_density_set switches them off again
 *   nxc_density_moments_accumulate[_f32] adds P host samples to {sum_frac, count} AND the ten sums in
 *                                       one pass (float32 ones widened as restore() does)
 *   nxc_density_moments_accumulate_rows the same for rows [first, first + count) of a row store
 *                                       (columns 1..7: x, y, z, vx, vy, vz, frac)
 *   nxc_density_moments_download        sums[Q][10], in the index's (sorted) point order
 * NXC_ERR_STATE names the missing call (nxc_density_set, then the enable); NXC_ERR_ARG for p < 0 or
 * a null column with p > 0; p = 0 or Q = 0 adds nothing.  nxc_density_accumulate* keep adding to
 * {sum_frac, count} only, enabled or not, and nxc_density_download keeps returning that pair. */
int nxc_density_moments_enable(nxc_handle *h, int on);
int nxc_density_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                   const double *z, const double *vx, const double *vy,
                                   const double *vz, const double *frac);
int nxc_density_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                       const float *z, const float *vx, const float *vy,
                                       const float *vz, const float *frac);
int nxc_density_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first,
                                        int64_t count);
int nxc_density_moments_download(nxc_handle *h, double *sums);

/* ---- Density spectrum: speed and flux spectra at the points, seen from a moving spacecraft ---------
 * EXTENSION -- what a neutral mass spectrometer flown through the cloud counts: the atoms that arrive
 * within a cone around its boresight, resolved in arrival speed, in the frame of the spacecraft.
 * Per indexed point q the host hands over a frame record of eight doubles {ux, uy, uz, 0, bx, by, bz,
 * 0}: u the spacecraft velocity [R/s] in the planet-centred model frame of the rows, b a unit
 * boresight.  A spectrum has nv >= 1 speed bins over [s_lo, s_hi) [R/s]; the host forms
 * inv_ds = nv / (s_hi - s_lo) once in fp64; cos_half is the cosine of the cone's half angle; all_sky
 * (0 or 1) switches the cone off.  For a row that counts for point q (the membership of
 * nxc_density_set, unchanged), with p, v and f = frac widened to fp64, one rounding per operation and
 * no contraction:
 *   1. c = v - u, component by component
 *   2. s2 = (cx*cx + cy*cy) + cz*cz;   s = sqrt(s2)          (correctly rounded)
 *   3. a = -((cx*bx + cy*by) + cz*bz)
 *   4. the row is SEEN iff all_sky != 0 || a >= cos_half * s: the direction the atom arrives from,
 *      -c/|c|, lies within the half angle of b.  There is no division.  A NaN fails the comparison:
 *      not seen unless all_sky.
 *   5. t = (s - s_lo) * inv_ds, and the plane is the velocity cube's rule:
 *        k = 0            if t < 0
 *        k = 1 + (int)t   if 0 <= t < nv
 *        k = nv + 1       otherwise: at or above s_hi, or s not a number
 *   6. every such row, seen or not, adds {f, 1} to the point's {sum_frac, count} pair, as
 *      nxc_density_accumulate does
 *   7. a seen row adds {f, f*f} to record q*(nv + 2) + k of plane 0 and {g, g*g}, g = f*s, to the same
 *      record of plane 1, which starts 2*Q*(nv + 2) doubles after plane 0 (formed in 64 bits).
 * Nothing else is filtered: a non-finite value poisons what it reaches, as elsewhere.  Plane 0 is the
 * density per speed bin of the atoms in view, plane 1 their number flux; the second half of a record
 * gives sum^2 / sum-of-squares, the effective number of packets of that bin.  The record index is an
 * int on the device: Q*(nv + 2) must stay below 2^31.  The order of addition is not fixed.
 *   nxc_density_spectrum_enable          after nxc_density_set: allocates and zeroes 2*Q*(nv + 2)
 *                                        16-byte records and uploads frames[Q][8], in the index's
 *                                        (sorted) point order; d == NULL or nv == 0 frees them;
 *                                        nxc_density_set switches the spectrum off again and frees
 *                                        them too (they reach gigabytes on a dense grid).
 *                                        NXC_ERR_ARG, before anything is freed or allocated, unless
 *                                        nv >= 1, s_lo and s_hi finite with 0 <= s_lo < s_hi and a
 *                                        finite width, cos_half finite in [-1, 1], every frame value
 *                                        finite, each |b| within 1e-12 of 1 (not asked with all_sky),
 *                                        n_frames == Q and Q*(nv + 2) < 2^31
 *   nxc_density_spectrum_accumulate[_f32] adds p host samples to {sum_frac, count} AND the spectrum in
 *                                        one pass (float32 ones widened as restore() does)
 *   nxc_density_spectrum_accumulate_rows the same for rows [first, first + count) of a row store
 *   nxc_density_spectrum_download        sums[2][Q][nv + 2][2], the device's own order: plane, point
 *                                        (index order), speed plane (0 below, 1..nv the bins, nv + 1
 *                                        above), {sum, sum of squares}
 * NXC_ERR_STATE names the missing call (nxc_density_set, then the enable); NXC_ERR_ARG for p < 0 or a
 * null column with p > 0; p = 0 or Q = 0 adds nothing.  The spectrum and the moments are independent
 * states of a handle: the spectrum entries add to {sum_frac, count} and the spectrum only, the moments
 * entries to {sum_frac, count} and the moments only, the plain entries to {sum_frac, count} only. */
typedef struct nxc_density_spectrum_desc {
    int64_t nv;               /* speed bins (0: free the spectrum)                                */
    double s_lo, s_hi;        /* [R/s]                                                            */
    double cos_half;          /* cosine of the cone's half angle                                  */
    int32_t all_sky;          /* != 0: no cone, every row within dr is seen                       */
    int32_t reserved;
    int64_t n_frames;         /* records in `frames`: must be Q, the points of nxc_density_set    */
    const double *frames;     /* host [Q][8]: ux uy uz 0 bx by bz 0, in the index's point order   */
} nxc_density_spectrum_desc;

int nxc_density_spectrum_enable(nxc_handle *h, const nxc_density_spectrum_desc *d);
int nxc_density_spectrum_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                    const double *z, const double *vx, const double *vy,
                                    const double *vz, const double *frac);
int nxc_density_spectrum_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                        const float *z, const float *vx, const float *vy,
                                        const float *vz, const float *frac);
int nxc_density_spectrum_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first,
                                         int64_t count);
int nxc_density_spectrum_download(nxc_handle *h, double *sums);

/* ---- Density ages: density per age bin at the points, for a time-varying source rate --------------
 * EXTENSION -- nxc_density_accumulate sums a point's ball over all ages; this keeps the age ("Age
 * cube" says what an age is and why the density is linear in the source's history).  A block has
 * na >= 1 bins over [a_lo, a_hi) seconds of age at the epoch t0, the run's endtime.  The host forms
 * inv_da = na / (a_hi - a_lo) once in fp64.  A row that is a member of point q's ball (the membership
 * of nxc_density_set, unchanged) is filed as follows with f = (double)frac, fp64, one rounding per
 * operation, no contraction (time: the row's first column, widened when it is float32):
 *   age = t0 - (double)time
 *   u   = (age - a_lo) * inv_da
 *   k = 0                 if u < 0                              (younger than the range)
 *   k = 1 + (int)u        if 0 <= u < na                        (bin (int)u of the range)
 *   k = na + 1            otherwise: at or above a_hi, or time not a number
 * -- the plane of "Age cube" -- and the member row adds
 *   {f, 1}     to point q's {sum_frac, count} pair, as nxc_density_accumulate does
 *   {f, f*f}   to record q*(na + 2) + k of the block.
 *   - Nothing is filtered.  A member with f == 0 adds zeros and is still counted (nxc_density_* count
 *     every member; the image's age cube, where w == 0 adds nothing, differs).  A non-finite f
 *     poisons the record it reaches.
 *   - So the na + 2 planes of a point sum to its sum_frac up to the order of the additions, which is
 *     not fixed.
 *   - time and frac are read only for a row that passed the cell cull.
 *   nxc_density_ages_enable          after nxc_density_set: na >= 1 allocates and zeroes Q*(na + 2)
 *                                    16-byte records (NXC_ERR_NOMEM when they cannot be had), na == 0
 *                                    frees them; nxc_density_set switches the block off again and
 *                                    frees it, as it does the spectrum.  NXC_ERR_ARG, before anything
 *                                    is allocated or freed, for Q < 1, na < 0, t0, a_lo or a_hi not
 *                                    finite, a_lo >= a_hi (or a width that is not finite),
 *                                    Q*(na + 2) >= 2^31
 *   nxc_density_ages_accumulate[_f32] adds p host samples -- five columns, time first -- to
 *                                    {sum_frac, count} AND the block in one pass
 *   nxc_density_ages_accumulate_rows the same for rows [first, first + count) of a row store, whose
 *                                    column 0 is the time
 *   nxc_density_ages_download        sums[Q][na + 2][2] = {f sum, f*f sum}, point (index order), plane
 *                                    0 below, planes 1..na the bins, na + 1 above
 *   nxc_density_ages_upload          the block replaced by sums of that layout
 *   nxc_density_ages_apply           nxc_image_ages_apply over the Q points in place of the pixels:
 *                                    out[ne][Q][2], the same sums in the same order, the same refusals
 * NXC_ERR_STATE names the missing call (nxc_density_set, then the enable), then NXC_ERR_ARG for p < 0,
 * a null column with p > 0 or a null sums; p = 0 adds nothing.  The age block, the moments and the
 * spectrum are independent states of a handle: the ages entries add to {sum_frac, count} and the
 * block only, and the plain, moments and spectrum entries never touch the block. */
int nxc_density_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi);
int nxc_density_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                                const double *y, const double *z, const double *frac);
int nxc_density_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                    const float *y, const float *z, const float *frac);
int nxc_density_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_density_ages_download(nxc_handle *h, double *sums);
int nxc_density_ages_upload(nxc_handle *h, const double *sums);
int nxc_density_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out);

/* ---- CameraImage: perspective image from a position inside or near the cloud ----------------------
 * EXTENSION -- the reference images from infinity only (ModelImage.create_image); this is the same
 * weighting seen by a pinhole (gnomonic) camera at a finite distance.  Samples are x, y, z [R],
 * vy [R/s], frac in the model frame, as nxc_image_accumulate reads them.  The camera: position o
 * (|o| >= 1), row-major orthonormal basis C with rows right, boresight, up, and tangent-plane bin
 * edges uedges[nx + 1], vedges[nz + 1], each np.linspace(-a, a, n + 1) (full field of view
 * 2 atan(a) < 180 degrees per axis).  Per sample, fp64, one rounding per operation, in this order:
 *   1. dx = x - o[0], dy = y - o[1], dz = z - o[2];  radvel = vy + vrplanet
 *      xc = (C[0]*dx + C[1]*dy) + C[2]*dz;  dc = (C[3]*dx + C[4]*dy) + C[5]*dz;
 *      zc = (C[6]*dx + C[7]*dy) + C[8]*dz
 *   2. !(dc > 0): behind the camera, not binned
 *   3. u = xc / dc, v = zc / dc;  ix, iz = the bins of u in uedges and of v in vedges as
 *      np.histogram2d takes them (searchsorted(edges, ., 'right') - 1, the last edge inclusive);
 *      outside either range: not binned.  Pixel = ix * nz + iz.  A sample that is not binned (2 or
 *      3) counts in `nonfinite` iff frac is not finite or radvel is NaN, as outside a ModelImage frame
 *   4. r2 = (dx*dx + dy*dy) + dz*dz;  b = -((o[0]*dx + o[1]*dy) + o[2]*dz);
 *      cx = o[1]*z - o[2]*y, cy = o[2]*x - o[0]*z, cz = o[0]*y - o[1]*x;  c2 = (cx*cx + cy*cy) + cz*cz;
 *      hidden by the unit sphere iff b > 0 && b < r2 && c2 < r2 (the point of the segment camera ->
 *      sample nearest the centre lies inside it, strictly between its ends; division-free): f =
 *      frac * 0, else f = frac.  c2 = |o x p|^2 is |o|^2 r2 - b^2 formed without that difference,
 *      which at a camera distance D cancels two terms of order D^4 to one of order D^2 and has no
 *      correct digit left from D ~ 1e8.  A hidden sample still counts in the packet image
 *      (create_image's inview)
 *   5. quantity 1: f = f * 0 unless (x*x + z*z > 1 + 2^-52) || (y < 0)  (sunlit, as nxc_image_*)
 *   6. w = f (quantity 0) or (f * sum_l interp(radvel, line_v[l], line_g[l])) / 1e6 (quantity 1;
 *      the sum starts with line 0 and adds the others in order); w not finite or radvel NaN:
 *      `nonfinite`, dropped
 *   7. r = sqrt(r2);  foot = ((dc*dc)*dc) / r  -- r^2 dOmega of a tangent-plane pixel, in R^2 per
 *      unit du dv;  w = w / (foot * pix_area_cm2), pix_area_cm2 = du dv unit_cm^2 from the host
 *   8. w not finite: `nonfinite`, dropped; else image[pixel] += w, packets[pixel] += 1
 * (sqrt and / are IEEE-754 correctly rounded.)  The image is a column density [1/cm^2 per packet
 * weight] or a radiance along the pixel's line of sight for uniform emitters at the samples.
 * The camera image is a device buffer of its own: nxc_set_image / nxc_image_* and the calls below
 * never touch each other's image.  Counters (nxc_counters_get) of an accumulate call: samples,
 * samples_binned (step 8 reached), nonfinite.  Moons do not occult.
 *   nxc_camera_set               checks the description (NXC_ERR_ARG: o not finite or inside the
 *                                planet, C not orthonormal to 1e-12, dims outside 1..8192, edges
 *                                not finite / increasing / symmetric, n_lines outside
 *                                0..NXC_MAX_LINES, null tables, pix_area_cm2 not > 0, tables + edges
 *                                beyond the 160 KiB of LDS), copies the tables to the device and
 *                                zeroes the resident camera image
 *   nxc_camera_accumulate[_f32]  adds p samples held on the host (float32 ones are widened exactly)
 *   nxc_camera_accumulate_rows   adds rows [first, first + count) of a row store
 *   nxc_camera_download          image[nx * nz], counts[nx * nz] (either nullable) */
typedef struct nxc_camera_desc {
    double o[3];          /* camera position, R, model frame                                    */
    double C[9];          /* row-major: right, boresight, up                                    */
    double vrplanet;      /* R/s, added to vy for the g-value lookup                            */
    double pix_area_cm2;  /* du * dv * unit_cm^2                                                */
    int32_t quantity;     /* 0 = column (w = frac), 1 = radiance                                */
    int32_t n_lines;      /* g-value tables summed for radiance (<= NXC_MAX_LINES)              */
    int64_t nx, nz;       /* bins along u (right) and v (up), 1..8192                           */
    const double *uedges; /* nx + 1 tangent-plane edges, symmetric about 0                      */
    const double *vedges; /* nz + 1                                                             */
    int64_t line_n[NXC_MAX_LINES];
    const double *line_v[NXC_MAX_LINES]; /* R/s ascending                                       */
    const double *line_g[NXC_MAX_LINES]; /* 1/s                                                 */
} nxc_camera_desc;

int nxc_camera_set(nxc_handle *h, const nxc_camera_desc *d);
int nxc_camera_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                          const double *z, const double *vy, const double *frac);
int nxc_camera_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                              const float *z, const float *vy, const float *frac);
int nxc_camera_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_camera_download(nxc_handle *h, double *image, uint64_t *counts);

/* ---- Pixel moments: Doppler shift, line width and statistical error per pixel ---------------------
 * EXTENSION -- the reference's images hold a brightness and a packet count per pixel.  A sample runs
 * through the image steps unchanged (nxc_image_accumulate: rotation, bins, occultation, shadow,
 * weight; nxc_camera_*: steps 1-8 above).  If it reaches its pixel with a final weight w -- the value
 * added to image[pixel] -- it also contributes the following, all fp64, one rounding per operation,
 * no contraction.
 * Line-of-sight velocity vlos [R/s], planet frame, positive when receding from the observer:
 *   image:   vlos = (M[3]*vx + M[4]*vy) + M[5]*vz        row 1 of the image rotation (the
 *            occultation test y_obs < 0 puts the observer at y_obs -> -inf).  With downcast_f32, vx
 *            and vz take the float32 round trip of the other five values (vy's is the one the image
 *            itself uses).  The same three products whatever M is, so a non-finite vx always counts
 *   camera:  vlos = ((dx*vx + dy*vy) + dz*vz) / r         dx, dy, dz of step 1, r = sqrt(r2) of step
 *            7: the velocity along that sample's own ray, away from the camera
 * Terms:
 *   a  = w*vlos
 *   m1 = a        m2 = a*vlos        m3 = (a*vlos)*vlos        ww = w*w
 * added to four sums per pixel, kept in the order m1 m2 m3 ww.
 *   - A sample with w == 0 (hidden, shadowed, frac == 0, g == 0) adds nothing to the four sums; it is
 *     still counted in the packet image.  vx and vz of such a sample are not read.
 *   - Nothing else is filtered: a non-finite vx or vz makes that pixel's sums non-finite.
 *   - The image pair, the counts and the counters (samples, samples_binned, nonfinite) of a moments
 *     pass are those of the plain pass over the same samples, up to the fp64 addition order of the
 *     image sum.  The order of addition is not fixed (device atomics).
 * With S0 = image[pixel] before any scaling: m1/S0 is the mean line-of-sight velocity (Doppler
 * shift), m2/S0 - (m1/S0)^2 its variance (line width), m3 its third moment, S0^2/ww the effective
 * number of packets, and S0/sqrt(S0^2/ww) the 1-sigma statistical error of S0.
 *   nxc_image_moments_enable            after nxc_set_image: on != 0 allocates and zeroes nx*nz*4
 *                                       doubles (NXC_ERR_NOMEM when they cannot be had), 0 frees
 *                                       them; nxc_set_image switches the moments off again;
 *                                       nxc_image_clear zeroes them with the image while they are on
 *   nxc_image_moments_accumulate[_f32]  adds p host samples to the image pair AND the four sums in one
 *                                       pass, always one atomic pair per request (at most three
 *                                       requests per binned sample), never the tiles of
 *                                       nxc_image_mode
 *   nxc_image_moments_accumulate_rows   the same for rows [first, first + count) of a row store
 *   nxc_image_moments_download          sums[nx*nz][4], pixel index ix*nz + iz
 *   nxc_camera_moments_*                the same five against the camera's own image buffer
 * NXC_ERR_STATE names the missing call (the set first, then the enable); NXC_ERR_ARG for p < 0 or a
 * null column with p > 0; p = 0 adds nothing but still zeroes the counters.  nxc_image_accumulate*
 * and nxc_camera_accumulate* keep adding to the image pair only, moments enabled or not. */
int nxc_image_moments_enable(nxc_handle *h, int on);
int nxc_image_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                 const double *z, const double *vx, const double *vy,
                                 const double *vz, const double *frac);
int nxc_image_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                     const float *z, const float *vx, const float *vy,
                                     const float *vz, const float *frac);
int nxc_image_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_image_moments_download(nxc_handle *h, double *sums);
int nxc_camera_moments_enable(nxc_handle *h, int on);
int nxc_camera_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                  const double *z, const double *vx, const double *vy,
                                  const double *vz, const double *frac);
int nxc_camera_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                      const float *z, const float *vx, const float *vy,
                                      const float *vz, const float *frac);
int nxc_camera_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_camera_moments_download(nxc_handle *h, double *sums);

/* ---- Velocity cube: one image per Doppler bin, a line profile per pixel ---------------------------
 * EXTENSION -- the pixel moments above stop at a line's shift and width; the cube keeps the profile.
 * A cube has nv >= 1 bins over [v_lo, v_hi), in the rows' velocity unit (planet radii per second).
 * The host forms inv_dv = nv / (v_hi - v_lo) once in fp64 and hands it to the device.  A sample
 * that reaches pixel pix with the final weight w -- exactly what is added to image[pix] -- and
 * w != 0 has the line-of-sight velocity vlos of "Pixel moments": for the image row 1 of the rotation
 * (with the float32 round trip under downcast_f32), for the camera (d . v) / r along its own ray.
 * Then, fp64, one rounding per operation, no contraction:
 *   t = (vlos - v_lo) * inv_dv
 *   k = 0                 if t < 0                              (below the range)
 *   k = 1 + (int)t        if 0 <= t < nv                        (bin (int)t of the range)
 *   k = nv + 1            otherwise: at or above v_hi, or vlos not a number
 * and the sample adds {w, w*w} to record pix*(nv + 2) + k.
 *   - A sample with w == 0 adds nothing to the cube; it is still counted in the packet image.  vx and
 *     vz of such a sample are not read.
 *   - Nothing else is filtered: every sample that adds to image[pix] adds the same w to exactly one
 *     plane of that pixel, so the nv + 2 planes of a pixel sum to image[pix] up to the order of the
 *     additions.
 *   - The image pair, the counts and the counters of a cube pass are those of the plain pass.
 *   - The second half of a record gives w_sum^2 / ww_sum, the effective number of packets of that
 *     spectral bin: the profile's error bars.
 *   nxc_image_cube_enable            after nxc_set_image: nv >= 1 allocates and zeroes
 *                                    nx*nz*(nv + 2) 16-byte records (NXC_ERR_NOMEM when they cannot
 *                                    be had), nv == 0 frees them; nxc_set_image switches the cube
 *                                    off again; nxc_image_clear zeroes it with the image while it is
 *                                    on.  NXC_ERR_ARG, before anything is allocated or freed, for
 *                                    nv < 0, v_lo or v_hi not finite, v_lo >= v_hi (or a width that
 *                                    is not finite), nx*nz*(nv + 2) >= 2^31
 *   nxc_image_cube_accumulate[_f32]  adds p host samples to the image pair AND the cube in one pass,
 *                                    one atomic pair per request (at most two requests per binned
 *                                    sample), never the tiles of nxc_image_mode
 *   nxc_image_cube_accumulate_rows   the same for rows [first, first + count) of a row store
 *   nxc_image_cube_download          sums[nx*nz][nv + 2][2] = {w sum, w*w sum}, pixel index
 *                                    ix*nz + iz, plane 0 below, planes 1..nv the bins, nv + 1 above
 *   nxc_camera_cube_*                the same five against the camera's own image buffer
 * NXC_ERR_STATE names the missing call (the set first, then the enable), then NXC_ERR_ARG as for the
 * moments.  The cube and the moments are independent states of a handle: the cube entries add to the
 * image pair and the cube only, the moments entries to the image pair and the moments only, the
 * plain entries to the image pair only. */
int nxc_image_cube_enable(nxc_handle *h, int64_t nv, double v_lo, double v_hi);
int nxc_image_cube_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                              const double *z, const double *vx, const double *vy,
                              const double *vz, const double *frac);
int nxc_image_cube_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                  const float *z, const float *vx, const float *vy,
                                  const float *vz, const float *frac);
int nxc_image_cube_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_image_cube_download(nxc_handle *h, double *sums);
int nxc_camera_cube_enable(nxc_handle *h, int64_t nv, double v_lo, double v_hi);
int nxc_camera_cube_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                               const double *z, const double *vx, const double *vy,
                               const double *vz, const double *frac);
int nxc_camera_cube_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                   const float *z, const float *vx, const float *vy,
                                   const float *vz, const float *frac);
int nxc_camera_cube_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_camera_cube_download(nxc_handle *h, double *sums);

/* ---- ShellMap: density on spherical shells and zenith column per local time ------------------------
 * EXTENSION -- the reference has nothing like it.  Every stored sample is binned into cells of
 * solar-fixed longitude x sin(latitude) x altitude around the planet's centre.  Samples are x, y, z
 * [R], vy [R/s], frac in the model frame, as nxc_image_accumulate reads them.  The grid: nlon
 * longitude bins with lon_edges[nlon + 1] = np.linspace(0, 2 pi, nlon + 1), nlat latitude bands with
 * mu_edges[nlat + 1] = np.linspace(-1, 1, nlat + 1) (uniform in sin(latitude): every cell has the
 * solid angle dlon dmu), and nalt >= 1 altitude bins over [r_lo, r_hi) in planet radii from the
 * centre; the host forms inv_dr = nalt / (r_hi - r_lo) once in fp64.  Per sample, fp64, one rounding
 * per operation, no contraction, in this order:
 *   1. radvel = vy + vrplanet;  r2 = (x*x + y*y) + z*z;  r = sqrt(r2);  mu = z / r
 *   2. lon = atan2(x, -y);  if lon < 0: lon = lon + 2 pi (the double nearest 2 pi, lon_edges[nlon]).
 *      The package's solar-fixed longitude: 0 at the sub-solar point, pi/2 at dusk
 *   3. ix, iz = the bins of lon in lon_edges and of mu in mu_edges as np.histogram2d takes them
 *      (searchsorted(edges, ., 'right') - 1, the last edge inclusive, NaN outside);  cell =
 *      ix * nlat + iz.  A sample outside either axis (r = 0 makes mu a NaN) is not binned; it counts
 *      in `nonfinite` iff frac is not finite or radvel is NaN, as outside a ModelImage frame
 *   4. f = frac;  quantity 1: f = f * 0 unless (x*x + z*z > 1 + 2^-52) || (y < 0)  (sunlit, as
 *      nxc_image_*).  Nothing occults: there is no observer
 *   5. w = f (quantity 0) or (f * sum_l interp(radvel, line_v[l], line_g[l])) / 1e6 (quantity 1; the
 *      sum starts with line 0 and adds the others in order); w not finite or radvel NaN:
 *      `nonfinite`, dropped
 *   6. c = w / r2;  c not finite: `nonfinite`, dropped
 *   7. column[cell] += c, packets[cell] += 1
 *   8. if w != 0:  t = (r - r_lo) * inv_dr;  k = 0 if t < 0,  1 + (int)t if 0 <= t < nalt,  nalt + 1
 *      otherwise (the velocity cube's rule with r in the velocity's place);  {w, w*w} is added to
 *      record cell * (nalt + 2) + k of plane A and {c, c*c} to the same record of plane B
 * (sqrt and / are IEEE-754 correctly rounded.)  lon is the only transcendental value: it decides a
 * bin and enters no sum, so only its bin is part of the definition, for samples whose lon is not
 * within rounding of an edge.  Three atomic requests per binned sample at most; the order of addition
 * is not fixed.  Plane A over a shell's volume is the number density, plane B and column over the
 * cell's solid angle the zenith column: sum_k B[cell][k] = column[cell] up to the order of addition.
 * The shell map owns its device buffers: nxc_set_image / nxc_camera_set and their entries never touch
 * them, nor the calls below theirs.  Counters (nxc_counters_get) of an accumulate call: samples,
 * samples_binned (step 7 reached), nonfinite.
 *   nxc_shell_set               checks the description (NXC_ERR_ARG: nlon or nlat outside 1..8192,
 *                               nalt < 1, r_lo or r_hi not finite, r_lo < 1, r_lo >= r_hi,
 *                               nlon*nlat*(nalt + 2) >= 2^31 records, edges null / not finite / not
 *                               increasing / not spanning [0, 2 pi] and [-1, 1], vrplanet not finite,
 *                               quantity not 0 or 1, n_lines outside 0..NXC_MAX_LINES, null tables,
 *                               tables + edges beyond the 160 KiB of LDS), copies the tables to the
 *                               device and zeroes the resident sums (NXC_ERR_NOMEM when they cannot be
 *                               had)
 *   nxc_shell_accumulate[_f32]  adds p samples held on the host (float32 ones are widened exactly)
 *   nxc_shell_accumulate_rows   adds rows [first, first + count) of a row store
 *   nxc_shell_download          column[nlon*nlat], counts[nlon*nlat], sums[2][nlon*nlat][nalt + 2][2]
 *                               = plane A, plane B, record 0 below r_lo, 1..nalt the bins, nalt + 1 at
 *                               or above r_hi (each nullable)
 * NXC_ERR_STATE before nxc_shell_set; NXC_ERR_ARG for p < 0 or a null column with p > 0; p = 0 adds
 * nothing but still zeroes the counters. */
typedef struct nxc_shell_desc {
    double vrplanet;        /* R/s, added to vy for the g-value lookup                          */
    double r_lo, r_hi;      /* altitude range in R from the centre, 1 <= r_lo < r_hi            */
    int32_t quantity;       /* 0 = column (w = frac), 1 = radiance                              */
    int32_t n_lines;        /* g-value tables summed for radiance (<= NXC_MAX_LINES)            */
    int64_t nlon, nlat;     /* bins in longitude and in sin(latitude), 1..8192                  */
    int64_t nalt;           /* altitude bins, >= 1                                              */
    const double *lon_edges; /* nlon + 1: np.linspace(0, 2 pi, nlon + 1)                        */
    const double *mu_edges;  /* nlat + 1: np.linspace(-1, 1, nlat + 1)                          */
    int64_t line_n[NXC_MAX_LINES];
    const double *line_v[NXC_MAX_LINES]; /* R/s ascending                                       */
    const double *line_g[NXC_MAX_LINES]; /* 1/s                                                 */
} nxc_shell_desc;

int nxc_shell_set(nxc_handle *h, const nxc_shell_desc *d);
int nxc_shell_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                         const double *z, const double *vy, const double *frac);
int nxc_shell_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                             const float *z, const float *vy, const float *frac);
int nxc_shell_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_shell_download(nxc_handle *h, double *column, uint64_t *counts, double *sums);

/* ---- ShellMap moments: bulk velocity, temperature and fluxes per cell and altitude record ----------
 * EXTENSION.  In the same single pass as "ShellMap", every sample that step 8 there files (w != 0)
 * also files its velocity, resolved in the local spherical basis at the sample, under the same
 * record cell * (nalt + 2) + k.  Samples are x, y, z [R], vx, vy, vz [R/s], frac; they are relative
 * to whatever the rows are relative to (a moon, after nxc_frame_rows).  vrplanet is not added to
 * the velocity: it enters radvel for the g-value alone.  cell, k, w and has = (step 7 reached &&
 * w != 0) are exactly those of "ShellMap", and column, packets and planes A and B are filled exactly
 * as there.  Per sample with `has`, fp64, one rounding per operation, no contraction, sqrt and /
 * correctly rounded, in this order:
 *   1. p2 = x*x + y*y;  r2 = p2 + z*z;  r = sqrt(r2);  p = sqrt(p2);  h = x*vx + y*vy
 *   2. v_r = (h + z*vz) / r                  positive is upward
 *   3. v_e = (x*vy - y*vx) / p               positive is toward increasing solar-fixed longitude
 *                                            (lon = atan2(x, -y): 0 at noon, pi/2 at dusk)
 *   4. v_n = (p2*vz - z*h) / (r*p)           positive is northward
 *   5. p2 == 0 (exactly on the polar axis, where east and north are 0/0): nothing more is added
 *   6. u_r = w*v_r, u_e = w*v_e, u_n = w*v_n;  up = v_r > 0 ? u_r : 0;  dn = v_r < 0 ? -u_r : 0
 *   7. twelve sums go to the sample's record of six planes of 16-byte records,
 *      [6][nlon*nlat][nalt + 2][2]:
 *        plane 0  {u_r, u_e}            plane 3  {u_r*v_e, u_r*v_n}
 *        plane 1  {u_n, u_r*v_r}        plane 4  {u_e*v_n, up}
 *        plane 2  {u_e*v_e, u_n*v_n}    plane 5  {up*up, dn*dn}
 * Non-finite vx or vz are not filtered: they reach the sums of their record, as in "Density
 * moments" (a NaN vy makes radvel a NaN and is dropped by step 5 of "ShellMap").  up and dn*dn are
 * continuous at v_r = 0.  Six more atomic requests per filed sample, each made by lanes l and
 * l + 32 of one instruction; a trip of a wave in which no lane files makes none.  The order of
 * addition is not fixed.
 *   nxc_shell_moments_enable          after nxc_shell_set: on != 0 allocates and zeroes the six planes
 *                                     (NXC_ERR_NOMEM when they cannot be had), on == 0 frees them;
 *                                     the next nxc_shell_set switches them off again
 *   nxc_shell_moments_accumulate[_f32] adds p host samples to everything nxc_shell_accumulate adds
 *                                     to AND to the six planes, in one pass
 *   nxc_shell_moments_accumulate_rows the same for rows [first, first + count) of a row store
 *   nxc_shell_moments_download        sums[6][nlon*nlat][nalt + 2][2]
 * NXC_ERR_STATE naming nxc_shell_set before it, then NXC_ERR_STATE "moments not enabled" before the
 * enable; NXC_ERR_ARG for p < 0, a null column with p > 0 or a null `sums`.  nxc_shell_accumulate*
 * and nxc_shell_download serve unchanged beside them and never touch the six planes. */
int nxc_shell_moments_enable(nxc_handle *h, int on);
int nxc_shell_moments_accumulate(nxc_handle *h, int64_t p, const double *x, const double *y,
                                 const double *z, const double *vx, const double *vy,
                                 const double *vz, const double *frac);
int nxc_shell_moments_accumulate_f32(nxc_handle *h, int64_t p, const float *x, const float *y,
                                     const float *z, const float *vx, const float *vy,
                                     const float *vz, const float *frac);
int nxc_shell_moments_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_shell_moments_download(nxc_handle *h, double *sums);

/* ---- ShellMap ages: density and zenith column per age bin, for a time-varying source rate ----------
 * EXTENSION -- nxc_shell_accumulate sums a record over all ages; this keeps the age ("Age cube" says
 * what an age is and why the sums are linear in the source's history).  A block has na >= 1 bins over
 * [a_lo, a_hi) seconds of age at the epoch t0, the run's endtime.  The host forms inv_da =
 * na / (a_hi - a_lo) once in fp64.  Samples are time, x, y, z, vy, frac (time: the row's first column,
 * widened when it is float32).  A sample goes through steps 1 to 7 of "ShellMap" unchanged: column and
 * packets of its cell, the counters, `nonfinite` and the replicas of the pair array are what
 * nxc_shell_accumulate makes them.  If step 8 files the sample (w != 0) under record rec =
 * cell * (nalt + 2) + k, it adds to planes A and B exactly as there, and it forms the plane ka, fp64,
 * one rounding per operation, no contraction:
 *   age = t0 - (double)time
 *   u   = (age - a_lo) * inv_da
 *   ka = 0                if u < 0                              (younger than the range)
 *   ka = 1 + (int)u       if 0 <= u < na                        (bin (int)u of the range)
 *   ka = na + 1           otherwise: at or above a_hi, or time not a number
 * -- the plane of "Age cube" -- and adds
 *   {w, w*w}   to record rec * (na + 2) + ka of age plane A
 *   {c, c*c}   to the same record of age plane B.
 *   - Five atomic requests per filed sample at most, each made from uniform control flow; a trip of
 *     a wave in which no lane files makes none of the four record requests.
 *   - A sample with w == 0, or one that was not binned, adds nothing to the block, and its time is
 *     not read.
 *   - So the na + 2 planes of a record sum to that record of plane A (and of plane B), and age plane
 *     B summed over a cell's nalt + 2 records is the cell's column per age, both up to the order of
 *     the additions, which is not fixed.
 * The block is [2][R][na + 2] 16-byte records, R = nlon*nlat*(nalt + 2), a buffer of its own on the
 * handle.  The age block and the moments are independent states of a shell map.
 *   nxc_shell_ages_enable            after nxc_shell_set: na >= 1 allocates and zeroes the block
 *                                    (NXC_ERR_NOMEM when the two planes cannot be had), na == 0 frees
 *                                    it; nxc_shell_set switches the block off again and frees it, as
 *                                    it does the moments' planes.  NXC_ERR_ARG, before anything is
 *                                    allocated or freed, for na < 0, t0, a_lo or a_hi not finite,
 *                                    a_lo >= a_hi (or a width that is not finite), R*(na + 2) >= 2^31
 *   nxc_shell_ages_accumulate[_f32]  adds p host samples -- six columns, time first -- to everything
 *                                    nxc_shell_accumulate adds to AND to the block, in one pass
 *   nxc_shell_ages_accumulate_rows   the same for rows [first, first + count) of a row store, whose
 *                                    column 0 is the time
 *   nxc_shell_ages_download          sums[2][R][na + 2][2]: age plane A = {w sum, w*w sum}, age plane
 *                                    B = {c sum, c*c sum}; plane 0 below, 1..na the bins, na + 1 above
 *   nxc_shell_ages_upload            the block replaced by sums of that layout
 *   nxc_shell_ages_apply             K[na + 2][ne], out[2][ne][R][2]: per plane nxc_image_ages_apply
 *                                    over the R records in place of the pixels, the same sums in the
 *                                    same order, the same refusals
 * NXC_ERR_STATE names the missing call (nxc_shell_set, then the enable), then NXC_ERR_ARG for p < 0, a
 * null column with p > 0 or a null sums / out; p = 0 adds nothing but still zeroes the counters.
 * nxc_shell_accumulate*, nxc_shell_moments_* and nxc_shell_download serve unchanged beside them and
 * never touch the block. */
int nxc_shell_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi);
int nxc_shell_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                              const double *y, const double *z, const double *vy, const double *frac);
int nxc_shell_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                  const float *y, const float *z, const float *vy, const float *frac);
int nxc_shell_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_shell_ages_download(nxc_handle *h, double *sums);
int nxc_shell_ages_upload(nxc_handle *h, const double *sums);
int nxc_shell_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out);

/* ---- Line-of-sight profile: radiance per Doppler bin along each line of sight ----------------------
 * EXTENSION -- nxc_los_accumulate gives one radiance per spectrum; the profile keeps the line: per
 * spectrum nv >= 1 bins over [v_lo, v_hi), in the rows' velocity unit (planet radii per second), and
 * the four moment sums of "Pixel moments".  A (sample, spectrum) pair is decided exactly as in
 * nxc_los_accumulate.  If it reaches the point where its wtemp = weight/Apix (times 0 when the
 * foot point is in shadow) is added to radiance[spectrum], and wtemp != 0, it also contributes the
 * following, all fp64, one rounding per operation, no contraction:
 *   vlos = (vx*bx + vy*by) + vz*bz       bx, by, bz: the spectrum's boresight as given in sc; the
 *                                        velocity of the sample along it [R/s], planet frame,
 *                                        positive when receding from the spacecraft.  float32
 *                                        columns are widened exactly, as the other columns are
 *   t = (vlos - v_lo) * inv_dv           inv_dv = nv / (v_hi - v_lo), formed once on the host
 *   k = 0                 if t < 0
 *   k = 1 + (int)t        if 0 <= t < nv
 *   k = nv + 1            otherwise: at or above v_hi, or vlos not a number
 * and the pair adds {wtemp, wtemp*wtemp} to record spectrum*(nv + 2) + k (the cube's rule), and
 *   a  = wtemp*vlos
 *   m1 = a        m2 = a*vlos        m3 = (a*vlos)*vlos        ww = wtemp*wtemp
 * to four sums per spectrum, kept in the order m1 m2 m3 ww.
 *   - A pair with wtemp == 0 (foot point in shadow, frac == 0, g == 0) adds nothing to either; it is
 *     still counted in npackets and `included`.  vx and vz of a pair that is not decided, or that has
 *     wtemp == 0, are not read.
 *   - Nothing else is filtered: the nv + 2 records of a spectrum sum to its radiance up to the order
 *     of the additions; a non-finite vx or vz makes that spectrum's moment sums non-finite and
 *     files the pair under nv + 1.
 *   - The spacecraft's own velocity is NOT subtracted: vlos is the planet-frame velocity along the
 *     boresight.  A moving spacecraft shifts every bin of its spectrum by its own velocity along
 *     its boresight; the caller subtracts that.
 *   - radiance, npackets, `included`, the used pairs and the counters of a profile pass are those of
 *     the plain pass over the same samples, up to the fp64 addition order of radiance.
 * With S0 = radiance[spectrum] of the same passes the quotients are those of "Pixel moments".
 *   nxc_los_profile_enable          nv >= 1 allocates and zeroes S*(nv + 2) 16-byte records and S*4
 *                                   doubles (NXC_ERR_NOMEM when they cannot be had), nv == 0 frees
 *                                   them; a second enable replaces and zeroes.  NXC_ERR_ARG, before
 *                                   anything is allocated or freed, for S < 1, nv < 0, v_lo or v_hi
 *                                   not finite, v_lo >= v_hi (or a width that is not finite),
 *                                   S*(nv + 2) >= 2^31
 *   nxc_los_profile_accumulate[_f32], _rows
 *                                   nxc_los_accumulate[_f32], _rows with the vx and vz columns
 *                                   (a row store carries them): everything the plain entry returns,
 *                                   and the pairs' contributions added to the profile.  Sums
 *                                   accumulate over calls.  NXC_ERR_STATE without an enabled
 *                                   profile; NXC_ERR_ARG when S is not the enabled one, or vx or vz is
 *                                   null with P > 0; P == 0 adds nothing
 *   nxc_los_profile_download        sums[S][nv + 2][2] = {wtemp sum, wtemp*wtemp sum}, record 0 below
 *                                   the range, 1..nv the bins, nv + 1 above; moments[S][4]
 * nxc_los_accumulate* never touch the profile, enabled or not. */
int nxc_los_profile_enable(nxc_handle *h, int64_t S, int64_t nv, double v_lo, double v_hi);
int nxc_los_profile_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                               int64_t P, const double *x, const double *y, const double *z,
                               const double *vx, const double *vy, const double *vz,
                               const double *frac, const int64_t *index, int64_t n_index,
                               double *radiance, int64_t *npackets, uint8_t *included,
                               int64_t used_cap, int64_t *used_pairs, int64_t *n_used);
int nxc_los_profile_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                   int64_t P, const float *x, const float *y, const float *z,
                                   const float *vx, const float *vy, const float *vz,
                                   const float *frac, const int64_t *index, int64_t n_index,
                                   double *radiance, int64_t *npackets, uint8_t *included,
                                   int64_t used_cap, int64_t *used_pairs, int64_t *n_used);
int nxc_los_profile_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                    const nxc_rows *r, int64_t first, int64_t count,
                                    int64_t index_shift, int64_t n_index, double *radiance,
                                    int64_t *npackets, uint8_t *included, int64_t used_cap,
                                    int64_t *used_pairs, int64_t *n_used);
int nxc_los_profile_download(nxc_handle *h, double *sums, double *moments);

/* ---- Source maps: where the packets of fitted Outputs came from ---------------------------------
 * data_simulation/make_source_map.py:11-174 per Output, summed over the Outputs of a result on the
 * device.  Grid: nlon x nlat points at the bin centres point_lon[nlon], point_lat[nlat]; point p =
 * i_lon * nlat + j_lat.  Packet q is in point p's ball iff (BallTree haversine query_radius, fp64,
 * one rounding per operation in this order)
 *     sin(0.5*(phi_p - phi_q))^2 + cos(phi_p)*cos(phi_q)*sin(0.5*(lam_p - lam_q))^2 <= threshold[j],
 * with point_cos[j] = cos(phi_p) and threshold[j] = sin(0.5 * smear_radius * cos(phi_p))^2.  The
 * host sorts each Output's packets by cell, lat-major (cell j * nlon + i of the bucket it files them
 * in; cell_start[ncells] may be < n: packets after it are in no ball), and lists for every tile of
 * `tile` consecutive longitudes of one latitude row (tile k covers row k / ceil(nlon / tile)) the
 * cell runs [seg[2s], seg[2s + 1]] (inclusive, s in seg_off[k] .. seg_off[k + 1] - 1) that hold every
 * packet of its points' balls.  Histograms follow np.histogram with `range=`: bins between
 * np.linspace edges, the right edge inclusive, values outside dropped.
 * Map per point: [nvel speed | nalt altitude | naz azimuth | n_total | n_included | weight sum],
 * then hist2d[npoints]: the unsmeared lon/lat histogram (np.histogram2d of the included packets).
 * Included: frac > 0; weight: frac, or 1 when `available`.
 *   nxc_source_map_set         uploads the grid and segments and zeroes the resident map.  A grid
 *                              whose kernels would ask for more than 64 KiB of LDS -- a tile's
 *                              histograms and segment table, 8 * tile * (nvel + nalt + naz + 3) +
 *                              8 * (longest segment list + 1) bytes, or the staged edges and
 *                              whole-planet histograms, 8 * (2 * (nvel + nalt + naz) + nlon + nlat
 *                              + 5) bytes -- is refused (NXC_ERR_ARG, the resident map unchanged)
 *   nxc_source_map_accumulate  adds one Output: n packets' lat, lon, v [R/s], altitude, azimuth,
 *                              frac (sorted), cell_start[ncells + 1], its speed edges [nvel + 1]
 *                              (speed = v * r_km); the speed histograms of the map are added times
 *                              `factor`.  small[nvel + nalt + naz + nvel] receives the Output's
 *                              whole-planet speed, altitude and azimuth histograms and its speed
 *                              map summed over the grid (unscaled)
 *   nxc_source_map_download    map[npoints][nvel + nalt + naz + 3], hist2d[npoints] */
typedef struct nxc_source_map_desc {
    int64_t nlon, nlat, nvel, nalt, naz;
    int64_t tile;             /* grid points per workgroup (<= nlon)                              */
    double r_km;              /* planet radius [km]                                              */
    const double *alt_edges;  /* host [nalt + 1]; az_edges [naz + 1]; lon_edges [nlon + 1];      */
    const double *az_edges;   /* lat_edges [nlat + 1]                                            */
    const double *lon_edges;
    const double *lat_edges;
    const double *point_lon;  /* host [nlon]                                                     */
    const double *point_lat;  /* host [nlat]                                                     */
    const double *point_cos;  /* host [nlat]                                                     */
    const double *threshold;  /* host [nlat]                                                     */
    int64_t n_seg;
    const int32_t *seg;       /* host [n_seg][2]                                                 */
    const int32_t *seg_off;   /* host [ntiles + 1]                                               */
} nxc_source_map_desc;

int nxc_source_map_set(nxc_handle *h, const nxc_source_map_desc *d);
int nxc_source_map_accumulate(nxc_handle *h, int64_t n, const double *lat, const double *lon,
                              const double *v, const double *alt, const double *az,
                              const double *frac, const int32_t *cell_start,
                              const double *vel_edges, int32_t available, double factor,
                              double *small);
int nxc_source_map_download(nxc_handle *h, double *map, double *hist2d);

/* ---- LOSResultFitted: packet weights refitted to observed radiances ------------------------------
 * data_simulation/LOSResultFitted.py:118-214 per Output, over the (spectrum, row) pairs its UNFITTED
 * line-of-sight pass found with weight > 0 (compute_iteration.py:210's `used`).
 *   nxc_pairs_create       a device pair list of `capacity` pairs (the Output's sum of npackets over
 *                          the spectra bounds it: every used pair is a counted one)
 *   nxc_los_set_pairs      the nxc_los_accumulate* calls that follow (until set to NULL) write their
 *                          used pairs into p in place of used_pairs (which must then be NULL): rows
 *                          as numbered in the call's sample range.  More pairs than the capacity:
 *                          NXC_ERR_OVERFLOW (p then holds none that can be trusted)
 *   nxc_pairs_count / nxc_pairs_download   the pairs of the last pass (any order): spectrum, row
 *   nxc_fit_set            per spectrum: position [3][S] (host), ratio_j = data / unfitted model,
 *                          weight_j (weight_mode 3: the reference's 1/sigma*2; nullable otherwise),
 *                          mask_j; zeroes the fitted radiance sums
 *   nxc_fit_source_rows / nxc_fit_source[_f32]   the samples the pairs' rows index: rows
 *                          [first, first + count) of a store (packet = index - index_shift) or P host
 *                          columns x, y, z, vy, frac with their packet index
 *   nxc_fit_packets        per packet i over the pairs with mask_j: num_i = sum ratio_j w,
 *                          den_i = sum w, cnt_i = pairs; w = 1, 1/d, 1/d^2 (weight_mode 0, 1, 2; d as
 *                          the pair test forms it) or weight_j; f_i = num_i / den_i (0 where
 *                          den_i = 0); mult_i = f_i / mean(f over den > 0), the mean in a fixed
 *                          order; all 0 when no packet was seen.  stats: {sum f, packets seen}.
 *                          Outputs nullable; the multipliers stay on the device
 *   nxc_fit_radiance       adds, for every pair (no mask), frac mult_i gg / 1e6 / Apix to its
 *                          spectrum's sum: the weight of nxc_los_accumulate with d's dphi, vrplanet,
 *                          unit and g-value tables (ladder and thresholds unused)
 *   nxc_fit_rows           (store sources) the rows with frac' = frac mult_i in fp64, narrowed to
 *                          the store's type, with compress only those with frac' > 0, in their order,
 *                          as a new store of the same layout; lengths_out[n_packets] (nullable):
 *                          rows kept per packet
 *   nxc_fit_download       the fitted radiance sums [S] */
typedef struct nxc_pairs nxc_pairs;
int nxc_pairs_create(nxc_handle *h, int64_t capacity, nxc_pairs **out);
int nxc_pairs_free(nxc_handle *h, nxc_pairs *p);
int nxc_pairs_count(const nxc_pairs *p, int64_t *n);
int nxc_pairs_download(nxc_handle *h, const nxc_pairs *p, int64_t *spectrum, int64_t *row);
int nxc_los_set_pairs(nxc_handle *h, nxc_pairs *p);

typedef struct nxc_fit_desc {
    int64_t n_spectra;        /* S                                                                */
    int32_t weight_mode;      /* 0 none, 1 'dist', 2 'dist2', 3 'sigma'                            */
    int32_t reserved;
    const double *position;   /* host [3][S]: spacecraft x, y, z                                   */
    const double *ratio;      /* host [S]                                                         */
    const double *weight;     /* host [S] (weight_mode 3)                                          */
    const uint8_t *mask;      /* host [S]                                                         */
} nxc_fit_desc;

int nxc_fit_set(nxc_handle *h, const nxc_fit_desc *d);
int nxc_fit_source_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count,
                        int64_t index_shift);
int nxc_fit_source(nxc_handle *h, int64_t P, const double *x, const double *y, const double *z,
                   const double *vy, const double *frac, const int64_t *index);
int nxc_fit_source_f32(nxc_handle *h, int64_t P, const float *x, const float *y, const float *z,
                       const float *vy, const float *frac, const int64_t *index);
int nxc_fit_packets(nxc_handle *h, const nxc_pairs *p, int64_t n_packets, double *num, double *den,
                    int32_t *cnt, double *mult, double *stats);
int nxc_fit_radiance(nxc_handle *h, const nxc_pairs *p, const nxc_los_desc *d);
int nxc_fit_rows(nxc_handle *h, int compress, nxc_rows **out, int64_t *lengths_out);
int nxc_fit_download(nxc_handle *h, double *radiance);

/* ---- a-9 / multi-GPU: sum of the per-GPU image pairs over RCCL ---------------------------------
 * One process per GPU.  Rank 0 calls nxc_comm_unique_id and hands the 128 bytes to the other
 * ranks (any side channel); every rank then calls nxc_comm_init (NXC_ERR_ARG when RCCL refuses
 * the layout, which is what happens when two ranks share one device).  nxc_image_allreduce sums the
 * resident image and packet counts over all ranks in place (one fp64 all-reduce: the device keeps
 * {weight sum, count} interleaved, counts as integer-valued doubles, exact below 2^53). */
#define NXC_UNIQUE_ID_BYTES 128
int nxc_comm_unique_id(uint8_t id[NXC_UNIQUE_ID_BYTES]);
int nxc_comm_init(nxc_handle *h, const uint8_t id[NXC_UNIQUE_ID_BYTES], int rank, int nranks);
int nxc_comm_destroy(nxc_handle *h);
int nxc_image_allreduce(nxc_handle *h);
int nxc_allreduce_max_f64(nxc_handle *h, double *value);   /* control plane: max-over-ranks timer */
int nxc_allreduce_sum_f64(nxc_handle *h, double *value);   /* control plane: whole-job work counters */
int nxc_barrier(nxc_handle *h);
/* In-place sum over the ranks of n host doubles (the per-file radiance sum of
 * data_simulation/LOSResult.py:264-266 across GPUs: S radiances + S packet counts). */
int nxc_allreduce_f64(nxc_handle *h, double *values, int64_t n);
/* No wait on a collective is unbounded.  nxc_image_allreduce only enqueues; the next call that
 * waits for the handle's stream (nxc_synchronize, a download, the scalar reductions above) polls
 * the stream together with ncclCommGetAsyncError, and when `seconds` have passed (default 120, or
 * the environment's NXC_COLLECTIVE_TIMEOUT_S at nxc_comm_init) -- a peer rank died or never issued
 * its half of the collective -- it calls ncclCommAbort, leaves the handle without a communicator
 * and returns NXC_ERR_RCCL.  The data the collective was to produce are then undefined; the process
 * is expected to report and exit.  nxc_comm_abort does the same on request (a rank that must
 * leave while its peers may already be inside a collective). */
int nxc_comm_set_timeout(nxc_handle *h, double seconds);
int nxc_comm_abort(nxc_handle *h);
/* The one call that may come from ANOTHER thread while the owning thread waits inside the library
 * (the control plane's failure watcher): the wait in progress, or the next collective, ends with
 * NXC_ERR_RCCL at once instead of at the deadline. */
int nxc_comm_request_abort(nxc_handle *h);
/* Fault injection for the tests of the deadline: holds the handle's stream for `seconds` (<= 30;
 * the kernel ends by itself) and marks it as a collective in flight. */
int nxc_comm_test_stall(nxc_handle *h, double seconds);

/* ---- measurement helpers for bench.py's roofline object -------------------------------------------
 * nxc_stream_copy_gbs: best of `reps` device-to-device streaming copies of `bytes` (16 B per lane),
 * GB/s of bytes read + written: the box's own HBM ceiling.  nxc_shader_clock_mhz: the clock the
 * chip holds under an fp64 load, from in-kernel stamps of a diagnostic launch. */
int nxc_stream_copy_gbs(nxc_handle *h, int64_t bytes, int reps, double *gbs);
int nxc_shader_clock_mhz(nxc_handle *h, double *mhz);

/* Diagnostics of generator 1: out[nvec][count] = the uniforms of draws 0..nvec-1 for rows row0 ..
 * row0 + count - 1 of n-packet vectors, i.e. default_rng(seed).random(n)[row0:row0+count] nvec
 * times in a row. */
int nxc_pcg64_uniforms(nxc_handle *h, const uint64_t state[2], const uint64_t inc[2], int64_t n,
                       int64_t row0, int64_t count, int32_t nvec, double *out);

/* ---- diagnostics used by the parity tests -------------------------------------------------------
 * which: 0 = exp, 1 = log, 2 = cube (r^3), 3 = sqrt, 4 = x/y with y = in2 (in2 nullable otherwise) */
int nxc_math_batch(nxc_handle *h, int which, int64_t n, const double *in, const double *in2,
                   double *out);

/* ---- Moon-centred frame: stored rows moved into the frame that co-rotates with a moon -----------
 * EXTENSION -- the reference stops at planets with moons (Output.py:153-155).  A constant-step run
 * stores every step of every packet, and the stored-sample products read a row at t_remaining = t
 * as a packet of age t0 - t seen at the epoch t_remaining = 0.  That steady-state reading holds in
 * a frame in which the source stands still: for a run launched from a moon, the frame that
 * co-rotates with the moon.  Moon m (nxc_bodies_desc) has radius rad and orbit radius a [R], rate
 * omega [rad/s] and phase phi at t_remaining = 0; at t_remaining = t it is at
 * a (-sin(phi - omega t), cos(phi - omega t), 0).  The host forms in fp64
 *     M = a (-sin phi, cos phi, 0)               the moon at the epoch              [R]
 *     U = a omega (-cos phi, -sin phi, 0)        its velocity at the epoch          [R/s]
 *     scale = k = 1 / rad
 * and every row (t, x, y, z, vx, vy, vz, frac, lossfrac, index) becomes
 *     theta = omega * t  (one fp64 product),  (s, c) = sincos(theta)
 *     q = (c x - s y,  s x + c y,  z)          p' = (q - M) * k
 *     w = (c vx - s vy, s vx + c vy, vz)       v' = (w - U) * k
 * with t, frac, lossfrac and index copied bit for bit: the rotation about z by +omega t carries the
 * moon of the row's time onto the moon of the epoch.  One rounding per operation, in the order
 * written; float32 stores are widened, computed in fp64 and rounded once.  Lengths come out in moon
 * radii and velocities in moon radii per second relative to the moon; the axes stay parallel to the
 * model frame (Sun at -y), so sub-observer angles, local time and the shadow test keep their
 * meaning, with the unit sphere at the origin now the moon.  The Sun-relative radial velocity the
 * g-values need is vy' + (vrplanet + U_y) in the moved unit: a consumer adds U_y * k to the vrplanet
 * it is set with.  The planet neither occults nor shadows in this frame.
 *   nxc_frame_rows         rows [first, first + count) of src as a new store of count rows of
 *                          src's width (the caller frees it with nxc_rows_free)
 *   nxc_frame_columns[_f32]  p rows of host columns; out [6][p]: x', y', z', vx', vy', vz'
 * The three give identical bits for identical input (one kernel, k_frame_rows).  p = 0 or
 * count = 0 does nothing (nxc_frame_rows then delivers a store without rows).  Refused with
 * NXC_ERR_ARG (host-only code, nxc_frame_check.hpp): a null description, a field that is not
 * finite, scale <= 0, first or count outside the store, a null column with p > 0. */
typedef struct nxc_frame_desc {
    double omega;             /* rad/s                                                             */
    double M[3];              /* R: the moon at t_remaining = 0                                    */
    double U[3];              /* R/s: its velocity then                                            */
    double scale;             /* k = 1 / (the moon's radius in R)                                  */
} nxc_frame_desc;
int nxc_frame_rows(nxc_handle *h, const nxc_frame_desc *d, const nxc_rows *src, int64_t first,
                   int64_t count, nxc_rows **out);
int nxc_frame_columns(nxc_handle *h, const nxc_frame_desc *d, int64_t p, const double *t,
                      const double *x, const double *y, const double *z, const double *vx,
                      const double *vy, const double *vz, double *out);
int nxc_frame_columns_f32(nxc_handle *h, const nxc_frame_desc *d, int64_t p, const float *t,
                          const float *x, const float *y, const float *z, const float *vx,
                          const float *vy, const float *vz, float *out);

/* ---- Age cube: the image's impulse response, and images for a time-varying source rate -----------
 * EXTENSION -- every other product reads the stored rows as a steady state: a row at t_remaining =
 * time is a packet of age t0 - time, t0 the run's endtime, and the image sums over all ages.  A row
 * of age a stands for atoms launched a seconds before the epoch, so the image is linear in the
 * source's history: filed by age, the weights give the image's response to a pulse of the source
 * rate, and the image at any epoch for any history is one contraction of that cube.
 * A block has na >= 1 bins over [a_lo, a_hi) seconds of age.  The host forms inv_da = na / (a_hi -
 * a_lo) once in fp64.  A sample that reaches pixel pix with the final weight w -- exactly what is
 * added to image[pix] -- and w != 0 is filed as follows, fp64, one rounding per operation, no
 * contraction (time: the row's first column, widened when it is float32):
 *   age = t0 - (double)time
 *   u   = (age - a_lo) * inv_da
 *   k = 0                 if u < 0                              (younger than the range)
 *   k = 1 + (int)u        if 0 <= u < na                        (bin (int)u of the range)
 *   k = na + 1            otherwise: at or above a_hi, or time not a number
 * and the sample adds {w, w*w} to record pix*(na + 2) + k: one more atomic request per binned
 * sample, pixel-major like the velocity cube.
 *   - A sample with w == 0 adds nothing to the block; it is still counted in the packet image.  Its
 *     time is not read.
 *   - Nothing else is filtered: the na + 2 planes of a pixel sum to image[pix] up to the order of the
 *     additions.
 *   - The image pair, the counts and the counters of an ages pass are those of the plain pass.
 *   nxc_image_ages_enable            after nxc_set_image: na >= 1 allocates and zeroes
 *                                    nx*nz*(na + 2) 16-byte records (NXC_ERR_NOMEM when they cannot
 *                                    be had), na == 0 frees them; nxc_set_image switches the block
 *                                    off again; nxc_image_clear zeroes it with the image while it is
 *                                    on.  NXC_ERR_ARG, before anything is allocated or freed, for
 *                                    na < 0, t0, a_lo or a_hi not finite, a_lo >= a_hi (or a width
 *                                    that is not finite), nx*nz*(na + 2) >= 2^31
 *   nxc_image_ages_accumulate[_f32]  adds p host samples -- six columns, time first -- to the image
 *                                    pair AND the block in one pass, never the tiles of
 *                                    nxc_image_mode
 *   nxc_image_ages_accumulate_rows   the same for rows [first, first + count) of a row store, whose
 *                                    column 0 is the time
 *   nxc_image_ages_download          sums[nx*nz][na + 2][2] = {w sum, w*w sum}, pixel index
 *                                    ix*nz + iz, plane 0 below, planes 1..na the bins, na + 1 above
 *   nxc_image_ages_upload            the block replaced by sums of that layout (for totals that were
 *                                    added on the host)
 *   nxc_image_ages_apply             ne >= 1 epochs: with K[na + 2][ne] (host, row-major, every value
 *                                    finite) out[ne][nx*nz][2] (host) receives
 *                                      out[e][pix] = { sum_k S[pix][k] * K[k][e],
 *                                                      sum_k WW[pix][k] * (K[k][e] * K[k][e]) }
 *                                    {S, WW} being the pixel's record of plane k.  Each sum runs over
 *                                    k = 0, 1, .., na + 1 in that order from 0.0, one rounding per
 *                                    operation, no contraction: a pure function of the block and K,
 *                                    which a loop in the same order reproduces bit for bit.  The rows
 *                                    of the two outer planes are applied like every other.
 *                                    NXC_ERR_ARG for ne < 1, a null K or out, a value of K that is
 *                                    not finite, planes that do not fit a workgroup's LDS even
 *                                    at one pixel and one epoch, and more than 65535 epoch chunks
 *                                    (of up to 64 epochs) -- all before anything is allocated
 *   nxc_camera_ages_*                the same seven against the camera's own image buffer
 * NXC_ERR_STATE names the missing call (the set first, then the enable), then NXC_ERR_ARG.  The age
 * block, the velocity cube and the moments are independent states of a handle: enabling, clearing
 * or freeing one never touches the others, and each pass adds to the image pair and its own block
 * only. */
int nxc_image_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi);
int nxc_image_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                              const double *y, const double *z, const double *vy,
                              const double *frac);
int nxc_image_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                  const float *y, const float *z, const float *vy,
                                  const float *frac);
int nxc_image_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_image_ages_download(nxc_handle *h, double *sums);
int nxc_image_ages_upload(nxc_handle *h, const double *sums);
int nxc_image_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out);
int nxc_camera_ages_enable(nxc_handle *h, int64_t na, double t0, double a_lo, double a_hi);
int nxc_camera_ages_accumulate(nxc_handle *h, int64_t p, const double *time, const double *x,
                               const double *y, const double *z, const double *vy,
                               const double *frac);
int nxc_camera_ages_accumulate_f32(nxc_handle *h, int64_t p, const float *time, const float *x,
                                   const float *y, const float *z, const float *vy,
                                   const float *frac);
int nxc_camera_ages_accumulate_rows(nxc_handle *h, const nxc_rows *r, int64_t first, int64_t count);
int nxc_camera_ages_download(nxc_handle *h, double *sums);
int nxc_camera_ages_upload(nxc_handle *h, const double *sums);
int nxc_camera_ages_apply(nxc_handle *h, int64_t ne, const double *K, double *out);

/* ---- Line-of-sight ages: radiance per age bin along each line of sight ---------------------------
 * EXTENSION -- nxc_los_accumulate gives one radiance per spectrum, summed over all ages; this keeps
 * the age ("Age cube" says what an age is and why the radiance is linear in the source's history).
 * Per spectrum there are na >= 1 bins over [a_lo, a_hi) seconds of age, t0 being the run's endtime;
 * the host forms inv_da = na / (a_hi - a_lo) once in fp64.  A (sample, spectrum) pair is decided
 * and weighed exactly as in nxc_los_accumulate.  Where its wtemp = weight/Apix (times 0 when the foot
 * point is in shadow) is added to radiance[spectrum], and wtemp != 0, the row's time is read and
 * the pair is filed as follows, fp64, one rounding per operation, no contraction (time: the row's
 * first column, widened exactly when it is float32):
 *   age = t0 - (double)time
 *   u   = (age - a_lo) * inv_da
 *   k = 0                 if u < 0                              (younger than the range)
 *   k = 1 + (int)u        if 0 <= u < na                        (bin (int)u of the range)
 *   k = na + 1            otherwise: at or above a_hi, or time not a number
 * -- the plane of "Age cube" -- and the pair adds {wtemp, wtemp*wtemp} to record
 * spectrum*(na + 2) + k.
 *   - A pair with wtemp == 0 (foot point in shadow, frac == 0, g == 0) adds nothing.  Its time is not
 *     read.  It is still counted in npackets and `included`, as for the profile.
 *   - Nothing else is filtered: the na + 2 planes of a spectrum sum to its radiance up to the order
 *     of the additions.
 *   - radiance, npackets, `included`, the used pairs and the counters of an ages pass are those of
 *     the plain pass over the same samples, up to the fp64 addition order of radiance.
 *   nxc_los_ages_enable             na >= 1 allocates and zeroes S*(na + 2) 16-byte records
 *                                   (NXC_ERR_NOMEM when they cannot be had), na == 0 frees them; a
 *                                   second enable replaces and zeroes.  NXC_ERR_ARG, before anything
 *                                   is allocated or freed, for S < 1, na < 0, t0, a_lo or a_hi not
 *                                   finite, a_lo >= a_hi (or a width that is not finite),
 *                                   S*(na + 2) >= 2^31
 *   nxc_los_ages_accumulate[_f32], _rows
 *                                   nxc_los_accumulate[_f32], _rows with the time column in front (a
 *                                   row store carries it: its column 0): everything the plain entry
 *                                   returns, and the pairs' contributions added to the block.  Sums
 *                                   accumulate over calls, slabs and Outputs until the next enable.
 *                                   NXC_ERR_STATE without an enabled block; NXC_ERR_ARG when S is not
 *                                   the enabled one, or time is null with P > 0; P == 0 adds nothing
 *   nxc_los_ages_download           sums[S][na + 2][2] = {wtemp sum, wtemp*wtemp sum}, plane 0 below
 *                                   the range, 1..na the bins, na + 1 above
 * The block is a state of the handle of its own: nxc_los_accumulate* and nxc_los_profile_* never
 * touch it, and these entries never touch the profile or the image's and camera's age blocks. */
int nxc_los_ages_enable(nxc_handle *h, int64_t S, int64_t na, double t0, double a_lo, double a_hi);
int nxc_los_ages_accumulate(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                            int64_t P, const double *time, const double *x, const double *y,
                            const double *z, const double *vy, const double *frac,
                            const int64_t *index, int64_t n_index, double *radiance,
                            int64_t *npackets, uint8_t *included, int64_t used_cap,
                            int64_t *used_pairs, int64_t *n_used);
int nxc_los_ages_accumulate_f32(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                int64_t P, const float *time, const float *x, const float *y,
                                const float *z, const float *vy, const float *frac,
                                const int64_t *index, int64_t n_index, double *radiance,
                                int64_t *npackets, uint8_t *included, int64_t used_cap,
                                int64_t *used_pairs, int64_t *n_used);
int nxc_los_ages_accumulate_rows(nxc_handle *h, const nxc_los_desc *d, int64_t S, const double *sc,
                                 const nxc_rows *r, int64_t first, int64_t count,
                                 int64_t index_shift, int64_t n_index, double *radiance,
                                 int64_t *npackets, uint8_t *included, int64_t used_cap,
                                 int64_t *used_pairs, int64_t *n_used);
int nxc_los_ages_download(nxc_handle *h, double *sums);

#ifdef __cplusplus
}
#endif
#endif
