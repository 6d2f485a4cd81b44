/*
 * scarplet_hip.h - C ABI of libscarplet_hip.so, the MI355X (gfx950) engine
 * behind scarplet's template-matching hot path.
 *
 * The reference (stgl/scarplet) is pure Python; the interface this library
 * replaces is the body of
 *
 *     scarplet/core.py:297-377   match_template()      (per-template kernel)
 *     scarplet/core.py:198-243   compare()             (running-best fold)
 *     scarplet/dem.py:68-107     _calculate_directional_laplacian()
 *     scarplet/WindowedTemplate.py:159-183, 498-520, 66-84, 257-304
 *                                template() / get_window_limits() /
 *                                get_err_mask() of the built-in plugins
 *
 * i.e. everything that runs once per (age, orientation) template.  The search
 * drivers above it (core.py:139-195 calculate_best_fit_parameters,
 * core.py:266-294 match) stay host code: they build the parameter grids,
 * turn every template into an sc_template descriptor and make ONE call.
 * INTEGRATION.md shows the ctypes binding a scarplet maintainer would add.
 *
 * Conventions
 *   - plain C types only; all host buffers are caller-owned, C order;
 *   - every call returns SC_OK (0) or a negative SC_ERR_* code and never
 *     throws; sc_last_error() gives the message for the last failure;
 *   - calls are synchronous unless the name ends in _async; an sc_ctx is
 *     bound to one GPU and is not thread-safe; distinct contexts are
 *     independent (one context per GPU / per process).
 */
#ifndef SCARPLET_HIP_H
#define SCARPLET_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 10

#define SC_OK               0
#define SC_ERR_INVALID     -1   /* bad argument                                */
#define SC_ERR_HIP         -2   /* HIP runtime failure (see sc_last_error)     */
#define SC_ERR_NO_DEM      -3   /* sc_set_dem has not been called              */
#define SC_ERR_UNSUPPORTED -4   /* plan outside what the kernels are built for */
#define SC_ERR_COMM        -5   /* RCCL failure                                */

/* template kinds (WindowedTemplate.py classes) */
#define SC_KIND_SCARP   0       /* Scarp and the UpperBreak variants (l.87-304) */
#define SC_KIND_RICKER  1       /* Ricker / Channel (l.434-525)                 */
#define SC_KIND_WINDOW  2       /* any other plugin: W window uploaded by host  */

/* template flags */
#define SC_FLAG_NEGATE      1   /* W -> -W            (WindowedTemplate.py:254) */
#define SC_FLAG_ERR_XR_LE0  2   /* snr=0 where xr<=0  (WindowedTemplate.py:265) */
#define SC_FLAG_ERR_XR_GE0  4   /* snr=0 where xr>=0  (WindowedTemplate.py:302) */
#define SC_FLAG_NO_LIMITS   8   /* get_window_limits() all False (l.495-496)    */

/* matching method */
#define SC_METHOD_DIRECT 0      /* real-space sliding window                    */
#define SC_METHOD_FFT    1      /* overlap-save tiles, LDS FFTs                 */

#define SC_ID_NONE 0xFFFFFFFFu  /* best-id value of a cell no template has won  */

typedef struct sc_ctx sc_ctx;

/*
 * One (scale, age, orientation) template = one call of match_template()
 * in the reference (core.py:297).  All doubles are evaluated by the host with
 * numpy exactly as the reference evaluates them, so that the support W != 0
 * decided on the device in float64 is bit-for-bit the reference's.
 */
typedef struct sc_template {
    int32_t  kind;            /* SC_KIND_*                                      */
    int32_t  flags;           /* SC_FLAG_*                                      */
    double   cos_a, sin_a;    /* cos/sin of the template's alpha = -orientation */
    double   c, d;            /* window half-widths along xr / yr (l.61-64)     */
    double   p0, p1;          /* SCARP: 2*kt**1.5*sqrt(pi), 4*kt (l.177-178)
                                 RICKER: pi*f, unused (l.514-515)
                                 WINDOW: n = count(W != 0), sum(W**2)           */
    double   cc, sc2, ss;     /* curvature mix, dem.py:103-104:
                                 curv = cc*d2z_dx2 - sc2*d2z_dxdy + ss*d2z_dy2  */
    int32_t  ilo, ihi, jlo, jhi;     /* cells kept by get_window_limits()
                                        (l.66-84): ilo<=i<=ihi && jlo<=j<=jhi   */
    int32_t  pmin, pmax, qmin, qmax; /* support bounding box in offsets from
                                        the template centre (ny//2, nx//2)      */
    uint32_t id;              /* recorded in the best-id plane when it wins     */
    int32_t  window;          /* SC_KIND_WINDOW: slot given to sc_upload_window */
} sc_template;

/* Geometry of one sc_match call (computed by the host planner). */
typedef struct sc_plan {
    int32_t method;           /* SC_METHOD_*                                    */
    int32_t Ty, Tx;           /* FFT tile size (powers of two, 64..4096)        */
    int32_t Vy, Vx;           /* valid outputs per tile = T - support span      */
    int32_t nty, ntx;         /* tiles covering the core region                 */
    int32_t circ_y, circ_x;   /* axis handled by its own periodicity (T == n)   */
    int32_t Py, Qx;           /* max pmax / qmax over the batch                 */
    int32_t group;            /* templates per inverse-transform launch (>= 1)  */
} sc_plan;

/* ---- lifetime ---------------------------------------------------------- */
int  sc_abi_version(void);
/* Which sources this binary was compiled from: the first 16 hex digits of the SHA-256 over the
 * library's sources (the seven .hip files of csrc, sc_internal.h, this header) in the Makefile's order, worked out
 * at build time - `make -C scarplet_amd/csrc print-build-id` prints the same string for the tree
 * at hand.  bench.py prints it in every line and __graft_entry__.build() compares the two: a
 * stale prebuilt binary is visible instead of silently benchmarked. */
const char* sc_build_id(void);
int  sc_device_count(void);
int  sc_create(int device, sc_ctx** out);
void sc_destroy(sc_ctx* ctx);
const char* sc_last_error(sc_ctx* ctx);

/*
 * Hand over the elevation block this context works on.
 *   z            ly x lx float64, rows gy0.. / columns gx0.. of the ny x nx DEM
 *                (global indices may lie outside [0,n): halo cells of a
 *                periodic DEM); replaces DEMGrid._griddata (dem.py:84)
 *   core         [cy0,cy1) x [cx0,cx1): global cells whose results this
 *                context owns
 *   wrap         1: the block IS the whole DEM (ly==ny, lx==nx, gy0==gx0==0)
 *                and neighbours are found modulo the DEM size
 *   xaxis,yaxis  centred cell coordinates (WindowedTemplate.py:50-53)
 * Computes the three curvature stencils of dem.py:88-101 on the device.
 */
int sc_set_dem(sc_ctx* ctx, const double* z, int ly, int lx, int gy0, int gx0,
               int ny, int nx, int cy0, int cy1, int cx0, int cx1,
               double dx, double dy, int wrap,
               const double* xaxis, const double* yaxis);

/*
 * What the device found in the block handed over last (one pass over it in HBM, part of
 * sc_set_dem / sc_set_dem_device):
 *   nan_cells  cells that are NaN.  One NaN turns every output of the reference NaN (its
 *              whole-grid FFTs spread it, core.py:349-363): the host layer answers such a DEM
 *              with the reference's maps and does not search it (scarplet_amd/core.py);
 *   hash2      128-bit fingerprint of the float64 bit patterns (two 64-bit words);
 *   unchanged  1: the block, its geometry and cell size equal what the context held before this
 *              hand-over - the curvature planes were kept, and so were the curvature spectra of
 *              the last search (option "spectra_mb"): the next scale of a multi-scale job, which
 *              the reference runs as one sl.match per scale on the same data
 *              (docs/source/examples/channels.ipynb).
 * Replaces two host passes over the DEM (np.isnan(z).any(), a hash of the values) per call.
 * Any pointer may be NULL.
 */
int sc_dem_info(sc_ctx* ctx, long long* nan_cells, unsigned long long* hash2, int* unchanged);

/* Same, with z already in device memory (used after sc_halo_exchange). */
int sc_set_dem_device(sc_ctx* ctx, const void* z_dev, int ly, int lx, int gy0,
                      int gx0, int ny, int nx, int cy0, int cy1, int cx0,
                      int cx1, double dx, double dy, int wrap,
                      const double* xaxis, const double* yaxis);

/* Explicit template window for SC_KIND_WINDOW (generic plugins): w is the
 * h x w float64 block W[ny//2+pmin .., nx//2+qmin ..]; returns the slot.
 * The slot keeps it twice: in float32 for the searches and as given, in
 * float64, for the float64 scorers (sc_settle_exact, sc_score_*_f64; ABI 10). */
int sc_upload_window(sc_ctx* ctx, const double* w, int h, int wd, int* slot);
/* Optional per-cell masks for generic plugins (ny x nx uint8, global):
 * get_window_limits() and get_err_mask() results; pass NULL to clear. */
int sc_set_masks(sc_ctx* ctx, int slot, const uint8_t* limits,
                 const uint8_t* err);
int sc_clear_windows(sc_ctx* ctx);

/*
 * The reference's Crater template (WindowedTemplate.py:528-605; docs/craters.md) for every (radius, age) of a grid,
 * synthesised on the device in float64 straight into window slots - no host array, no upload.  Template
 * k = i_radius * n_ages + i_age is W = sum over theta_j, j ascending, of sign_j * (-xr / p0) * exp(-(xr * xr) / p1) where
 * |xr| < 1 and |yr| < d_half, with xm = x - dx, yp = y + dy, xr = xm * cos_a + yp * sin_a, yr = -xm * sin_a + yp * cos_a on
 * the axes of the last sc_set_dem (SC_ERR_NO_DEM without one), every operation correctly rounded and in this order.
 * The caller evaluates what decides the two compares with numpy, as the reference does:
 *   theta_tab  n_theta x 3: cos(alpha_j), sin(alpha_j) of alpha_j = -theta_j, and the sign (-1 where
 *              pi/2 < theta_j < 3 pi/2, else +1)
 *   dxy        n_radii x n_theta x 2: dx = R cos(theta_j), dy = R sin(theta_j)
 *   ring       n_radii x 2: bounds lo <= x^2 + y^2 <= hi outside which no strip keeps a cell - at most
 *              max(R - 1, 0)^2 and at least (R + 1)^2 + d_half^2, widened beyond rounding; such cells are 0 unevaluated
 *   age_tab    n_ages x 2: p0 = 2 kt^1.5 sqrt(pi), p1 = 4 kt
 *   d_half     5 / de
 *   boxes      n_radii x 4: pmin, pmax, qmin, qmax of the radius's support box in offsets from (ny / 2, nx / 2); a box
 *              that leaves the grid is SC_ERR_INVALID
 * slots, count, sumsq: n_radii x n_ages each - the window slot (what sc_upload_window returns: the float64 window, its
 * float32 copy and the W != 0 bytes, for sc_template.window), count(W != 0) and sum(W * W) (sc_template.p0 / p1 of an
 * SC_KIND_WINDOW descriptor), summed in a fixed order: the same bits on every run.  w_out: the float64 windows back on
 * the host, one box after the other in template order, or NULL.  All slots of a call share one allocation, which
 * sc_clear_windows frees.  SC_ERR_UNSUPPORTED beyond 4096 strips, 65535 templates or 2^31 - 1 window cells.  Timed
 * under SC_K_WINDOWS.
 */
int sc_crater_windows(sc_ctx* ctx, int n_radii, int n_ages, int n_theta, const double* theta_tab, const double* dxy,
                      const double* ring, const double* age_tab, double d_half, const int32_t* boxes, int* slots,
                      double* count, double* sumsq, double* w_out);

/*
 * Engine options, set explicitly (nothing is read from the environment):
 *   "kappa"    float32 resolution floor of the FFT epilogue in units of eps32
 *              (default 4; 0 switches the floor off; sc_internal.h sc_epi_floor)
 *   "variant"  alternative kernel paths kept for cross-checks in the tests:
 *              0 default, 1 paired-template chunks by the four-column LDS-parked kernel at
 *              every tile size, 2 inverse column pass by the four-column kernels throughout
 *              (no wave-per-column kernel), 5 no paired-template mode, 6 inverse
 *              column pass as two launches per tile pair (own columns, mirrors) instead
 *              of one launch with the two kinds paired per XCD, 7 template spectra by the
 *              separate column-transform and split kernels, 8 complex-spectrum I1 for
 *              symmetric templates, 9 generic row kernel at every tile size, 10 the round-2
 *              real-space kernel (walks the support box; one orientation per launch), 11 the
 *              real-space kernel with T3 accumulated tap by tap on every row (no sum shared
 *              between a lane's adjacent outputs), 12 no paired orientations (one-tile searches
 *              with one template per orientation then leave half of every transform empty),
 *              13 the inverse passes store and transform every valid tile row (default: rows
 *              that a template's window limits mask are skipped for that template), 15 the row
 *              pass of small grids folds a launch's transforms in ONE workgroup per row (default:
 *              dealt out over up to four, the shares merged in order), 16 the real-space kernel's
 *              256 x 16 patch also where the 512 x 16 patch would be taken, 17 the orientation's
 *              curvature plane written by a pass of its own and read back by the forward row pass
 *              (default: mixed from the three stencil planes inside that pass - the same bits), 18 the
 *              inverse column pass at column length 512 by the four-column kernels (default: half a wave
 *              per column, k_inv_cols_h2 - the same bits), 19 paired orientations on k_inv_cols_h2 too,
 *              20 at most 64 templates per row-pass launch (default: the dealt-out row pass of small grids
 *              takes up to 255 in shares of at most 64 transforms - the same bits)
 *   "batch"    1 (default): searches whose single orientation does not fill the
 *              chip send several orientations through every launch; 0: one
 *              orientation per launch sequence.  Results are bit-identical.
 *   "batch_fill"  column-pass workgroups a batched launch sequence aims at (0: the default, 4096):
 *              orientations per launch = batch_fill / (tile pairs x Tx / 8), at most 64 and what the
 *              row pass's tables hold.  Results are bit-identical whatever the batch.
 *   "fuse_fwd" 1 (default): the wave-per-column inverse pass (column length 1024 / 2048, symmetric
 *              templates) runs the curvature's forward column transform on the columns it parks,
 *              instead of a k_fwd_cols launch per orientation; 0: the two-launch form.  Off by itself
 *              while curvature spectra are kept ("spectra_mb").  Results are bit-identical.
 *   "i1_pairs" tile pairs per launch of the wave-per-column inverse pass (default 2; 1: one pair per
 *              launch), interleaved so that the workgroups which stream the same template
 *              coefficients run on one XCD at the same time.  Results are bit-identical.
 *   "near_window"  > 0: the FFT row pass flags near-ties within this relative window (sc_get_near_ties); needs
 *              the fast row kernel (tile widths 512 / 1024 / 2048) and templates without per-cell masks, else
 *              sc_match answers SC_ERR_UNSUPPORTED.  Default 0.
 *   "split_i1" 1 (default): a column pass whose workgroups do not fill the chip (a small DEM with many
 *              templates per orientation) deals its transforms out over up to eight workgroups per column
 *              block; 0: one workgroup per column block walks all of them.  Results are bit-identical.
 *   "split_fill"  waves the dealt-out row pass of small grids may come to (0: the default, 4300 - four
 *              per SIMD and 5 %; round 4: 2048).  Results are bit-identical.
 *   "y_gb"     memory budget of the column -> row pass hand-off buffers in GB
 *              (0: a quarter of the free memory, at most 32)
 *   "sib"      sibling rendezvous (bit 0: row pass): the two workgroups that read the two
 *              halves of the same 128-byte hand-off lines keep within one template of each
 *              other so that the second read hits the XCD's L2.  Default 0: it moves 10 % fewer
 *              bytes and takes 3 % longer (profiles/r03_sibling_rendezvous.txt).  Results are
 *              bit-identical either way.
 *   "spectra_mb"  > 0: a search whose orientations' curvature spectra fit this many MiB keeps
 *              them (one slot per orientation instead of one per batched orientation), and a
 *              later sc_match on the same DEM with the same tile plan and the same orientations
 *              - the next scale of a multi-scale job, the reference's one sl.match per scale
 *              (docs/source/examples/channels.ipynb) - skips the curvature passes.  The spectra
 *              are the same bits either way, so are the results.  Setting the option (to any
 *              value) and loading a DEM drop what was kept.  Default 0 in the library; the
 *              Python host sets 8192.
 *   "fit_chunk"  n > 0: every fit call (sc_fit_profiles*, sc_lateral_offsets*, sc_fit_segments*,
 *              sc_bootstrap_segments*, sc_fit_strike*, sc_strike_bootstrap*, sc_channel_*, sc_snr_surface) closes a chunk of its work at n cells
 *              where its built-in bound (2^19 cells, the parked bytes of SC_SEGMENT_MAX_PARK, 256 MiB of
 *              cubes) lies higher; it never raises one.  The per-cell calls launch on at most n cells; the
 *              segment calls take whole segments while their cells stay within n, a longer segment alone
 *              (a segment above SC_SEGMENT_MAX_PARK is refused as before); sc_snr_surface rounds n up to
 *              whole batches of eight cells.  An integer >= 0, finite; 0 (default): the built-in bounds
 *              alone.  Every output byte is the same for every value: the option exists so that the
 *              tests run the chunks' hand-over on small inputs (tests/test_gpu_fit_chunks.py).
 *   "channel_terms"  1 (default): sc_channel_profiles* forms what a pair's column leaves against (1, s) on a
 *              profile without a missing point once per call, and such a profile runs two sweeps per pair; 0: every
 *              profile runs the four sweeps.  0 or 1.  Every output byte is the same either way: the option exists so
 *              that a test compares the two routes (tests/test_gpu_channels.py).
 *   "templ_gb"  memory budget, in GB, of the template coefficient planes a context keeps across searches.  The
 *              templates' forward chain (k_windows, the row transform, the column transform and split) reads nothing of
 *              the DEM's values: a later sc_match / sc_match_template with the same descriptors, grid spacing, axis
 *              values under the windows, tile size and route - the next DEM of a survey, the next call - finds the
 *              planes and launches nothing of the chain.  Symmetric built-in templates (Scarp, Ricker / Channel) on the
 *              FFT path only: generic templates (complex spectra) and SC_KIND_WINDOW templates keep the uncached path,
 *              the real-space path has no such planes.  An entry is one orientation run, or the runs a batched launch
 *              takes together.  Least recently used entries go first; a search never evicts what it has used itself, so
 *              a search larger than the budget keeps what fits and runs the chain for the rest.  0: off (what is held
 *              is freed); < 0: automatic - half of the device memory that is free when a search has its buffers, the
 *              entries held counted as free.  Whatever the budget, an allocation of the context that finds no memory
 *              drops entries before it fails.  Results are bit-identical for every value.  Default 0 in the library;
 *              the Python host sets the automatic budget on the context it keeps per device between calls.
 */
int sc_set_option(sc_ctx* ctx, const char* name, double value);

/* Drop the template coefficient planes kept by option "templ_gb" (sc_set_dem and option "spectra_mb" do not: those are
 * about the DEM's spectra).  sc_destroy drops them too. */
int sc_forget_templates(sc_ctx* ctx);
/* The template cache since the context was made: orientation runs served from an entry (hits) and sent through the
 * forward chain (misses: those that found no room included), and entries and bytes held now, entries dropped for room,
 * for a smaller budget or under allocation pressure (evictions).  Any pointer may be NULL. */
int sc_templ_cache_info(sc_ctx* ctx, long long* hits, long long* misses, long long* entries, long long* bytes,
                        long long* evictions);

/*
 * One pass of the nodata fill that precedes the matcher (DEMGrid._fill_nodata,
 * dem.py:388-414: rasterio.fill.fillnodata -> GDALFillNodata).  z: ny x nx
 * float64 host array, NaN = nodata, filled in place the way GDAL's second pass
 * does it (alg/rasterfill.cpp as restated in oracle/scarplet_oracle.py
 * fill_nodata_pass): float32 work values (valid cells come back rounded through
 * float32 as well), per nodata cell the nearest valid cell of each quadrant over
 * the columns x -+ step, step <= floor(max_search_distance) - left quadrants from
 * step 0, right quadrants from step 1, columns clamped at the raster edge (the
 * steps end at nx: beyond it both clamped columns repeat checks already made, so
 * a distance far larger than the raster costs no more than one equal to nx) - and
 * the mean weighted by 1 / distance over the quadrants within
 * max_search_distance; then smoothing_iterations 3x3 means over the filled cells.
 * *remaining = cells still nodata (no source within reach); the host repeats with
 * a new distance as the reference does.  Independent of the DEM held by the
 * context.  PARITY UNPINNED: GDAL is not available to check against and no
 * GDAL-written fixture exists.
 */
int sc_fill_nodata(sc_ctx* ctx, double* z, int ny, int nx, double max_search_distance,
                   int smoothing_iterations, long long* remaining);

/* ---- the hot path ------------------------------------------------------ */
/* Zero the running-best record (compare() start state, core.py:222-225). */
int sc_reset_best(sc_ctx* ctx);

/* Match n templates and fold them, in the order given, into the running
 * best record (snr, amp, id), float32 per cell.  Fold rule (compare(),
 * core.py:227-240, as far as it is meaningful in float32):
 *   - a template takes a cell when its SNR is strictly greater than the
 *     record's; cells it masks (window limits, error mask) score 0 and never
 *     take a cell;
 *   - an exact SNR tie KEEPS THE INCUMBENT.  The reference's two strict
 *     compares zero the record on a tie; in its float64 arithmetic that is a
 *     rounding accident, in float32 it is systematic (an even or odd template
 *     gives bit-identical SNR at -pi/2 and +pi/2) and the zeroed record would
 *     be overtaken by an arbitrary later template.  The literal float64 rule,
 *     ties and sticky NaNs included, is sc_compare_*;
 *   - the order of the fold is the order of t[]; it matters on ties only;
 *   - NaN cannot arise: sc_set_dem's elevations must be finite (the host layer
 *     answers a DEM with NaNs the way the reference does, without the device).
 * Templates with equal (cc, sc2, ss) share one curvature plane; send them
 * adjacent. */
int sc_match(sc_ctx* ctx, const sc_template* t, int n, const sc_plan* plan);
int sc_match_async(sc_ctx* ctx, const sc_template* t, int n,
                   const sc_plan* plan);
int sc_sync(sc_ctx* ctx);

/* amp / snr maps of ONE template over the core region (match_template(),
 * core.py:377), float32, (cy1-cy0) x (cx1-cx0). */
int sc_match_template(sc_ctx* ctx, const sc_template* t, const sc_plan* plan,
                      float* amp, float* snr);

/* Copy the running best of the core region to the host. */
int sc_get_best(sc_ctx* ctx, float* amp, float* snr, uint32_t* id);

/* The running best as the reference returns it (core.py:243, 194): four float64
 * planes [amp, age, angle, snr] of the core region, out = 4 x (cy1-cy0) x
 * (cx1-cx0) doubles.  param_of_id / angle_of_id map a template id (< n_ids) to
 * its (age, orientation); cells no template has won are all zero. */
int sc_get_result(sc_ctx* ctx, const double* param_of_id, const double* angle_of_id,
                  int n_ids, double* out);

/*
 * compare() for results that already sit on the host (core.py:198-243), e.g.
 * user code that calls match_template() per orientation and folds itself.
 * float64, literally best = (best_snr > snr)*best + (best_snr < snr)*this for
 * the four planes, snr last.  Independent of the DEM state.
 */
int sc_compare_begin(sc_ctx* ctx, int ny, int nx);
int sc_compare_fold(sc_ctx* ctx, const double* amp, const double* snr,
                    double age, double angle);
/* The same step for a result whose age and angle are per-cell planes - the
 * output of an earlier fold, as match() feeds calculate_best_fit_parameters'
 * (4, ny, nx) arrays to compare() (core.py:288-292). */
int sc_compare_fold_planes(sc_ctx* ctx, const double* amp, const double* age,
                           const double* angle, const double* snr);
int sc_compare_end(sc_ctx* ctx, double* amp, double* age, double* angle,
                   double* snr);

/* Directional curvature of the block (dem.py:68-107), float32 ly x lx. */
int sc_curvature(sc_ctx* ctx, double cc, double sc2, double ss, float* out);
/* The same as the reference's data object returns it - float64, dem.py:103-104's expression in
 * numpy's evaluation order: out = d2z_dx2 * cos2 - 2 * d2z_dxdy * sin_a * cos_a + d2z_dy2 * sin2,
 * cos2 = cos(alpha)**2 and sin2 = sin(alpha)**2 evaluated by the caller.  Replaces
 * CalculationMixin._calculate_directional_laplacian (dem.py:68-107) and _calculate_laplacian
 * (dem.py:62-66) behind scarplet_amd.dem.DEMGrid's methods of those names. */
int sc_curvature_f64(sc_ctx* ctx, double cos2, double sin_a, double cos_a, double sin2,
                     double* out);

/* The moments behind CalculationMixin._estimate_curvature_noiselevel (dem.py:152-179), float64.  With A, B, C the
 * three stencil planes of the grid (d2z_dx2, d2z_dxdy, d2z_dy2, as sc_curvature_f64 forms them) and
 * H_P = P - G * P, G the separable filter whose 2 radius + 1 correlation weights the caller passes
 * (gaussian_filter's, mode 'reflect': half-sample symmetric, period 2 n, so any radius holds on any grid):
 *   out[0..9]    n, mean[3], C[6] of (H_A, H_B, H_C) over all cells; C = sum of centred products, upper
 *                triangle, row-major (AA, AB, AC, BB, BC, CC);
 *   out[10..19]  the same over the cells farther than radius (Chebyshev distance) from every cell nan_mask
 *                flags (ny x nx bytes, nonzero = NaN in the caller's grid) - the cells the reference's first
 *                orientation keeps; with nan_mask NULL a copy of out[0..9].
 * Works on the whole grid sc_set_dem set: a context holding a block of it (tile sharding) gets
 * SC_ERR_INVALID, and so does radius < 0; radius > SC_NOISE_MAX_RADIUS gets SC_ERR_UNSUPPORTED.  The grid
 * must be finite (the caller zero-fills NaN cells, as dem.py:84-86 does).  Deterministic: the same bits on
 * every run.  Timed as one bracket, SC_K_NOISE. */
#define SC_NOISE_MAX_RADIUS 1048576
int sc_curvature_noise(sc_ctx* ctx, const double* weights, int radius, const uint8_t* nan_mask,
                       double* out);

/*
 * Traces of a result (docs/traces.md): the line one cell wide along the strike that a scarp or a channel leaves in
 * the result planes, cut into connected segments, one row of a table each.  Nothing in the reference does this (its
 * CHANGELOG lists non-maximum suppression as open; docs/source/examples/scarps.ipynb walks the rows in a Python loop).
 * A cell is valid when its snr is finite and > 0 and its angle finite with |angle| <= 1e6.  Steps:
 *   1. thinning: q = floor((angle / pi) * 4 + 0.5), s = q - 4 floor(q / 4) picks the step d = (drow, dcol) =
 *      (0,+1), (+1,-1), (+1,0), (+1,+1) for s = 0..3 - along the profile of the template that won the cell, whose
 *      alpha is -angle (x along the columns, y along the rows); correctly rounded float64 operations only.  With
 *      v(n) = snr(n) inside the grid where finite, -inf otherwise: thin(c) = valid(c) && snr(c) >= snr_low &&
 *      snr(c) > v(c - d) && snr(c) >= v(c + d) (of a plateau of two equal cells one stays);
 *   2. connected components of thin under 8-connectivity; a cell is strong where snr >= snr_high; a component with
 *      at least one strong cell and at least min_cells cells is a segment; segments are numbered 1..K in ascending
 *      order of their smallest linear index (r * nx + c);
 *   3. one sc_segment per segment, in label order.  Sums are float64 and the same bits on every run (no float atomics).
 * thin: ny x nx bytes (1 = thinned cell), labels: ny x nx int32 (0 outside segments), either may be NULL;
 * *n_segments = K.  SC_ERR_INVALID for snr_low not finite or <= 0, snr_high < snr_low or not finite, min_cells < 1;
 * SC_ERR_UNSUPPORTED for more than 2^31 - 1 cells.  The buffers are the trace's own: the record, the result planes,
 * the curvature spectra and the fill buffers are not touched.  One read-back of K (and the cell count) mid-sequence.
 */
typedef struct sc_segment {
    int64_t  first;           /* smallest linear index                          */
    int64_t  n_cells;         /* cells of the segment                           */
    int64_t  n_strong;        /* cells with snr >= snr_high                     */
    int32_t  row_min, row_max, col_min, col_max;   /* bounding box               */
    int64_t  peak;            /* linear index of the largest snr (ties: the smallest index) */
    double   snr_peak, amp_peak, age_peak, angle_peak;  /* the planes at peak, as they are */
    double   sum_amp, sum_abs_amp, sum_age, sum_snr;    /* sums over the cells    */
    double   sum_cos2a, sum_sin2a;                      /* of cos(2 angle), sin(2 angle): the axial mean orientation */
} sc_segment;
/* planes: 4 x ny x nx float64 on the host, (amp, age, angle, snr) as sc_get_result writes them; uploaded, then traced */
int sc_trace_planes(sc_ctx* ctx, const double* planes, int ny, int nx, double snr_low, double snr_high,
                    long long min_cells, uint8_t* thin, int32_t* labels, long long* n_segments);
/* the same on the context's own result: the planes sc_get_result would return (param_of_id, angle_of_id, n_ids as
 * there, the exact mode's patches laid over them), formed on the device and traced there - no upload */
int sc_trace_result(sc_ctx* ctx, const double* param_of_id, const double* angle_of_id, int n_ids, double snr_low,
                    double snr_high, long long min_cells, uint8_t* thin, int32_t* labels, long long* n_segments);
/* the first n rows (n <= K) of the last trace's table */
int sc_trace_segments(sc_ctx* ctx, sc_segment* out, long long n);

/*
 * Scarp-profile dating across a trace (docs/profiles.md): for each of K cells an elevation profile is cut across the
 * strike, z(s) = c0 + b s + a erf(s / (2 sqrt(kt))) is fitted to it for every age of a grid, and the best age, its
 * coefficients and the interval of ages the data do not tell apart come back as one sc_profile_fit.  The window of
 * the Scarp template is the second derivative of that erf, so `a` estimates what the amp plane of a search estimates.
 *   cells   K linear indices r * nx + c;  sa, ca: sin and cos of the cell's orientation (as sc_get_result's angle
 *           plane gives it), evaluated by the caller: the profile runs along (row, col) = (-sa, ca), the strike
 *           along (ca, sa)
 *   samples for j = -h..h, k = -w..w: rr = r + (k ca - j sa), cc = c + (j ca + k sa); inside when 0 <= rr <= ny - 1
 *           and 0 <= cc <= nx - 1; bilinear between the four cells around it (r0 = min(floor rr, ny - 2), likewise
 *           c0); valid when inside and finite.  p_j = mean of the valid samples in ascending k, s_j = j de; j is a
 *           valid point when one k is
 *   fit     the cell is fitted when at least min_samples valid points lie on either side of j = 0; else status 1,
 *           kt_index -1 and NaN in every float field.  For every age least squares of p on (1, s, erf(s / (2
 *           sqrt(kt_i)))) over the valid points (columns orthogonalised, never normal equations on raw s);
 *           sse_i = sum of the squared explicit residuals; kt_index = argmin, ties to the smallest index
 *   interval thr = sse_min (1 + delta / (n - 3)); lo_index walks down from kt_index while sse[lo_index - 1] <= thr,
 *           hi_index up likewise; status gains 2 where lo_index == 0 and 4 where hi_index == A - 1
 * out_rows: K rows in the order of the cells (repeats allowed); out_sse: K x A float64 or NULL.  Every sum runs in a
 * fixed order: the same bytes on every run.  SC_ERR_INVALID: a cell outside the grid, sa / ca not finite, ages not
 * finite, not positive or not strictly increasing, A < 1, h < 1, w < 0, min_samples < 2 or > h, delta < 0 or not
 * finite, de not finite or <= 0, ny or nx < 2.  SC_ERR_UNSUPPORTED: A > SC_PROFILE_MAX_AGES, h > SC_PROFILE_MAX_HALF,
 * w > SC_PROFILE_MAX_SWATH, K > 2^31 - 1, a context that holds a block of a larger grid.  The buffers are the call's
 * own: the record, the result planes, the kept spectra, the trace and fill buffers are not touched.  Timed as
 * SC_K_PROFILE.
 */
#define SC_PROFILE_MAX_AGES  64
#define SC_PROFILE_MAX_HALF  1024
#define SC_PROFILE_MAX_SWATH 32
typedef struct sc_profile_fit {
    int64_t  cell;            /* the input cell                                  */
    int32_t  n;               /* valid points of the profile                     */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;   /* the interval, as indices of the age grid   */
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) */
    double   kt, kt_lo, kt_hi;
    double   a, b, c0;        /* of the best age: the scarp's offset is 2 a      */
    double   sse, rmse;       /* rmse = sqrt(sse / (n - 3))                      */
} sc_profile_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_profiles(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                    const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                    sc_profile_fit* out_rows, double* out_sse);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own: the context's DEM, if it has
 * one, stays as it is */
int sc_fit_profiles_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                        const double* ca, long long K, const double* ages, int A, int h, int w, double de,
                        double delta, int min_samples, sc_profile_fit* out_rows, double* out_sse);

/*
 * One scarp age per trace segment, fitted jointly (docs/segments.md): the K cells come grouped into S segments
 * (seg_start[S + 1], a CSR array from 0 to K; seg_label[S], positive and strictly increasing), each cell's profile is
 * sampled exactly as sc_fit_profiles samples it, and per segment and age ONE least-squares problem is solved over all
 * its usable profiles: the amplitude a and the age are the segment's, every profile keeps an intercept c0_c and a
 * slope b_c of its own (fixed effects).
 *   usable   a profile with at least min_samples valid points on either side of j = 0 (the rule of sc_fit_profiles);
 *            other cells count in n_cells only
 *   per profile c and age i: sbar, pbar, ebar, beta, gamma, See_ci, Sep_ci as passes 0 to 2 of sc_fit_profiles form them
 *   segment  a_i = (sum_c Sep_ci) / (sum_c See_ci); b_ci = beta_c - a_i gamma_ci; c0_ci = (pbar_c - a_i ebar_ci) -
 *            b_ci sbar_c; sse_ci = sum_j of the squared explicit residuals; sse_i = sum_c sse_ci.  The sums over c
 *            run over the usable profiles in input order: blocks of 64 consecutive ones summed in sequence from the
 *            first, then the block sums in sequence from the first - a shape that depends on n_profiles alone, and
 *            no addition at all for one profile
 *   choice   n pooled valid points, dof = n - 2 n_profiles - 1; fitted when n_profiles >= min_profiles and dof >= 1,
 *            else status 1, indices -1, NaN floats.  kt_index = argmin sse_i (ties to the smallest index), rmse =
 *            sqrt(sse / dof), thr = sse_min (1 + delta / dof), lo_index / hi_index / status 2 and 4 as sc_fit_profiles
 * A segment of one usable profile returns the kt_index, lo_index, hi_index, status, a, sse and rmse of sc_fit_profiles
 * for that cell, bit for bit.  out_rows: S rows; out_cells: K rows in the order of the cells, or NULL; out_sse: S x A
 * float64, or NULL.  No float atomics, every sum in a fixed order: the same bytes on every run.
 * The profiles are sampled once and parked on the device between the two passes: with the per-age terms 8 ((2h + 1) +
 * 4 A) bytes per cell.  A call runs in chunks of whole segments of at most SC_SEGMENT_MAX_PARK such bytes; a single
 * segment that needs more is SC_ERR_UNSUPPORTED (1.5 million cells at h = 100 and 35 ages, 232 thousand at h = 1024
 * and 64 ages) - this is the largest supported call, next to the limits of sc_fit_profiles (A, h, w, K <= 2^31 - 1,
 * the whole grid on the context), which hold here too.  SC_ERR_INVALID: what sc_fit_profiles refuses, and seg_start
 * not non-decreasing from 0 to K, S < 0, a label <= 0 or not above its predecessor, min_profiles < 1.  The buffers are
 * the call's own: the record, the result planes, the kept spectra, the trace, fill and profile buffers are not
 * touched.  Every kernel is timed under SC_K_PROFILE (there is no slot of its own).
 */
#define SC_SEGMENT_MAX_PARK (1ll << 32)
typedef struct sc_segment_fit {
    int32_t  label;
    int32_t  n_cells;         /* cells of the segment                            */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n;               /* pooled valid points of the usable profiles      */
    int32_t  dof;             /* n - 2 n_profiles - 1                            */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) */
    double   kt, kt_lo, kt_hi;
    double   a;               /* the segment's amplitude: its offset is 2 a      */
    double   sse, rmse;       /* rmse = sqrt(sse / dof)                          */
} sc_segment_fit;
typedef struct sc_segment_cell {
    int64_t  cell;            /* the input cell                                  */
    int32_t  used;            /* 1: a usable profile                             */
    int32_t  n;               /* valid points of the profile                     */
    double   b, c0, sse;      /* at the segment's best age; NaN where not used or the segment is not fitted */
} sc_segment_cell;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                    const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                    int h, int w, double de, double delta, int min_samples, int min_profiles,
                    sc_segment_fit* out_rows, sc_segment_cell* out_cells, double* out_sse);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                        const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                        long long S, const double* ages, int A, int h, int w, double de, double delta,
                        int min_samples, int min_profiles, sc_segment_fit* out_rows, sc_segment_cell* out_cells,
                        double* out_sse);

/*
 * The centre shift (docs/profiles.md, "The centre shift"; docs/segments.md): trace cells do not sit on the scarp's
 * centre, so the step of the model may move along the profile by a whole number of cells,
 *   z(s) = c0 + b s + a erf((s - d de) / (2 sqrt(kt))),   d = -D..D.
 * The profile is sampled exactly as sc_fit_profiles samples it (the same points, the same validity and min_samples
 * rules about j = 0); the erf column of shift d is row j - d of a table over j = -(h + D)..(h + D) whose rows -h..h are
 * the bits of the unshifted table, and for each (age i, shift d) the arithmetic is that of sc_fit_profiles.
 *   single profile  sse*_i = min_d sse_id with d_i its argmin, the candidates taken in the order 0, -1, +1, -2, +2, ...
 *                   and the first smallest winning; kt_index = argmin_i sse*_i (ties to the smallest index),
 *                   shift_index = d_kt_index; a, b, c0, sse are those of that pair.  dof = n - 3 - (D > 0): a cell with
 *                   dof < 1 has status 1 like an unusable one.  rmse = sqrt(sse / dof), thr = sse_min (1 + delta / dof),
 *                   lo_index / hi_index walk along sse* (a profile likelihood over the shift).  Status 1, 2 and 4 as
 *                   sc_fit_profiles; 8: |shift_index| == D with D > 0 - the range ended before the fit did
 *   segment         every usable profile c takes its own d_ci by the single-profile rule at every age; the joint fit
 *                   of sc_fit_segments at age i then has profile c's erf column shifted by d_ci.
 *                   dof = n - 2 n_profiles - 1 - (D > 0 ? n_profiles : 0); status 8: a usable profile of the segment
 *                   has |d_ci| == D at the best age, D > 0.  The parked bytes per cell grow by A (d_ci): 8 ((2h + 1) +
 *                   4 A) + A, which is what SC_SEGMENT_MAX_PARK bounds here
 * D = 0 returns the bytes of sc_fit_profiles / sc_fit_segments in every shared field; a segment of one usable profile
 * returns the kt_index, lo_index, hi_index, status, a, sse and rmse of sc_fit_profiles_shift for that cell and its
 * shift_index in the cell table, bit for bit.  out_sse holds sse* (K x A; S x A for segments: the pooled curve);
 * out_shift: K x A int8 in the order of the cells, or NULL.  sc_fit_profiles_shift: d_i of every age, 0 in the rows of
 * cells with status 1.  sc_fit_segments_shift: d_ci of every age for every USABLE cell - whether or not its segment is
 * fitted (stage one does not know the segment) - and 0 in the rows of cells that are not usable; the cell table's
 * shift_index is 0 wherever its b is NaN.  Refused before any device work: what the unshifted calls refuse, and D < 0 or D > h - min_samples
 * (SC_ERR_INVALID), D > SC_PROFILE_MAX_SHIFT (SC_ERR_UNSUPPORTED).  The same bytes on every run; timed as SC_K_PROFILE.
 */
#define SC_PROFILE_MAX_SHIFT 64
typedef struct sc_profile_shift_fit {
    int64_t  cell;            /* the input cell                                  */
    int32_t  n;               /* valid points of the profile                     */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;   /* the interval, as indices of the age grid   */
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) + 8 (shift at its limit) */
    double   kt, kt_lo, kt_hi;
    double   a, b, c0;        /* of the best (age, shift): the scarp's offset is 2 a */
    double   sse, rmse;       /* rmse = sqrt(sse / dof)                          */
    int32_t  shift_index;     /* d of the best age, in cells (0 where not fitted) */
    double   shift;           /* d de (NaN where not fitted)                     */
} sc_profile_shift_fit;
typedef struct sc_segment_shift_cell {
    int64_t  cell;            /* the input cell                                  */
    int32_t  used;            /* 1: a usable profile                             */
    int32_t  n;               /* valid points of the profile                     */
    double   b, c0, sse;      /* at the segment's best age; NaN where not used or the segment is not fitted */
    int32_t  shift_index;     /* d_ci at the segment's best age (0 where b is NaN) */
} sc_segment_shift_cell;
int sc_fit_profiles_shift(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                          const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples,
                          sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift);
int sc_fit_profiles_shift_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                              const double* ca, long long K, const double* ages, int A, int h, int w, int D, double de,
                              double delta, int min_samples, sc_profile_shift_fit* out_rows, double* out_sse,
                              int8_t* out_shift);
int sc_fit_segments_shift(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                          const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                          int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                          sc_segment_fit* out_rows, sc_segment_shift_cell* out_cells, double* out_sse,
                          int8_t* out_shift);
int sc_fit_segments_shift_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                              const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                              long long S, const double* ages, int A, int h, int w, int D, double de, double delta,
                              int min_samples, int min_profiles, sc_segment_fit* out_rows,
                              sc_segment_shift_cell* out_cells, double* out_sse, int8_t* out_shift);

/*
 * Block-bootstrap intervals of the age of sc_fit_segments (docs/bootstrap.md): a moving-block bootstrap along the strike.
 * The cells of a segment come cut into blocks of neighbouring profiles (CSR over blocks and cells, below); the blocks are
 * resampled with replacement and the segment's shared amplitude and age are re-fitted in every replicate.
 *   stage one   the sampling and parking of sc_fit_segments (D = 0) or sc_fit_segments_shift (D > 0): See_ci, Sep_ci of
 *               every usable profile and age, at d_ci with a shift
 *   block       (sum See_ci, sum Sep_ci) over the block's usable profiles in hand-over order: runs of 64 consecutive
 *               ones summed in sequence from the first, then the run sums in sequence from the first.  A block without a
 *               usable profile stays in the partition with terms (0, 0)
 *   draws       segment s of nb blocks and label L; replicate 0 takes blocks 0..nb-1 once each.  Replicate r = 1..R takes
 *               nb draws k = 0..nb-1: u = mix(mix(seed ^ (L * 0x9E3779B97F4A7C15)) + ((r << 32) | k)) modulo 2^64, mix the
 *               splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *               z ^= z >> 31), block = ((u >> 32) * nb) >> 32.  Integers only; keyed by the label, not by the position
 *   replicate   SSee_i, SSep_i: the drawn blocks' terms added in draw order.  Failed when SSee_i is 0 or not finite at
 *               any age (index -1, a NaN); else kt_index = argmax_i SSep_i^2 / SSee_i (ties to the smallest index; a NaN
 *               never wins), a = SSep / SSee at that age.  This is the argmin of the pooled sse, with nothing subtracted
 *   summary     n_ok replicates of 1..R that did not fail, n_failed the others.  q = (1 - level) / 2 in float64; over the
 *               n_ok indices sorted ascending, lo_index = x[floor(q n_ok)], hi_index = x[ceil((1 - q) n_ok) - 1], taken
 *               from an A-bin integer histogram; a_lo, a_hi by the same ranks over the sorted a; a_mean and a_sd (n - 1;
 *               NaN for n_ok = 1) summed in replicate order.  kt_index0, a0: replicate 0
 *   status      1: not bootstrapped - fewer than min_blocks blocks, fewer than min_profiles usable profiles, or n_ok = 0;
 *               the indices are -1 and the floats NaN.  Otherwise 2 where lo_index == 0, + 4 where hi_index == A - 1
 * seg_blk_start[S + 1]: CSR over blocks, 0 to NB; blk_start[NB + 1]: CSR over cells, 0 to K, with segment s's blocks
 * covering exactly its cells.  R in 1..SC_BOOT_MAX_REPLICATES, 0 < level < 1, min_blocks >= 2.  out_rows: S rows;
 * out_hist: S x A int32 (the histogram of replicates 1..R), out_index: S x (R + 1) int8 and out_a: S x (R + 1) float64
 * (replicate 0 first), each or NULL.  Refused before any device work: what sc_fit_segments_shift refuses (a segment above
 * the park limit included), CSR arrays that do not fit together, R, level or min_blocks out of range.  No float atomics,
 * every sum in a fixed order: the same bytes on every run.  Timed as SC_K_PROFILE.
 */
#define SC_BOOT_MAX_REPLICATES 4096
typedef struct sc_segment_boot {
    int32_t  label;
    int32_t  n_cells;         /* cells of the segment                            */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n_blocks;        /* blocks of the segment, empty ones included      */
    int32_t  replicates;      /* R                                               */
    int32_t  n_failed;        /* replicates of 1..R that failed                  */
    int32_t  kt_index0;       /* replicate 0: every block once                   */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not bootstrapped), or 2 (lo_index == 0) + 4 (hi_index == A - 1) */
    double   kt0, kt_lo, kt_hi;
    double   a0;              /* replicate 0's amplitude                         */
    double   a_mean, a_sd, a_lo, a_hi;
} sc_segment_boot;
int sc_bootstrap_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                          const long long* seg_start, const int32_t* seg_label, long long S,
                          const long long* seg_blk_start, const long long* blk_start, long long NB, const double* ages,
                          int A, int h, int w, int D, double de, int min_samples, int min_profiles, int min_blocks, int R,
                          double level, uint64_t seed, sc_segment_boot* out_rows, int32_t* out_hist, int8_t* out_index,
                          double* out_a);
int sc_bootstrap_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                              const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                              long long S, const long long* seg_blk_start, const long long* blk_start, long long NB,
                              const double* ages, int A, int h, int w, int D, double de, int min_samples, int min_profiles,
                              int min_blocks, int R, double level, uint64_t seed, sc_segment_boot* out_rows,
                              int32_t* out_hist, int8_t* out_index, double* out_a);

/*
 * Joint scarp fits in windows along the strike (docs/strike.md): the offset 2 a and the age kt as functions of the
 * position along a segment.  The cells of a segment arrive sorted along its strike; a window is a contiguous range
 * [win_lo, win_hi) of them (cell indices into `cells`), cut on the host - the library never compares floats to cut a
 * window.  Window g of segment s (seg_win_start[s] <= g < seg_win_start[s + 1]) is station g - seg_win_start[s].  The
 * model is sc_fit_segments' on the window's usable profiles: a and kt shared, an intercept and a slope per profile.
 *   stage one   the sampling and parking of sc_fit_segments (D = 0) or sc_fit_segments_shift (D > 0): See_ci, Sep_ci of
 *               every usable profile and age, at d_ci with a shift - the shifts are stage one's, not re-fitted per window
 *   Spp_c       per usable profile, the sum over its valid points in ascending order of the squared residuals about its
 *               own line b = beta, c0 = pbar - beta sbar: the residual sum of sc_fit_profiles with a = 0
 *   sums        SSee_i, SSep_i, SSpp and the integer n over the window's usable profiles in hand-over order: runs of 64
 *               consecutive ones summed in sequence from the window's first, then the run sums in sequence from the first.
 *               One profile is no addition at all
 *   fit         n_profiles usable profiles, dof = n - 2 n_profiles - 1 - (D > 0 ? n_profiles : 0).  Not fitted (status 1,
 *               indices -1, NaN floats, a NaN curve): n_profiles < min_profiles, dof < 1, SSee_i 0 or not finite at any
 *               age, or no age with a number for Q.  Else Q_i = SSep_i^2 / SSee_i, kt_index = argmax_i Q_i (ties to the
 *               smallest index; a NaN never wins), a = SSep / SSee there; sse_i = max(SSpp - Q_i, 0), sse that of
 *               kt_index, rmse = sqrt(sse / dof); lo_index and hi_index: the run of ages around kt_index with
 *               sse_i <= sse (1 + delta / dof).  Status 2 and 4 as sc_fit_profiles; 8: a usable profile of the window has
 *               |d_ci| == D at the best age, D > 0
 * SSpp - Q_i cancels where the scarp explains almost all of the profiles' energy: the error of sse_i is a few ulps of
 * SSpp, not of sse_i (kt_index and a have no subtraction).  sc_fit_segments' explicit residuals remain the route for a
 * single pooled fit.  An empty window (win_lo == win_hi) is allowed: n_cells 0, status 1.  out_rows: NW rows; out_sse:
 * NW x A (sse_i) or NULL.  Refused before any device work: what sc_fit_segments_shift refuses, CSR arrays or ranges
 * that do not fit together (seg_start[s] <= win_lo <= win_hi <= seg_start[s + 1]), NW > 2^31 - 1.  No float atomics,
 * every sum in a fixed order: the same bytes on every run.  Timed as SC_K_PROFILE.
 */
typedef struct sc_strike_fit {
    int32_t  label;
    int32_t  station;         /* the window's number within its segment          */
    int32_t  n_cells;         /* cells of the window                             */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n;               /* their valid points, pooled                      */
    int32_t  dof;
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) + 8 (a shift at its limit) */
    double   kt, kt_lo, kt_hi;
    double   a;               /* the window's amplitude: its offset is 2 a       */
    double   sse, rmse;       /* rmse = sqrt(sse / dof)                          */
} sc_strike_fit;
int sc_fit_strike(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                  const long long* win_lo, const long long* win_hi, long long NW, const double* ages, int A, int h, int w,
                  int D, double de, double delta, int min_samples, int min_profiles, sc_strike_fit* out_rows,
                  double* out_sse);
int sc_fit_strike_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                      const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                      const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                      const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples,
                      int min_profiles, sc_strike_fit* out_rows, double* out_sse);

/*
 * Intervals per station (docs/strike.md): sc_bootstrap_segments' block bootstrap in every window of sc_fit_strike.
 *   hand-over   the cells, the stations and the windows [win_lo, win_hi) are sc_fit_strike's, unchanged; stage one is
 *               unchanged; with a shift the parked shifts are stage one's and are not re-fitted
 *   blocks      of a window, whose cells are sorted by t: the block of a cell is floor((t_c - t_first) / block_length),
 *               t_first the t of the window's first cell; the blocks that hold a cell are numbered along the strike, a
 *               stretch without a cell is no block.  Cut by the caller in float64 and handed over as integers:
 *               win_blk_start[NW + 1], CSR over blocks, 0 to NWB, and blk_hi[NWB], the end cell (an index into `cells`)
 *               of every block - a window's first block begins at win_lo, every other where the one before ends, the
 *               last ends at win_hi.  The library never compares floats.  A block whose cells have no usable profile
 *               stays in the partition with terms (0, 0)
 *   block terms (sum See_ci, sum Sep_ci) over the block's usable profiles in hand-over order: runs of 64 summed in
 *               sequence from the first, then the run sums in sequence from the first
 *   draws       sc_bootstrap_segments' generator keyed by label L and station: key = mix(seed ^ (L * 0x9E3779B97F4A7C15)
 *               ^ (station * 0xD1B54A32D192ED03)), u = mix(key + ((r << 32) | k)), block = ((u >> 32) * nb) >> 32, all
 *               modulo 2^64: station 0 has sc_bootstrap_segments' key.  Replicate 0 takes every block once
 *   replicate, summary, status: sc_bootstrap_segments' rules per window - the failed rule, argmax_i Q_i with ties to the
 *               smallest index (a NaN never wins), the ranks from an A-bin integer histogram, a_mean and a_sd in
 *               replicate order, a_lo and a_hi by the same ranks over the sorted a.  Status 1: fewer than min_blocks
 *               blocks, fewer than min_profiles usable profiles, n_ok = 0, or an empty window; otherwise 2 where
 *               lo_index == 0, + 4 where hi_index == A - 1
 * A window's block terms must fit 64 KiB: nb A 16 <= 65536, SC_ERR_UNSUPPORTED beyond.  R in 1..SC_BOOT_MAX_REPLICATES,
 * 0 < level < 1, min_blocks >= 2, NW <= 2^31 - 1.  out_rows: NW rows; out_hist: NW x A int32 (the histogram of replicates
 * 1..R) or NULL.  Per-replicate outputs are not built: they would be NW x (R + 1) values.  Refused before any device
 * work: what sc_fit_strike refuses, block arrays that do not tile their windows exactly, R, level or min_blocks out of
 * range.  No float atomics, no float sum across lanes: the same bytes on every run and for every "fit_chunk", and a
 * segment's rows do not depend on the other segments of the call.  Timed as SC_K_PROFILE.
 */
typedef struct sc_strike_boot {
    int32_t  label;
    int32_t  station;         /* the window's number within its segment          */
    int32_t  n_cells;         /* cells of the window                             */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n_blocks;        /* blocks of the window, empty ones included       */
    int32_t  replicates;      /* R                                               */
    int32_t  n_failed;        /* replicates of 1..R that failed                  */
    int32_t  kt_index0;       /* replicate 0: every block once                   */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not bootstrapped), or 2 (lo_index == 0) + 4 (hi_index == A - 1) */
    double   kt0, kt_lo, kt_hi;
    double   a0;              /* replicate 0's amplitude                         */
    double   a_mean, a_sd, a_lo, a_hi;
} sc_strike_boot;
int sc_strike_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                        const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                        const long long* win_lo, const long long* win_hi, long long NW, const double* ages, int A, int h,
                        int w, int D, double de, int min_samples, int min_profiles, const long long* win_blk_start,
                        const long long* blk_hi, long long NWB, int min_blocks, int R, double level, uint64_t seed,
                        sc_strike_boot* out_rows, int32_t* out_hist);
int sc_strike_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                            const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                            long long S, const long long* seg_win_start, const long long* win_lo, const long long* win_hi,
                            long long NW, const double* ages, int A, int h, int w, int D, double de, int min_samples,
                            int min_profiles, const long long* win_blk_start, const long long* blk_hi, long long NWB,
                            int min_blocks, int R, double level, uint64_t seed, sc_strike_boot* out_rows,
                            int32_t* out_hist);

/*
 * Strike-slip offsets across a trace (docs/lateral.md, scarplet_amd/csrc/sc_lateral.hip): at each of K cells two
 * fault-parallel profiles are cut, one on either side of the trace, and the lag along the strike at which they agree
 * best comes back as one sc_lateral_fit.
 *   cells   K linear indices r * nx + c;  sa, ca: sin and cos of the strike's angle at the cell, as sc_fit_profiles
 *           takes them
 *   samples along-strike index t, across index q: rr = r + (t ca - q sa), cc = c + (q ca + t sa) - the point of
 *           sc_fit_profiles with k = t and j = q, inside, interpolated and valid exactly as there
 *   profiles u_t, t = -h..h: the mean of the valid samples at q = -q0, -(q0 + 1), .., -q1, summed in that order;
 *           v_t, t = -(h + D)..(h + D): the same at q = +q0, .., +q1.  NaN where no sample is valid
 *   lag d   in -D..D, over the points t = -h..h with u_t and v_{t + d} both valid (n_d of them, s = t de), every sum
 *           over ascending t: the plain sums of s, u, v give sbar, ubar, vbar; the centred Stt, Stu, Stv give
 *           bu = Stu / Stt and bv = Stv / Stt; with ru = (u - ubar) - bu (s - sbar) and rv likewise, Suu = sum ru^2,
 *           Svv = sum rv^2, Suv = sum ru rv, sse = sum (rv - ru)^2 (explicit residuals).  mse_d = sse / (n_d - 2),
 *           rho_d = Suv / sqrt(Suu Svv), NaN unless Suu Svv > 0.  The lag is skipped - mse_d NaN - when
 *           n_d < min_samples or Stt is not > 0
 *   best    lag = argmin mse_d over the candidates in the order 0, -1, +1, -2, +2, ..: a NaN never wins, the first
 *           smallest wins a tie.  No lag fitted: status 1, n = lag = lo = hi = 0, NaN in every float field
 *   interval thr = mse (1 + delta / (n - 2)); lo walks down from lag while mse[lo - 1] <= thr, hi up likewise (a NaN
 *           stops the walk)
 *   offset  (lag + frac) de: frac = 0.5 (m- - m+) / ((m- - m0) + (m+ - m0)) of the mse at lag - 1, lag, lag + 1
 *           where -D < lag < D, both neighbours are finite and the denominator is > 0; else frac = 0
 *   status  1, or the sum of 2 (lo == -D), 4 (hi == D), 8 (|lag| == D, D > 0), 16 (some lag was skipped)
 * out_rows: K rows in the order of the cells (repeats allowed); out_mse: K x (2 D + 1) float64, mse_d at column
 * d + D, or NULL.  No atomics, every sum in a fixed order: the same bytes on every run and for every order of the
 * cells.  SC_ERR_INVALID: a null argument, K < 0, a cell outside the grid, sa / ca not finite, h < 1, q0 < 1,
 * q1 < q0, D < 0, min_samples < 3 or > 2 h + 1, delta < 0 or not finite, de not finite or <= 0, ny or nx < 2.
 * SC_ERR_UNSUPPORTED: h > SC_PROFILE_MAX_HALF, q1 > SC_LATERAL_MAX_FAR, q1 - q0 + 1 > SC_LATERAL_MAX_BAND,
 * D > SC_LATERAL_MAX_LAG, K > 2^31 - 1, a context that holds a block of a larger grid.  The buffers are those of
 * sc_fit_profiles: the record, the result planes, the kept spectra, the trace and fill buffers are not touched.
 * Timed as SC_K_PROFILE.
 */
#define SC_LATERAL_MAX_LAG   255     /* D                                              */
#define SC_LATERAL_MAX_BAND  64      /* q1 - q0 + 1: the lines averaged on each side   */
#define SC_LATERAL_MAX_FAR   1024    /* q1                                             */
typedef struct sc_lateral_fit {
    int64_t  cell;            /* the input cell                                  */
    int32_t  n;               /* points of the best lag (0: not fitted)          */
    int32_t  lag;             /* best lag, cells along the strike                */
    int32_t  lo, hi;          /* the interval, as lags                           */
    int32_t  status;          /* 1 (not fitted), or 2 (open below) + 4 (open above) + 8 (lag at its limit) + 16 (a lag skipped) */
    double   offset, offset_lo, offset_hi;   /* (lag + frac) de, lo de, hi de    */
    double   mse, rho;        /* of the best lag                                 */
    double   dz, tilt;        /* vbar - ubar and bv - bu there                   */
} sc_lateral_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_lateral_offsets(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K, int h,
                       int q0, int q1, int D, double de, double delta, int min_samples, sc_lateral_fit* out_rows,
                       double* out_mse);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_lateral_offsets_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                           const double* ca, long long K, int h, int q0, int q1, int D, double de, double delta,
                           int min_samples, sc_lateral_fit* out_rows, double* out_mse);

/*
 * Weights and robust fits (docs/profiles.md, "Weights and robust fits"; scarplet_amd/csrc/sc_robust.hip): the fit of
 * sc_fit_profiles with a weight u_j on every point and, per age, T rounds of iteratively reweighted least squares under
 * the Huber or the Tukey loss, on one scale per profile.
 *   samples  as sc_fit_profiles.  With a weight plane (ny x nx float64 on the host, uploaded by the call) the same
 *            bilinear formula is applied to it at the same position; a sample is valid when the elevation sample is
 *            valid and the weight sample is finite and >= 0; p_j and u_j are the means of the two over the same valid k
 *            in ascending k; a point whose u_j is not > 0 is a missing point, and n counts what is left.  weights NULL:
 *            u_j = 1
 *   fit(q)   the four passes of sc_fit_profiles with every sum weighted by q_j, in the same order: W = sum q,
 *            sbar = sum q s / W (pbar, ebar likewise); Sss = sum q sc^2 (Sps, Ses likewise), beta = Sps / Sss,
 *            gamma = Ses / Sss; e2 = (e - ebar) - gamma sc, p2 = (p - pbar) - beta sc, See = sum q e2^2,
 *            Sep = sum q e2 p2; a = Sep / See, b = beta - a gamma, c0 = (pbar - a ebar) - b sbar; r_j the explicit
 *            residuals
 *   iterate 0  q = u for every age; ls_index = argmin of sum u r^2, ties to the smaller index.  loss SC_ROBUST_NONE
 *            stops here: the loss curve is that sum, scale is NaN, n_down 0 and ls_index = kt_index
 *   scale    sigma = `scale` where it is > 0; scale = 0: 1.4826 times the element of rank (n - 1) / 2 (0-based,
 *            ascending; an exact order statistic, no averaging) of |r_j| at ls_index over the n points.  sigma not > 0:
 *            the row of iterate 0 with loss = sse and status 16
 *   iterates t = 1..iterations, per age from that age's previous iterate: q_j = u_j f(|r_j|), c = tuning sigma;
 *            Huber f = 1 where |r| <= c, else c / |r|; Tukey f = (1 - (|r| / c)^2)^2 where |r| < c, else 0; then
 *            fit(q).  An age with fewer than min_samples points with q > 0 on either side of j = 0 at some iterate, or
 *            See not > 0, has loss NaN and never wins
 *   loss     of the last iterate, sum u_j rho(r_j): Huber rho = r^2 where |r| <= c, else 2 c |r| - c^2; Tukey
 *            rho = (c^2 / 3)(1 - (1 - (r / c)^2)^3) where |r| < c, else c^2 / 3
 *   choice   kt_index, lo_index and hi_index as sc_fit_profiles, on the loss curve: thr = loss_min (1 + delta / (n - 3)).
 *            sse = sum u r^2 of the last iterate at kt_index, rmse = sqrt(loss / (n - 3)), n_down = its points whose
 *            f(|r_j|) < 1.  Status 1, 2 and 4 as sc_fit_profiles; 16 as above; 1 | 32: every age's loss is NaN
 * weights NULL (or a plane of ones) with SC_ROBUST_NONE returns the bytes of sc_fit_profiles in every shared field.
 * out_rows: K rows in the order of the cells; out_loss: K x A float64 or NULL.  No atomics, no float sum across lanes,
 * the order statistic by integer counts: the same bytes on every run and for every order of the cells.
 * SC_ERR_INVALID: what sc_fit_profiles refuses, a loss that is none of the three, and with a robust loss a tuning
 * constant not finite or <= 0, iterations < 1, a scale not finite or < 0.  SC_ERR_UNSUPPORTED: what sc_fit_profiles
 * refuses, iterations > SC_ROBUST_MAX_ITER.  The buffers are those of sc_fit_profiles and one for the weight plane.
 * Timed as SC_K_PROFILE.
 */
#define SC_ROBUST_NONE     0
#define SC_ROBUST_HUBER    1
#define SC_ROBUST_TUKEY    2
#define SC_ROBUST_MAX_ITER 64
typedef struct sc_profile_robust_fit {
    int64_t  cell;            /* the input cell                                  */
    int32_t  n;               /* valid points of the profile (u_j > 0)           */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;   /* the interval, as indices of the age grid   */
    int32_t  status;          /* 1, 2, 4 as sc_profile_fit; 16: no scale; 1 | 32: no age survived */
    double   kt, kt_lo, kt_hi;
    double   a, b, c0;        /* of the best age's last iterate                  */
    double   sse, rmse;       /* sum u r^2 there; sqrt(loss / (n - 3))           */
    double   loss, scale;     /* sum u rho(r) there; sigma                       */
    int32_t  n_down;          /* points of that fit with f(|r|) < 1              */
    int32_t  ls_index;        /* best age of iterate 0                           */
} sc_profile_robust_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_profiles_robust(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                           const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                           const double* weights, int loss, double tuning, int iterations, double scale,
                           sc_profile_robust_fit* out_rows, double* out_loss);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_profiles_robust_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                               const double* ca, long long K, const double* ages, int A, int h, int w, double de,
                               double delta, int min_samples, const double* weights, int loss, double tuning,
                               int iterations, double scale, sc_profile_robust_fit* out_rows, double* out_loss);

/*
 * Weights and robust joint fits (docs/segments.md, "Weights and robust fits"; scarplet_amd/csrc/sc_segment_robust.hip): the
 * fit of sc_fit_segments with the weights and the losses of sc_fit_profiles_robust, on ONE scale per segment.
 *   samples  p_cj and u_cj as sc_fit_profiles_robust forms them (weights NULL: u = 1); a profile is usable with at least
 *            min_samples valid points on either side; n is the pooled number of valid points of the usable profiles and
 *            dof = n - 2 n_profiles - 1 (down-weighted points still count); fitted under the rule of sc_fit_segments
 *   fit(q)   per active profile the weighted passes 0 to 2 of sc_fit_profiles_robust give sbar, pbar, beta, ebar, gamma,
 *            See_ci, Sep_ci; a_i = (sum_c Sep_ci) / (sum_c See_ci); b_ci = beta_ci - a_i gamma_ci; c0_ci = (pbar_ci -
 *            a_i ebar_ci) - b_ci sbar_ci; r_cj = p_cj - ((c0_ci + b_ci s_j) + a_i e_ij).  Sums over c: the blocked sum of
 *            sc_fit_segments over the usable profiles in input order; a profile that adds nothing adds +0.0 in its
 *            place, so the shape of the sum depends on n_profiles alone
 *   iterate 0  q = u; ls_index = argmin_i sum_c sum_j u r^2, ties to the smaller index.  SC_ROBUST_NONE ends here, on that
 *            curve, with scale NaN, n_down 0, n_dormant 0 and ls_index = kt_index
 *   scale    `scale` where it is > 0, else ONE sigma per segment: 1.4826 times the element of rank (n - 1) / 2 (0-based,
 *            ascending; an exact order statistic by integer counts) of the pooled |r_cj| at ls_index over all n points of
 *            the usable profiles.  sigma not > 0: the row of iterate 0 with loss = sse and status 16
 *   iterates t = 1..iterations, per age from that age's previous (c0_ci, b_ci, a_i): q_cj = u_cj f(|r_cj|), c = tuning
 *            sigma, f and rho those of sc_fit_profiles_robust; then fit(q).  A profile with fewer than min_samples points
 *            of q > 0 at j < 0, or at j > 0, is DORMANT at that iterate and age: it adds +0.0 to both sums (no say in
 *            a_i), keeps the (c0, b) of the last iterate in which it was active, has its residuals re-formed with the new
 *            a_i and may wake at a later iterate.  An age whose sum See is not > 0 at some iterate has loss NaN from then
 *            on and never wins (the age at which every profile is dormant among them)
 *   loss     of the last iterate, sum_c sum_j u rho(r), through the blocked sum
 *   choice   kt_index, lo_index, hi_index as sc_fit_segments, on the loss curve: thr = loss_min (1 + delta / dof).  sse =
 *            sum u r^2 there, rmse = sqrt(loss / dof), n_down = the points of that fit with f < 1 over the profiles,
 *            n_dormant = the profiles dormant in it.  Status 1, 2, 4 as sc_fit_segments; 16 as above; 1 | 32: every
 *            age's loss is NaN - indices -1, floats NaN, scale stays
 * weights NULL (or a plane of ones) with SC_ROBUST_NONE returns the bytes of sc_fit_segments in every shared field of
 * rows, cell table and curve; a segment of one usable profile returns kt_index, lo_index, hi_index, status, a, sse, rmse,
 * loss, scale, n_down and ls_index of sc_fit_profiles_robust for that cell, and its b and c0 in the cell table, bit for
 * bit.  out_rows: S rows; out_cells: K rows in the order of the cells, or NULL (b, c0, sse of the final fit at the best
 * age, the profile's share of the loss, its down-weighted points, 1 where it was dormant); out_loss: S x A float64, or NULL.
 * Integer atomics in the order statistic alone; no float atomics, every float sum in a fixed order: the same bytes on every
 * run and for every order of the segments.
 * The park: per cell the profile, its weights where there is a plane, and SC_SEGMENT_ROBUST_PLANES planes per age (sbar, pbar,
 * beta, ebar, gamma, See, Sep, c0, b) - 8 ((2h + 1)(1 + plane) + 9 A) bytes.  Chunks are whole segments of at most
 * SC_SEGMENT_MAX_PARK such bytes; a single segment that needs more is SC_ERR_UNSUPPORTED.  SC_ERR_INVALID and
 * SC_ERR_UNSUPPORTED otherwise as sc_fit_segments and sc_fit_profiles_robust return them, before any launch.  The buffers
 * are those of sc_fit_segments and four of the call's own.  Timed as SC_K_PROFILE.
 */
#define SC_SEGMENT_ROBUST_PLANES 9
typedef struct sc_segment_robust_fit {
    int32_t  label;
    int32_t  n_cells;         /* cells of the segment                            */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n;               /* pooled valid points of the usable profiles      */
    int32_t  dof;             /* n - 2 n_profiles - 1                            */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 1, 2, 4 as sc_segment_fit; 16: no scale; 1 | 32: no age survived */
    double   kt, kt_lo, kt_hi;
    double   a;               /* the segment's amplitude: its offset is 2 a      */
    double   sse, rmse;       /* sum u r^2 at the best age; sqrt(loss / dof)     */
    double   loss, scale;     /* sum u rho(r) there; the segment's sigma         */
    int32_t  n_down;          /* points of that fit with f(|r|) < 1              */
    int32_t  ls_index;        /* best age of iterate 0                           */
    int32_t  n_dormant;       /* profiles dormant in that fit                    */
} sc_segment_robust_fit;
typedef struct sc_segment_robust_cell {
    int64_t  cell;            /* the input cell                                  */
    int32_t  used;            /* 1: a usable profile                             */
    int32_t  n;               /* valid points of the profile                     */
    double   b, c0, sse;      /* of the final fit at the segment's best age; NaN where not used or the segment is not fitted */
    double   loss;            /* the profile's share of the segment's loss       */
    int32_t  n_down;          /* its points with f(|r|) < 1                      */
    int32_t  dormant;         /* 1: dormant in that fit                          */
} sc_segment_robust_cell;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_segments_robust(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                           const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                           int h, int w, double de, double delta, int min_samples, int min_profiles,
                           const double* weights, int loss, double tuning, int iterations, double scale,
                           sc_segment_robust_fit* out_rows, sc_segment_robust_cell* out_cells, double* out_loss);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_segments_robust_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                               const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                               long long S, const double* ages, int A, int h, int w, double de, double delta,
                               int min_samples, int min_profiles, const double* weights, int loss, double tuning,
                               int iterations, double scale, sc_segment_robust_fit* out_rows,
                               sc_segment_robust_cell* out_cells, double* out_loss);

/*
 * The initial slope (docs/profiles.md, "The initial slope"; scarplet_amd/csrc/sc_ramp.hip): the fit of sc_fit_profiles
 * with the scarp started as a ramp of half-width L = m de, not as a vertical step (Hanks & Andrews 1989).  The initial
 * profile b s + a clamp(s / L, -1, 1), diffused for kt, is
 *   z(s) = c0 + b s + a g(s; kt, L),   g = (F(s + L) - F(s - L)) / (2 L),
 *   F(x) = x erf(x / (2 sqrt(kt))) + 2 sqrt(kt / pi) exp(-x^2 / (4 kt)),   F' = erf(x / (2 sqrt(kt))),
 * and g -> erf(s / (2 sqrt(kt))) as L -> 0.  m = 0..M is a whole number of cells.
 *   samples  as sc_fit_profiles: the same points, validity rule, n, n_neg, n_pos and min_samples rule
 *   tables   Ftab over x = -(h + M)..(h + M) and the A ages: with X = (double)x de, X erf(X / (2 sqrt(kt_i))) +
 *            (2 sqrt(kt_i / pi)) exp(-(X X) / (4 kt_i)); the erf table of sc_fit_profiles serves m = 0
 *   column   m = 0: e_ij is the erf table's entry; m >= 1: e_ij = (Ftab[j + m][i] - Ftab[j - m][i]) / (2 m de), the
 *            divisor formed as (double)(2 m) de
 *   fit      for each pair (age i, half-width m) the four passes of sc_fit_profiles with that column; n, sbar, pbar, Sss,
 *            beta and p2 depend on neither and are formed once.  A pair whose See is not > 0, or whose sse is NaN, never
 *            wins
 *   per age  SC_RAMP_FREE: m_i = argmin_m sse_im over m = 0..M, the first smallest winning.  SC_RAMP_SLOPE: over
 *            m = 1..M the key | |b_im + a_im / (m de)| - slope |, the first smallest winning; m = 0, an infinite slope,
 *            is no candidate.  sse*_i = sse_{i, m_i} in both modes (NaN where no pair of the age can win)
 *   choice   kt_index = argmin_i sse*_i, ties to the smaller index; dof = n - 3 - (M > 0) with SC_RAMP_FREE, n - 3 with
 *            SC_RAMP_SLOPE (the constraint fixes the width); dof < 1 gives status 1.  rmse = sqrt(sse / dof), thr =
 *            sse_min (1 + delta / dof), lo_index / hi_index walk along sse*.  Status 1, 2 and 4 as sc_fit_profiles; 8:
 *            width_index == M with M > 0 - the range ended before the fit did
 * M = 0 returns the bytes of sc_fit_profiles in every shared field.  out_rows: K rows in the order of the cells; out_sse:
 * K x A float64 (sse*) or NULL; out_width: K x A int8 (m_i of every age, 0 in the rows of cells with status 1) or NULL.
 * `slope` is read with SC_RAMP_SLOPE alone.  Refused before any device work: what sc_fit_profiles refuses, and M < 0,
 * M > h - min_samples, a mode that is neither, SC_RAMP_SLOPE with M < 1 or a slope that is not finite and > 0
 * (SC_ERR_INVALID); M > SC_PROFILE_MAX_WIDTH (SC_ERR_UNSUPPORTED).  No atomics, no float sum across lanes: the same bytes
 * on every run and for every order of the cells.  The buffers are those of sc_fit_profiles_shift and one for Ftab.
 * Timed as SC_K_PROFILE.
 */
#define SC_PROFILE_MAX_WIDTH 64
#define SC_RAMP_FREE  0
#define SC_RAMP_SLOPE 1
typedef struct sc_profile_ramp_fit {
    int64_t  cell;            /* the input cell                                  */
    int32_t  n;               /* valid points of the profile                     */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;   /* the interval, as indices of the age grid   */
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) + 8 (width at its limit) */
    double   kt, kt_lo, kt_hi;
    double   a, b, c0;        /* of the best (age, half-width): the scarp's offset is 2 a */
    double   sse, rmse;       /* rmse = sqrt(sse / dof)                          */
    int32_t  width_index;     /* m of the best age, in cells (0 where not fitted) */
    double   width;           /* m de, the half-width L (NaN where not fitted)   */
    double   initial_slope;   /* b + a / (m de), signed; copysign(inf, a) at m = 0; NaN where not fitted */
} sc_profile_ramp_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_profiles_ramp(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                         const double* ages, int A, int h, int w, int M, int mode, double slope, double de, double delta,
                         int min_samples, sc_profile_ramp_fit* out_rows, double* out_sse, int8_t* out_width);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_profiles_ramp_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                             const double* ca, long long K, const double* ages, int A, int h, int w, int M, int mode,
                             double slope, double de, double delta, int min_samples, sc_profile_ramp_fit* out_rows,
                             double* out_sse, int8_t* out_width);

/*
 * Channel depth and width across a trace (docs/channels.md): what sc_fit_profiles is to a Scarp search, for a Channel
 * search.  The Ricker window W = (1 - 2 u^2) exp(-u^2), u = pi f x, is -1 / (2 (pi f)^2) times the second derivative of
 * exp(-(pi f x)^2), so the elevation model of that search is a Gaussian trough across the strike,
 *   z(s) = c0 + b s + a exp(-(pi f (s - d de))^2),   d = -D..D,
 * a < 0 for a channel and a > 0 for a ridge; f is the search's own parameter and -2 (pi f)^2 a its amplitude.
 *   samples  as sc_fit_profiles: the same points, validity rule, n, n_neg, n_pos and min_samples rule
 *   table    G over x = -(h + D)..(h + D) and the F frequencies, frequency-minor: with X = (double)x de and
 *            u = (pi f_i) X the entry is exp(-(u u)); the column of shift d is row j - d
 *   fit      for each pair (frequency i, shift d) the four passes of sc_fit_profiles with that column; n, sbar, pbar, Sss,
 *            beta and p2 depend on neither and are formed once.  A pair whose See is not > 0 - no entry of its column
 *            on the profile's points is above 0 - or whose sse is NaN never wins
 *   choice   d_i = argmin_d sse_id in the order 0, -1, +1, -2, ..., the first smallest winning; sse*_i = sse_{i, d_i}
 *            (NaN, with d_i = 0, where no pair of the frequency can win); kt_index = argmin_i sse*_i, ties to the
 *            smaller index, a NaN counting as +inf; dof = n - 3 - (D > 0), and dof < 1 gives status 1; rmse =
 *            sqrt(sse / dof), thr = sse_min (1 + delta / dof), lo_index / hi_index walk along sse* and a NaN ends a walk.
 *            Status 1, 2 and 4 as sc_fit_profiles; 8: |shift_index| == D with D > 0; 1 | 32: no frequency has a pair
 *            that can win, and the row is that of a cell that is not fitted
 * The rows are sc_profile_shift_fit with kt, kt_lo and kt_hi carrying f, and kt_index, lo_index and hi_index indices of
 * the frequencies.  out_rows: K rows in the order of the cells; out_sse: K x F float64 (sse*) or NULL; out_shift: K x F
 * int8 (d_i, 0 in the rows of cells with status & 1) or NULL.  Refused before any device work: what sc_fit_profiles_shift
 * refuses with the frequencies for the ages - finite, > 0, strictly increasing (SC_ERR_INVALID), F >
 * SC_CHANNEL_MAX_FREQS (SC_ERR_UNSUPPORTED) - and (pi f) de > SC_CHANNEL_MAX_ARG (SC_ERR_INVALID): a Gaussian narrower
 * than anything a grid shows, whose neighbouring table entries leave the normal range.
 * For a profile without a missing point ebar, gamma and See of a pair depend on (i, d, h, de) alone: with option
 * "channel_terms" 1 (default) they are formed once per call by the loops of the fit on a profile of zeros, and such a
 * profile runs two sweeps per pair for four.  The same operations in the same order: every output byte is the same with
 * the option 0.  No atomics, no float sum across lanes: the same bytes on every run, for every order of the cells and
 * for every "fit_chunk".  The buffers are those of sc_fit_profiles_shift and one for the terms.  Timed as SC_K_PROFILE.
 */
#define SC_CHANNEL_MAX_FREQS 64
#define SC_CHANNEL_MAX_ARG   6.0
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_channel_profiles(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                        const double* frequencies, int F, int h, int w, int D, double de, double delta, int min_samples,
                        sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_channel_profiles_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                            const double* ca, long long K, const double* frequencies, int F, int h, int w, int D,
                            double de, double delta, int min_samples, sc_profile_shift_fit* out_rows, double* out_sse,
                            int8_t* out_shift);

/*
 * One channel width per reach (docs/channels.md, "One width per reach"): what sc_fit_segments_shift is to
 * sc_fit_profiles_shift, for sc_channel_profiles.  The cells, (sa, ca), the CSR array seg_start, the labels, h, w,
 * min_profiles and the order of the outputs are sc_fit_segments'; the frequencies, D and their limits are
 * sc_channel_profiles'.
 *   samples  a profile is cut as sc_channel_profiles cuts it and is usable with min_samples valid points on either side
 *            of j = 0; n is the pooled count of valid points over the usable profiles, n_profiles their number
 *   stage    every usable profile c takes at every frequency i the single-profile choice of sc_channel_profiles: d_ci over
 *            d = -D..D in the order 0, -1, +1, ..., the first smallest sse winning and a dead pair never; with it sse*_ci,
 *            a_ci, b_ci, c0_ci and the orthogonalised terms ebar, gamma, See, Sep at d_ci - the bits sc_channel_profiles
 *            forms, on either of its routes (option "channel_terms").  A frequency with no live pair in profile c has NaN
 *            there and d_ci = 0
 *   mode     SC_CHANNEL_DEPTH_PROFILE: the frequency is the reach's; depth, intercept, slope and centre are each profile's
 *            own.  sse_i = sum_c sse*_ci, the row's a is abar_i = (sum_c a_ci) / n_profiles at the best frequency, dof =
 *            n - (3 + (D > 0)) n_profiles.
 *            SC_CHANNEL_DEPTH_SEGMENT: the fixed-effects fit of sc_fit_segments_shift on the Gaussian column.  a_i =
 *            (sum_c Sep_ci) / (sum_c See_ci), b_ci and c0_ci follow, sse_ci is that of the explicit residuals with the
 *            column at d_ci, sse_i = sum_c sse_ci, dof = n - 2 n_profiles - 1 - (D > 0 ? n_profiles : 0); a frequency whose
 *            sum of See is not > 0 is dead
 *   sums     over the usable profiles in input order: blocks of 64 in sequence from the first term, then the block sums in
 *            sequence; one profile is no addition at all.  NaN propagates: a frequency that is dead in one usable profile
 *            of the reach is dead for the reach
 *   choice   fitted when n_profiles >= min_profiles and dof >= 1, else status 1, indices -1, NaN floats.  kt_index = argmin
 *            sse_i, ties to the smaller index, a NaN counting as +inf; rmse = sqrt(sse / dof), thr = sse_min (1 + delta /
 *            dof); lo_index / hi_index walk along the curve and a NaN ends a walk.  Status 2 / 4: the interval is open
 *            below / above; 8: a usable profile has |d_ci| == D at the best frequency, D > 0; 1 | 32: every frequency is
 *            dead, and the row is that of a reach that is not fitted
 * The rows are sc_segment_fit with kt, kt_lo and kt_hi carrying f, and kt_index, lo_index and hi_index indices of the
 * frequencies.  A reach of one usable profile returns, in both modes, the kt_index, lo_index, hi_index, status, a, sse and
 * rmse of sc_channel_profiles for that cell, and its b, c0 and shift_index in the cell table, bit for bit.  out_rows: S
 * rows; out_cells: K cells in the order of the cells, or NULL; out_sse: S x F float64, the pooled curves, or NULL;
 * out_shift: K x F int8, d_ci of every USABLE cell whether or not its reach is fitted, 0 in the rows of the others, or NULL.
 * The park per cell is SC_CHANNEL_SEGMENT_PARK(h, F) bytes in both modes - sc_fit_segments_shift's - counted against
 * SC_SEGMENT_MAX_PARK: a call runs in chunks of whole reaches, and a single reach that needs more is SC_ERR_UNSUPPORTED.
 * Refused before any device work: what sc_fit_segments_shift refuses with the frequencies for the ages, what
 * sc_channel_profiles refuses of the frequencies (SC_ERR_INVALID; F > SC_CHANNEL_MAX_FREQS: SC_ERR_UNSUPPORTED; (pi f) de >
 * SC_CHANNEL_MAX_ARG: SC_ERR_INVALID), and a mode that is neither of the two (SC_ERR_INVALID).  No atomics, no float sum
 * across lanes: the same bytes on every run, for every "fit_chunk" and for whole reaches handed over in any order.  Timed as
 * SC_K_PROFILE.
 */
#define SC_CHANNEL_DEPTH_PROFILE 0
#define SC_CHANNEL_DEPTH_SEGMENT 1
#define SC_CHANNEL_SEGMENT_PARK(h, F) (8 * ((2 * (h) + 1) + 4 * (F)) + (F))
typedef struct sc_channel_segment_cell {
    int64_t  cell;            /* the input cell                                  */
    int32_t  used;            /* 1: a usable profile                             */
    int32_t  n;               /* valid points of the profile                     */
    double   a, b, c0, sse;   /* at the reach's best frequency (a: the profile's own, or the reach's in segment mode); NaN
                                 where not used or the reach is not fitted       */
    int32_t  shift_index;     /* d_ci at the reach's best frequency (0 where b is NaN) */
} sc_channel_segment_cell;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_channel_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                        const long long* seg_start, const int32_t* seg_label, long long S, const double* frequencies, int F,
                        int h, int w, int D, int mode, double de, double delta, int min_samples, int min_profiles,
                        sc_segment_fit* out_rows, sc_channel_segment_cell* out_cells, double* out_sse, int8_t* out_shift);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_channel_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                            const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                            long long S, const double* frequencies, int F, int h, int w, int D, int mode, double de,
                            double delta, int min_samples, int min_profiles, sc_segment_fit* out_rows,
                            sc_channel_segment_cell* out_cells, double* out_sse, int8_t* out_shift);

/*
 * Block-bootstrap intervals per reach (docs/channels.md, "Intervals per reach"): what sc_bootstrap_segments is to
 * sc_fit_segments_shift, for sc_channel_segments.  The cells, (sa, ca), the CSR arrays over reaches, blocks and cells, R,
 * level, seed and min_blocks are sc_bootstrap_segments'; the frequencies, D, the mode and their limits sc_channel_segments'.
 *   stage one   sc_channel_segments': the same samples, the same d_ci and the same terms per usable profile and frequency,
 *               NaN where the frequency has no live pair in the profile.  No residual pass in either mode
 *   block       over the block's usable profiles in hand-over order - runs of 64 in sequence from the first, then the run
 *               sums in sequence from the first -: SC_CHANNEL_DEPTH_SEGMENT (sum See_ci, sum Sep_ci); SC_CHANNEL_DEPTH_PROFILE
 *               (sum sse*_ci, sum a_ci) and m_b, the block's usable profiles.  NaN propagates; an empty block has terms 0
 *               and m_b = 0 and stays in the partition
 *   draws       sc_bootstrap_segments', bit for bit: keyed by seed and label, replicate 0 takes every block once
 *   replicate   the sums of the drawn blocks' terms in draw order.  SC_CHANNEL_DEPTH_SEGMENT: frequency i is live when
 *               SSee_i > 0 and finite and Q_i = SSep_i^2 / SSee_i is a number; f_index = argmax Q_i over the live ones, ties to
 *               the smaller index; a = SSep / SSee there.  SC_CHANNEL_DEPTH_PROFILE: M = sum m_b over the draws; i is live
 *               when M > 0 and SSse_i is a number; f_index = argmin SSse_i over the live ones, ties to the smaller index;
 *               a = SA_i / (double)M there.  A frequency that is dead in a drawn profile is dead for that replicate only;
 *               the replicate is failed (index -1, a NaN) only when no frequency is live
 *   summary     sc_bootstrap_segments' over the n_ok replicates of 1..R that did not fail: lo_index and hi_index by its
 *               ranks on an F-bin integer histogram, a_mean and a_sd in replicate order, a_lo and a_hi by the same ranks on
 *               the sorted a; and the same four of area_r = -a_r / (sqrt(pi) f[index_r]).  f_index0, a0, area0: replicate 0
 *   status      1: not bootstrapped - fewer than min_blocks blocks, fewer than min_profiles usable profiles, or n_ok = 0;
 *               the indices are -1 and the floats NaN; 1 | 32 where the reach has the blocks and the profiles, n_ok = 0
 *               and replicate 0 has no live frequency either.  Otherwise 2 where lo_index == 0, + 4 where hi_index == F - 1
 * out_rows: S rows; out_hist: S x F int32 (the histogram of replicates 1..R), out_index: S x (R + 1) int8 and out_a: S x
 * (R + 1) float64 (replicate 0 first), each or NULL.  Refused before any device work: what sc_channel_segments refuses (a
 * reach above the park limit included) and what sc_bootstrap_segments refuses of the block arrays, R, level and min_blocks.
 * No float atomics, every sum in a fixed order: the same bytes on every run, whatever other reaches the call holds.  Timed
 * as SC_K_PROFILE.
 */
typedef struct sc_channel_boot {
    int32_t  label;
    int32_t  n_cells;         /* cells of the reach                              */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n_blocks;        /* blocks of the reach, empty ones included        */
    int32_t  replicates;      /* R                                               */
    int32_t  n_failed;        /* replicates of 1..R without a live frequency     */
    int32_t  f_index0;        /* replicate 0: every block once                   */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not bootstrapped; | 32), or 2 (lo_index == 0) + 4 (hi_index == F - 1) */
    double   f0, f_lo, f_hi;
    double   a0;              /* replicate 0's depth coefficient                 */
    double   a_mean, a_sd, a_lo, a_hi;
    double   area0;           /* -a0 / (sqrt(pi) f0)                             */
    double   area_mean, area_sd, area_lo, area_hi;
} sc_channel_boot;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_channel_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                         const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_blk_start,
                         const long long* blk_start, long long NB, const double* frequencies, int F, int h, int w, int D,
                         int mode, double de, int min_samples, int min_profiles, int min_blocks, int R, double level,
                         uint64_t seed, sc_channel_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_channel_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                             const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                             long long S, const long long* seg_blk_start, const long long* blk_start, long long NB,
                             const double* frequencies, int F, int h, int w, int D, int mode, double de, int min_samples,
                             int min_profiles, int min_blocks, int R, double level, uint64_t seed, sc_channel_boot* out_rows,
                             int32_t* out_hist, int8_t* out_index, double* out_a);

/*
 * A channel's width in windows along the strike of a reach (docs/channels.md, "Width along a reach"): what sc_fit_strike is
 * to sc_fit_segments_shift, for sc_channel_segments.  The cells, (sa, ca), the CSR arrays over reaches, windows and cells
 * and the windows [win_lo, win_hi) are sc_fit_strike's - the cells of a reach sorted along its strike, the windows cut on
 * the host, no float compared here to cut one -; the frequencies, D, the mode and their limits sc_channel_segments'.
 *   stage one   sc_channel_segments': the same samples, the same d_ci and the same terms per usable profile and frequency,
 *               NaN where the frequency has no live pair in the profile.  The shifts are not re-fitted per window
 *   sums        over the window's usable profiles in hand-over order - runs of 64 in sequence from the window's first, then
 *               the run sums in sequence from the first; one profile is no addition at all -, with the integers n and
 *               n_profiles.  NaN propagates: a frequency that is dead in one usable profile of the window is dead for the
 *               window (sc_channel_segments' rule, not the bootstrap's)
 *   mode        SC_CHANNEL_DEPTH_PROFILE: the sums of (sse*_ci, a_ci).  sse_i = SSse_i, kt_index = argmin sse_i, ties to
 *               the smaller index, a NaN counting as +inf; a = SA / (double)n_profiles there; dof = n - (3 + (D > 0))
 *               n_profiles.  No subtraction anywhere.
 *               SC_CHANNEL_DEPTH_SEGMENT: the sums of (See_ci, Sep_ci) and of Spp_c, sc_fit_strike's quantity - the
 *               profile's squared residuals about its own line.  Frequency i is live when SSee_i > 0 and finite and Q_i =
 *               SSep_i^2 / SSee_i is a number; kt_index = argmax Q_i over the live ones, ties to the smaller index; a =
 *               SSep / SSee there; sse_i = max(SSpp - Q_i, 0) where live, NaN where dead; dof = n - 2 n_profiles - 1 -
 *               (D > 0 ? n_profiles : 0).  SSpp - Q_i cancels where the trough explains almost all of the profiles'
 *               energy: the error of sse_i is a few ulps of SSpp, not of sse_i (kt_index and a have no subtraction)
 *   choice      not fitted (status 1, indices -1, NaN floats, a NaN curve): n_profiles < min_profiles or dof < 1; 1 | 32:
 *               every frequency is dead.  Else rmse = sqrt(sse / dof), thr = sse (1 + delta / dof); lo_index and hi_index
 *               walk along the curve and a NaN ends a walk.  Status 2 / 4: the interval is open below / above; 8: a usable
 *               profile of the window has |d_ci| == D at the best frequency, D > 0
 * The rows are sc_strike_fit with kt, kt_lo and kt_hi carrying f, and kt_index, lo_index and hi_index indices of the
 * frequencies.  An empty window is allowed.  out_rows: NW rows; out_sse: NW x F float64 (sse_i) or NULL; out_shift_sum: NW
 * int32, the sum of d_ci at the best frequency over the window's usable profiles (0 where the window is not fitted), or
 * NULL.  The park per cell is SC_CHANNEL_SEGMENT_PARK(h, F) bytes, as for sc_channel_segments.  Refused before any device
 * work: what sc_channel_segments refuses (a reach above the park limit included) and what sc_fit_strike refuses of the
 * window arrays.  No atomics, no float sum across lanes: the same bytes on every run, for every "fit_chunk" and whatever
 * other reaches the call holds.  Timed as SC_K_PROFILE.
 */
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_channel_strike(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                      const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                      const long long* win_lo, const long long* win_hi, long long NW, const double* frequencies, int F,
                      int h, int w, int D, int mode, double de, double delta, int min_samples, int min_profiles,
                      sc_strike_fit* out_rows, double* out_sse, int32_t* out_shift_sum);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_channel_strike_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                          const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                          const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                          const double* frequencies, int F, int h, int w, int D, int mode, double de, double delta,
                          int min_samples, int min_profiles, sc_strike_fit* out_rows, double* out_sse,
                          int32_t* out_shift_sum);

/*
 * Block-bootstrap intervals per station along a reach (docs/channels.md, "Intervals per station"): what sc_strike_bootstrap
 * is to sc_fit_strike, for sc_channel_strike - sc_channel_bootstrap's block bootstrap in every window of sc_channel_strike.
 *   hand-over   the cells, the stations and the windows [win_lo, win_hi) are sc_channel_strike's, unchanged
 *   stage one   sc_channel_segments': the same samples, the same d_ci and the same terms per usable profile and frequency,
 *               NaN where the frequency has no live pair in the profile.  The shifts are not re-fitted per window or per
 *               replicate.  No residual pass and no Spp in either mode
 *   blocks      sc_strike_bootstrap's, cut by the caller in float64 and handed over as integers: win_blk_start[NW + 1], CSR
 *               over blocks, 0 to NWB, and blk_hi[NWB], the end cell of every block - a window's first block begins at
 *               win_lo, every other where the one before ends, the last ends at win_hi.  The library never compares floats
 *   block terms sc_channel_bootstrap's, over the block's usable profiles in hand-over order - runs of 64 in sequence from
 *               the first, then the run sums in sequence from the first -: SC_CHANNEL_DEPTH_SEGMENT (sum See_ci, sum
 *               Sep_ci); SC_CHANNEL_DEPTH_PROFILE (sum sse*_ci, sum a_ci) and the integer m_b, the block's usable profiles.
 *               NaN propagates; an empty block has terms 0 and m_b = 0 and stays in the partition
 *   draws       sc_strike_bootstrap's generator, bit for bit: keyed by seed, label and station - station 0 has
 *               sc_channel_bootstrap's key -; replicate 0 takes every block once
 *   replicate   sc_channel_bootstrap's rules on the sums of the drawn blocks' terms in draw order: the live rule of the
 *               mode; f_index = argmax Q_i or argmin SSse_i over the live frequencies, ties to the smaller index; a = SSep /
 *               SSee or SA_i / (double)M there, M = sum m_b over the draws.  A frequency that is dead in a drawn profile is
 *               dead for that replicate only; the replicate is failed only when no frequency is live
 *   summary     sc_channel_bootstrap's per window, over the n_ok replicates of 1..R that did not fail: lo_index and hi_index
 *               by its ranks on an F-bin integer histogram, a_mean and a_sd in replicate order, a_lo and a_hi by the same
 *               ranks on the sorted a; and the same four of area_r = -a_r / (sqrt(pi) f[index_r]).  f_index0, a0, area0:
 *               replicate 0
 *   status      1: not bootstrapped - fewer than min_blocks blocks, fewer than min_profiles usable profiles, n_ok = 0, or
 *               an empty window; the indices are -1 and the floats NaN; 1 | 32 where the window has the blocks and the
 *               profiles, n_ok = 0 and replicate 0 has no live frequency either.  Otherwise 2 where lo_index == 0, + 4
 *               where hi_index == F - 1
 * A window's block terms must fit 64 KiB: nb F 16 <= 65536, SC_ERR_UNSUPPORTED beyond.  out_rows: NW rows; out_hist: NW x F
 * int32 (the histogram of replicates 1..R) or NULL.  Per-replicate outputs are not built: they would be NW x (R + 1) values.
 * The park per cell is SC_CHANNEL_SEGMENT_PARK(h, F) bytes, as for sc_channel_segments.  Refused before any device work:
 * what sc_channel_strike refuses (a reach above the park limit included) and what sc_strike_bootstrap refuses of the block
 * arrays, R, level and min_blocks.  No float atomics, no float sum across lanes: the same bytes on every run and for every
 * "fit_chunk", and a reach's rows do not depend on the other reaches of the call.  Timed as SC_K_PROFILE.
 */
typedef struct sc_channel_strike_boot {       /* sc_channel_boot with the station */
    int32_t  label;
    int32_t  station;         /* the window's number within its reach            */
    int32_t  n_cells;         /* cells of the window                             */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n_blocks;        /* blocks of the window, empty ones included       */
    int32_t  replicates;      /* R                                               */
    int32_t  n_failed;        /* replicates of 1..R without a live frequency     */
    int32_t  f_index0;        /* replicate 0: every block once                   */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not bootstrapped; | 32), or 2 (lo_index == 0) + 4 (hi_index == F - 1) */
    double   f0, f_lo, f_hi;
    double   a0;              /* replicate 0's depth coefficient                 */
    double   a_mean, a_sd, a_lo, a_hi;
    double   area0;           /* -a0 / (sqrt(pi) f0)                             */
    double   area_mean, area_sd, area_lo, area_hi;
} sc_channel_strike_boot;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_channel_strike_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                const long long* seg_start, const int32_t* seg_label, long long S,
                                const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                                const double* frequencies, int F, int h, int w, int D, int mode, double de, int min_samples,
                                int min_profiles, const long long* win_blk_start, const long long* blk_hi, long long NWB,
                                int min_blocks, int R, double level, uint64_t seed, sc_channel_strike_boot* out_rows,
                                int32_t* out_hist);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_channel_strike_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                    const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                    long long S, const long long* seg_win_start, const long long* win_lo,
                                    const long long* win_hi, long long NW, const double* frequencies, int F, int h, int w,
                                    int D, int mode, double de, int min_samples, int min_profiles,
                                    const long long* win_blk_start, const long long* blk_hi, long long NWB, int min_blocks,
                                    int R, double level, uint64_t seed, sc_channel_strike_boot* out_rows, int32_t* out_hist);

/*
 * Continuous ages (docs/profiles.md, "Continuous ages"; scarplet_amd/csrc/sc_refine.hip): the fit of sc_fit_profiles, and
 * after it R levels of 64 candidate ages of the cell's OWN bracket - for the minimum and for either end of the interval.
 * The samples, the validity rule, the min_samples rule, the orthogonalised fit and the explicit-residual sse are those of
 * sc_fit_profiles; every field of sc_profile_fit, and out_sse, are its bytes.
 *   column     of a candidate age x (a double): e_j = erf((double)j de / (2.0 sqrt(x))), the expression of the erf table -
 *              at a grid age the table's bits
 *   candidates of a bracket [p, q]: x_l = p + (q - p) ((double)l / 63.0) for l = 0..62 and x_63 = q; each is fitted by the
 *              four passes of sc_fit_profiles with its column.  A NaN sse counts as +inf
 *   status 1   every *_fine float is NaN, status_fine = 1
 *   minimum    i = kt_index.  The first bracket is [ages[max(i - 1, 0)], ages[min(i + 1, A - 1)]].  R times: fit the 64
 *              candidates, l* = argmin of their sse (ties to the smaller l), the next bracket is [x_max(l* - 1, 0),
 *              x_min(l* + 1, 63)].  kt_fine = x_l* of the last level with its a, b, c0, sse - unless that sse is not <=
 *              the grid's sse[i], or R = 0: then ages[i] with the grid's a, b, c0, sse.  So sse_fine <= sse.
 *              rmse_fine = sqrt(sse_fine / (n - 3)), height_fine = 2 a_fine
 *   interval   thr = sse_fine (1 + delta / (n - 3)).
 *              lower end: g = the largest grid index with ages[g] <= kt_fine; j = g, g - 1, ... while j >= 0 and the
 *              grid's sse[j] <= thr.  Off the grid: kt_lo_fine = ages[0] and status_fine gains 2.  Else outer = ages[j],
 *              inner = ages[j + 1] if j + 1 <= g, else kt_fine; R times over [outer, inner]: fit the candidates, take the
 *              smallest l >= 1 with sse <= thr (l = 63 always qualifies), the next bracket is [x_(l - 1), x_l].
 *              kt_lo_fine = the last inner.
 *              upper end, the mirror image: g = the smallest grid index with ages[g] >= kt_fine, walking up; off the
 *              grid: kt_hi_fine = ages[A - 1] and status_fine gains 4; brackets [inner, outer], the largest l <= 62 with
 *              sse <= thr (l = 0 always qualifies), next [x_l, x_(l + 1)].
 *              R = 0 gives the grid's kt_lo and kt_hi, and status_fine = status
 *   A = 1, or p == q: all candidates are equal, and the rules above give the grid age
 * One lane owns one candidate and sums over ascending j; the argmin and the "first l within thr" are shuffles and ballots
 * on (sse, l): no atomics, no float sum across lanes - the same bytes on every run, for every order of the cells and for
 * every chunk size.  Refused before any device work: what sc_fit_profiles refuses; R < 0 (SC_ERR_INVALID); R >
 * SC_PROFILE_MAX_REFINE (SC_ERR_UNSUPPORTED: a third level would decide on differences no second implementation
 * reproduces).  The buffers are those of sc_fit_profiles.  Timed as SC_K_PROFILE.
 */
#define SC_PROFILE_MAX_REFINE 2
typedef struct sc_profile_fine_fit {
    int64_t  cell;            /* the fields of sc_profile_fit, in its layout     */
    int32_t  n;
    int32_t  kt_index;
    int32_t  lo_index, hi_index;
    int32_t  status;
    double   kt, kt_lo, kt_hi;
    double   a, b, c0;
    double   sse, rmse;
    double   kt_fine, kt_lo_fine, kt_hi_fine;   /* the minimum and the interval, off the grid */
    double   a_fine, b_fine, c0_fine;           /* of kt_fine                                 */
    double   sse_fine, rmse_fine;               /* sse_fine <= sse                            */
    double   height_fine;                       /* 2 a_fine                                   */
    int32_t  status_fine;     /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) */
} sc_profile_fine_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_profiles_refine(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                           const double* ages, int A, int h, int w, int R, double de, double delta, int min_samples,
                           sc_profile_fine_fit* out_rows, double* out_sse);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_profiles_refine_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                               const double* ca, long long K, const double* ages, int A, int h, int w, int R, double de,
                               double delta, int min_samples, sc_profile_fine_fit* out_rows, double* out_sse);

/*
 * Continuous ages of the joint fit (docs/segments.md, "Continuous ages"; scarplet_amd/csrc/sc_segment_refine.hip): the fit
 * of sc_fit_segments, and after it the refinement of sc_fit_profiles_refine on the segment's POOLED criterion.
 *   shared     the samples, the usable-profile rule, n, n_profiles, dof, the grid fit and its curve are sc_fit_segments':
 *              every field of sc_segment_fit and of sc_segment_cell, and out_sse, are its bytes (its launches)
 *   column     of a candidate age x, and the candidates of a bracket [p, q]: those of sc_fit_profiles_refine
 *   joint fit  at x: per usable profile c, ebar_c, gamma_c, See_c, Sep_c by passes 0 to 2 with the candidate's column;
 *              a(x) = (sum_c Sep_c) / (sum_c See_c); b_c, c0_c and the explicit residuals sse_c with that a; sse(x) =
 *              sum_c sse_c.  The sums over c are the blocked sums of sc_fit_segments - no addition for one profile.  A
 *              NaN sse counts as +inf
 *   minimum, interval, status_fine: the rules of sc_fit_profiles_refine, on the segment's grid curve and with the
 *              segment's dof for n - 3.  rmse_fine = sqrt(sse_fine / dof)
 *   status 1   every *_fine float is NaN, status_fine = 1
 *   cells      b_fine, c0_fine, sse_fine: each usable profile's slope, intercept and share of the sse at kt_fine; NaN where
 *              b is NaN; the grid's b, c0, sse where the grid age was kept
 * R = 0 returns the grid's values in every fine field.  A segment of one usable profile returns the kt_fine, kt_lo_fine,
 * kt_hi_fine, a_fine, sse_fine, rmse_fine and status_fine - and b_fine, c0_fine - of sc_fit_profiles_refine for that cell,
 * bit for bit.  The refinement runs in 2 R rounds per chunk (R for the minimum, R for both ends side by side); a round's
 * candidate terms are parked beside the per-age terms, 8 ((2h + 1) + 4 (A + 128)) bytes per cell with R > 0, counted
 * against SC_SEGMENT_MAX_PARK; chunks are whole segments and a single segment that needs more is SC_ERR_UNSUPPORTED.  No
 * copy to the host between the rounds, no atomics, every sum in a fixed order: the same bytes on every run and for every
 * chunk size.  Refused before any device work: what sc_fit_segments refuses; R < 0 (SC_ERR_INVALID); R >
 * SC_PROFILE_MAX_REFINE (SC_ERR_UNSUPPORTED).  The buffers are those of sc_fit_segments and one of the call's own.  Timed
 * as SC_K_PROFILE.
 */
#define SC_SEGMENT_REFINE_COLUMNS 128   /* candidate columns parked per cell with R > 0: both ends of the interval in a round */
typedef struct sc_segment_fine_fit {
    int32_t  label;           /* the fields of sc_segment_fit, in its layout     */
    int32_t  n_cells;
    int32_t  n_profiles;
    int32_t  n;
    int32_t  dof;
    int32_t  kt_index;
    int32_t  lo_index, hi_index;
    int32_t  status;
    double   kt, kt_lo, kt_hi;
    double   a;
    double   sse, rmse;
    double   kt_fine, kt_lo_fine, kt_hi_fine;   /* the minimum and the interval, off the grid */
    double   a_fine;                            /* of kt_fine: the offset is 2 a_fine         */
    double   sse_fine, rmse_fine;               /* sse_fine <= sse                            */
    int32_t  status_fine;     /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) */
} sc_segment_fine_fit;
typedef struct sc_segment_fine_cell {
    int64_t  cell;            /* the fields of sc_segment_cell, in its layout    */
    int32_t  used;
    int32_t  n;
    double   b, c0, sse;
    double   b_fine, c0_fine, sse_fine;         /* at kt_fine; NaN where b is NaN */
} sc_segment_fine_cell;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_segments_refine(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                           const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                           int h, int w, int R, double de, double delta, int min_samples, int min_profiles,
                           sc_segment_fine_fit* out_rows, sc_segment_fine_cell* out_cells, double* out_sse);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_segments_refine_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                               const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                               long long S, const double* ages, int A, int h, int w, int R, double de, double delta,
                               int min_samples, int min_profiles, sc_segment_fine_fit* out_rows,
                               sc_segment_fine_cell* out_cells, double* out_sse);

/*
 * The initial slope of the joint fit (docs/segments.md, "The initial slope"; scarplet_amd/csrc/sc_segment_ramp.hip): the
 * fit of sc_fit_segments with the scarp of sc_fit_profiles_ramp,
 *   z_c(s) = c0_c + b_c s + a g(s; kt, L),   L = m de,   m = 0..M a whole number of cells.
 * The amplitude, the age AND the half-width are the segment's; every profile keeps its own intercept and far-field slope.
 *   samples  the sampling and the usable-profile rule of sc_fit_segments; the erf table of sc_fit_profiles (by its launch)
 *            serves m = 0, Ftab of sc_fit_profiles_ramp over x = -(h + M)..(h + M) serves m >= 1: e_cij = (Ftab[j + m][i] -
 *            Ftab[j - m][i]) / ((double)(2 m) de), formed in that order
 *   per profile c and pair (i, m): ebar, gamma, See_cim, Sep_cim as sc_fit_profiles (m = 0) and sc_fit_profiles_ramp (m >= 1)
 *            form them, summed over ascending j in one lane; n, sbar, pbar, Sss, beta and p2 depend on neither i nor m and
 *            are formed once
 *   segment  a_im = (sum_c Sep_cim) / (sum_c See_cim); b_cim = beta_c - a_im gamma_cim; c0_cim = (pbar_c - a_im ebar_cim) -
 *            b_cim sbar_c; sse_cim = sum_j of the squared explicit residuals; sse_im = sum_c sse_cim; bbar_im = (sum_c b_cim) /
 *            (double)n_profiles.  Every sum over c is the blocked sum of sc_fit_segments (64 consecutive usable profiles
 *            in input order in sequence, then the block sums in sequence; one profile: no addition).  A pair whose sum
 *            See is not > 0, or whose sse is NaN, never wins
 *   per age  SC_RAMP_FREE: m_i = argmin_m sse_im over m = 0..M, the first smallest winning.  SC_RAMP_SLOPE: over m = 1..M
 *            the key | |bbar_im + a_im / ((double)m de)| - slope |, the first smallest winning: the constraint of
 *            sc_fit_profiles_ramp with the segment's mean far-field slope for one profile's.  sse*_i = sse_{i, m_i}
 *   choice   kt_index = argmin_i sse*_i, ties to the smaller index; dof = n - 2 n_profiles - 1 - (M > 0) with SC_RAMP_FREE
 *            (the width is the segment's: one degree of freedom), n - 2 n_profiles - 1 with SC_RAMP_SLOPE; fitted when
 *            n_profiles >= min_profiles and dof >= 1.  rmse, thr and the walks run along sse*, as in sc_fit_segments.
 *            Status 1, 2 and 4 as sc_fit_segments; 8: width_index == M with M > 0
 * M = 0 returns the bytes of sc_fit_segments in every shared field of rows, cell table and curve; a segment of one usable
 * profile returns the kt_index, lo_index, hi_index, status, a, sse, rmse, width_index and initial_slope of
 * sc_fit_profiles_ramp for that cell, and its b and c0 in the cell table, bit for bit.  out_rows: S rows; out_cells: K rows
 * (b, c0 and sse of each profile at the best pair) or NULL; out_sse: S x A float64 (sse*) or NULL; out_width: S x A int8
 * (m_i, 0 in the rows of status 1) or NULL.  Per cell the call parks the profile and four float64 terms per pair: 8 ((2h +
 * 1) + 4 A (M + 1)) bytes, counted against SC_SEGMENT_MAX_PARK; chunks are whole segments and a single segment that needs
 * more is SC_ERR_UNSUPPORTED (367 thousand cells at h = 100, 35 ages and M = 8).  Refused before any device work: what
 * sc_fit_segments refuses, and what sc_fit_profiles_ramp refuses of M, mode and slope (SC_ERR_INVALID; M >
 * SC_PROFILE_MAX_WIDTH: SC_ERR_UNSUPPORTED).  No atomics, no float sum across lanes: the same bytes on every run.  The
 * buffers are those of sc_fit_segments and two of the call's own.  Timed as SC_K_PROFILE.
 */
typedef struct sc_segment_ramp_fit {
    int32_t  label;
    int32_t  n_cells;         /* cells of the segment                            */
    int32_t  n_profiles;      /* usable profiles among them                      */
    int32_t  n;               /* pooled valid points of the usable profiles      */
    int32_t  dof;             /* n - 2 n_profiles - 1 - (M > 0 with the width free) */
    int32_t  kt_index;        /* best age (-1: not fitted)                       */
    int32_t  lo_index, hi_index;
    int32_t  status;          /* 0, or 1 (not fitted), or 2 (open below) + 4 (open above) + 8 (width at its limit) */
    double   kt, kt_lo, kt_hi;
    double   a;               /* the segment's amplitude: its offset is 2 a      */
    double   sse, rmse;       /* rmse = sqrt(sse / dof)                          */
    int32_t  width_index;     /* m of the best age, in cells (0 where not fitted) */
    double   width;           /* m de, the half-width L (NaN where not fitted)   */
    double   initial_slope;   /* bbar + a / (m de), signed; copysign(inf, a) at m = 0; NaN where not fitted */
} sc_segment_ramp_fit;
/* on the DEM of the last sc_set_dem (the whole grid, float64, as the context holds it) */
int sc_fit_segments_ramp(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                         const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                         int h, int w, int M, int mode, double slope, double de, double delta, int min_samples,
                         int min_profiles, sc_segment_ramp_fit* out_rows, sc_segment_cell* out_cells, double* out_sse,
                         int8_t* out_width);
/* the same on z, ny x nx float64 on the host, uploaded into a buffer of the call's own */
int sc_fit_segments_ramp_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                             const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                             long long S, const double* ages, int A, int h, int w, int M, int mode, double slope,
                             double de, double delta, int min_samples, int min_profiles, sc_segment_ramp_fit* out_rows,
                             sc_segment_cell* out_cells, double* out_sse, int8_t* out_width);

/*
 * The search's float64 SNR surface at chosen cells (docs/surface.md, scarplet_amd/csrc/sc_surface.hip).
 *   t        n_par * n_ang descriptors, orientation-major (template of parameter ia and orientation ib at ib * n_par + ia:
 *            what Matcher.describe makes).  They become the context's template table as in sc_settle_pairs: nothing is
 *            matched, the running-best record, its patches and the near-tie lists stay as they are; the float64 scorers'
 *            "last search" (sc_score_cells_f64) afterwards is this table.
 *   cells    K (row, col) pairs, global; repeats allowed; rows and cubes come back in this order
 *   keep     1 - drop, in (0, 1]: the intervals and n_within hold the templates scoring >= snr * keep (one multiply)
 *   rows     K rows (host)
 *   snr, amp K * n_ang * n_par float64 each (host), the cell's scores in the order of t; either may be NULL
 * S[k][t] and Amp[k][t] are match_template() (core.py:297-377) in float64 as the real-space closed form (sc_score_cells_f64's
 * arithmetic; n and sum(W**2) summed in a fixed order).  A NaN score counts as -inf.  The first maximum of S[k] gives
 * par_index, ang_index, snr, amp; par_lo .. par_hi is the run of parameters around par_index whose best score over the
 * orientations stays >= snr * keep, ang_lo .. ang_hi likewise (it does not wrap); n_within counts the templates >= snr * keep.
 * status: 1 no score > 0 (the cell lies outside every template's window limits: indices -1, n_within 0, snr and amp NaN);
 * else the sum of 2 (par_lo == 0), 4 (par_hi == n_par - 1), 8 (ang_lo == 0), 16 (ang_hi == n_ang - 1).
 * SC_ERR_INVALID / SC_ERR_UNSUPPORTED: an empty grid, more than 65535 templates, more than 2^31 - 1 cells, a cell outside
 * the DEM, keep outside (0, 1], a DEM with NaN cells, a context that holds a block of a larger DEM, a table that is not
 * orientation-major.  The cells go through in chunks whose two score cubes take at most 256 MiB of device memory.  Timed
 * under SC_K_SETTLE.  The same bytes on every run.
 */
typedef struct sc_surface_row {
    int32_t par_index, ang_index, par_lo, par_hi, ang_lo, ang_hi, n_within, status;
    double snr, amp;
} sc_surface_row;
int sc_snr_surface(sc_ctx* ctx, const sc_template* t, int n_par, int n_ang, const int32_t* cells /* K (row, col) pairs */,
                   long long K, double keep, sc_surface_row* rows, double* snr /* K * n_ang * n_par, or NULL */,
                   double* amp /* or NULL */);

/* Float32 resolution of the FFT path on THIS surface, measured by the searches since the last
 * sc_reset_best: *wins = cells a template of the FFT path won, *near_floor = those whose residual
 * T3 - T1 (what the SNR divides by, core.py:362-366) lies within 256 x the transforms' float32
 * resolution floor (sc_internal.h sc_epi_floor) - their SNR is off by more than the stated
 * tolerance and their argmax is rounding noise.  ~0 on DEMs with a noise floor of their own
 * (lidar, the benchmark DEM), tens of per cent on synthetic surfaces stored without one; the
 * real-space path has no such limit.  scarplet_amd.match(method="auto") reads it to fall back. */
int sc_get_resolution_stats(sc_ctx* ctx, long long* wins, long long* near_floor);

/* Near-ties of the FFT searches since the last sc_reset_best, one byte per core cell, (cy1-cy0) x (cx1-cx0):
 * 1 where some template scored within the relative window of option "near_window" of the cell's running best
 * (either side of it; equal scores included since ABI 7).  A float32 FFT convolution carries an SNR error of up to half the
 * path's tie window (scarplet_amd: oracle-measured): between two templates closer than
 * that, which one the record holds is rounding noise.  The real-space path flags the same way with the option on - and
 * equal scores as well (its per-cell float32 sums can give two templates a rounding apart the same bits).
 * scarplet_amd.match(..., exact=True) settles the flagged cells in float64 (sc_get_near_events + sc_score_pairs_f64;
 * or, where the event list overflowed, a real-space search of them + sc_score_cells_f64): the argmax of every cell
 * is then the float64 reference's.  All zero when the option is 0 (the default: flags and events cost the row pass 13 %). */
int sc_get_near_ties(sc_ctx* ctx, uint8_t* out);

/* match_template() at single cells in FLOAT64 - core.py:297-377 as the real-space closed form, the template
 * evaluated with the reference's float64 expressions, the curvature from the float64 elevations (dem.py:88-104) -
 * for the m cells given (global row, column pairs) and EVERY template of the last sc_match in this context, in
 * the order they were handed over: amp, snr = m x n doubles each, masks applied (core.py:369-375).  The last step
 * of scarplet_amd.match(..., exact=True): the cells where two templates lie inside the float32 paths' own rounding
 * are settled the way the reference settles them.  Host-uploaded windows (SC_KIND_WINDOW) are scored from their slots'
 * float64 copies, with the curvature of the descriptor's (cc, sc2, ss) - the search orientation's, not the plugin's alpha -
 * and their per-cell masks (ABI 10; SC_ERR_INVALID when a slot no longer holds its template's window); the
 * context must hold the cells' neighbourhoods (a whole DEM does).  n_templates: what the caller sized amp / snr for -
 * SC_ERR_INVALID unless it is the number of templates of that last sc_match (ABI 8). */
int sc_score_cells_f64(sc_ctx* ctx, const int32_t* cells, int m, int n_templates, double* amp, double* snr);

/* The near-ties of the searches since the last sc_reset_best as EVENTS (round 5; ABI 8: FOUR 32-bit words each, both paths) -
 * the cell (index into the core planes, row-major), the id of the template that was being scored, the id of the template
 * that held the cell's record at that moment (SC_ID_NONE: none yet), the float32 bits of the LARGER of their two scores -
 * one per (cell, template) whose score came within option "near_window" of the record, either side.  The true float64
 * argmax of a flagged cell is the record's final holder or one of the templates its events name (two templates further
 * apart than the window differ by more than twice the path's error: the lower one cannot be the argmax), and only events
 * whose larger score lies within the window of the FINAL record can name it: sc_settle_exact scores exactly those (cell,
 * template) pairs in float64.  *n_events = events recorded; the device list holds two per core cell (a million at least).
 * A count above `capacity` copies nothing and returns SC_OK (the caller asks again with room); a list that OVERFLOWED on
 * the device answers SC_ERR_UNSUPPORTED (ABI 8: said by the call, not left to the caller's arithmetic) - the caller takes
 * the route without events (sc_get_near_ties + sc_score_cells_f64). */
int sc_get_near_events(sc_ctx* ctx, uint32_t* events, long long capacity, long long* n_events);

/* sc_score_cells_f64 for (cell, template) PAIRS: pair k = global cell (cells[2k], cells[2k+1]) against template
 * templates[k] of the last sc_match in this context (its index in hand-over order); amp, snr = m doubles each. */
int sc_score_pairs_f64(sc_ctx* ctx, const int32_t* cells, const int32_t* templates, int m, double* amp, double* snr);

/*
 * exact=True on the device (round 6, ABI 8): the reference's fold is an argmax over float64 SNR maps (compare(),
 * core.py:230-240); this call makes the record's (age, orientation) of every near-tie cell that argmax.  After an sc_match
 * with option "near_window" on (either path lists its near-ties since ABI 8): the flagged cells become slots in cell
 * order, every cell's candidates - the record's final holder and the templates named by its events (those whose larger score
 * the final record has left behind by more than the window are dropped: neither template can be the argmax) - become a list, exactly
 * those (cell, template) pairs are scored in float64 (sc_score_pairs_f64's arithmetic, one workgroup per pair; a template
 * named twice in a list, or a list of one template, is not scored), and every cell takes the largest float64 SNR, ties to
 * the earlier template of the hand-over order.  The winner's id goes into the record (amp and snr rounded to float32: what
 * sc_get_best, sc_gather_result and sc_fold_ranks then see) and its float64 (amp, snr) are kept as patches that
 * sc_get_result lays over the converted planes - until the next sc_match or sc_reset_best.  No host pass over the planes:
 * three 8-byte read-backs size the buffers.
 *   n_twin    the last n_twin templates of the search are one CLASS with its first n_twin (the orientation grid's two ends
 *             are one template for the symmetric built-ins: +pi/2 against -pi/2, core.py:173-175 - their float64 SNRs
 *             differ by rounding noise, one maximum by the parity policy); 0: none.  One member of a class is scored per
 *             cell - the record's holder where its class is named - as itself (its amplitude carries its own sign)
 *   max_work  > 0: nothing is scored when pairs x the largest support box exceeds it (SC_ERR_UNSUPPORTED)
 *   stats     8 values: flagged cells, pairs listed, pairs scored, cells scored, cells whose template changed, events,
 *             the audit, taps the scores weighed.  The audit (stats[6], ABI 10): over the cells whose record holder was
 *             scored in float64, the largest |snr32 - snr64| / snr64 of its float32 record against that score, as an
 *             integer in units of 1e-9, rounded up (at most 1e18; 0 when no holder was scored).  A lower bound on the
 *             search's float32 SNR error - only holders of near-tie cells are seen - measured at no extra cost.
 * Templates with host-uploaded windows (SC_KIND_WINDOW) are settled like the built-ins since ABI 10 (sc_score_cells_f64).
 * SC_ERR_UNSUPPORTED when the event list overflowed (the caller takes a longer route: sc_get_near_ties +
 * sc_score_cells_f64).
 */
int sc_settle_exact(sc_ctx* ctx, int n_twin, double max_work, long long* stats);

/*
 * exact=True for an ORIENTATION-SHARDED search (scarplet_amd.dist.OrientationMatcher; the reference's pool over orientations,
 * core.py:180-183, whose compare() folds float64 maps).  Every rank searched its share of the templates with "near_window"
 * on and sc_fold_ranks made every record the fold of all - a near-tie between templates of two ranks is in no rank's list.
 * But a template that can be the float64 argmax scores, in float32, within the window of the FOLDED record, and the rank that
 * matched it knows: it is named by one of that rank's events whose larger score lies within the window of the folded record,
 * or it held the rank's own record.  The sequence, the same on every rank:
 *   sc_match (near_window on) -> sc_snapshot_best -> sc_fold_ranks (or sc_get_best / host fold / sc_set_best)
 *   -> sc_rank_candidates -> sc_exchange_candidates (RCCL; or the launcher's transport concatenates the ranks' pair
 *   lists, in rank order) -> sc_settle_pairs with the descriptors of the WHOLE search.
 * Every rank scores the same pairs with the same float64 arithmetic: the records agree bit for bit without a further
 * collective, and equal what sc_settle_exact leaves in a single context that searched all the templates wherever the
 * float64 argmax is concerned (tests/test_gpu_exact.py).
 */
/* the record's (snr, id) planes as they stand, kept on the device (call it BEFORE the fold) */
int sc_snapshot_best(sc_ctx* ctx);
/* upload a record - core cells, row-major: amplitude, SNR, template id - as this context's running best (the host
 * backend's fold, or a record saved earlier); patches of an earlier settle are dropped */
int sc_set_best(sc_ctx* ctx, const float* amp, const float* snr, const uint32_t* id);
/* this rank's candidates against the folded record: (core cell index, template id) pairs, 2 x uint32 each.  *n_pairs is
 * the number found; they are copied to `pairs` when capacity (in pairs) holds them - call with capacity 0 to size the
 * buffer (the list is kept on the device in between).  SC_ERR_UNSUPPORTED when the event list overflowed. */
int sc_rank_candidates(sc_ctx* ctx, uint32_t* pairs, long long capacity, long long* n_pairs);
/* settle the union of all ranks' candidates: t[0..n) = the descriptors of the WHOLE search in fold order (they become the
 * context's template table; nothing is matched), pairs as sc_rank_candidates wrote them (ids = sc_template.id);
 * n_twin, max_work, stats as sc_settle_exact.  Built-in template classes only: a template with a host-uploaded window
 * (SC_KIND_WINDOW) answers SC_ERR_UNSUPPORTED - the other ranks' window slots do not exist in this context. */
int sc_settle_pairs(sc_ctx* ctx, const sc_template* t, int n, const uint32_t* pairs, long long n_pairs, int n_twin,
                    double max_work, long long* stats);
/* the exchange on the devices: after sc_rank_candidates (capacity 0 will do: the list stays on the device) every rank's
 * list becomes one list on every device - two ncclAllGather over RCCL/xGMI: the counts, then slots of the largest count in
 * rank order, short lists padded with cells no DEM has.  *n_union = pairs in it, padding included; sc_settle_pairs with
 * pairs == NULL and n_pairs == *n_union settles it.  Collective: all ranks of the communicator call it - a rank whose
 * sc_rank_candidates failed (an overflowed event list) too: it takes part in the counts' all-gather with a marker and every rank
 * returns SC_ERR_UNSUPPORTED, none is left waiting.  No communicator: the union is the rank's own list. */
int sc_exchange_candidates(sc_ctx* ctx, long long* n_union);

/* Per-template scalars of the last sc_match / sc_match_template call:
 * n = count(W != 0) + eps (core.py:350) and sum(W**2) (core.py:356). */
int sc_get_template_sums(sc_ctx* ctx, int n, double* n_out, double* ts_out);

/* ---- measurement ------------------------------------------------------- */
#define SC_K_CURV        0
#define SC_K_WINDOWS     1
#define SC_K_DIRECT      2
#define SC_K_FWD_ROWS    3
#define SC_K_FWD_COLS    4
#define SC_K_INV_COLS    5
#define SC_K_INV_ROWS    6
#define SC_K_SETTLE      7      /* sc_settle_exact, sc_snr_surface: all their kernels as one bracket */
#define SC_K_NOISE       8      /* sc_curvature_noise: all its kernels as one bracket */
#define SC_K_TRACE       9      /* sc_trace_planes / sc_trace_result: their kernels before and after the read-back of K */
#define SC_K_PROFILE     10     /* sc_fit_profiles* (_robust too), sc_fit_segments*, sc_bootstrap_segments*, sc_fit_strike*, sc_strike_bootstrap*: the table and every kernel of every chunk; sc_lateral_offsets*: the kernel of every chunk */
#define SC_K_COUNT       11
/* HIP-event timing of every launch on the context's stream. */
int sc_profile(sc_ctx* ctx, int enable);
int sc_profile_get(sc_ctx* ctx, int kernel, long long* launches,
                   double* total_ms);
const char* sc_kernel_name(int kernel);
/* device memory currently held by the context, bytes */
size_t sc_device_bytes(sc_ctx* ctx);

/* ---- multi-GPU: RCCL halo exchange (one process per GPU) ---------------- */
#define SC_COMM_ID_BYTES 128
int sc_comm_unique_id(void* id_out /* SC_COMM_ID_BYTES */);
int sc_comm_init(sc_ctx* ctx, const void* id, int rank, int nranks);
/*
 * One rectangle of the halo exchange, in cells of this rank's halo-extended
 * block.  The host (scarplet_amd/dist.py) derives the list for every rank from
 * the tile grid; all ranks walk the same global order, so sends and receives
 * between a pair of ranks match up.
 */
#define SC_XFER_RECV  0   /* receive h x w cells from `peer` into (dy0, dx0)       */
#define SC_XFER_SEND  1   /* send the h x w cells at (sy0, sx0) to `peer`          */
#define SC_XFER_LOCAL 2   /* copy (sy0, sx0) -> (dy0, dx0) inside the block
                             (periodic image of the rank's own core)              */
typedef struct sc_xfer {
    int32_t peer, kind;
    int32_t sy0, sx0, dy0, dx0, h, w;
} sc_xfer;

/*
 * Assemble this rank's halo-extended elevation block on the device.
 *   core      this rank's own cells, core_h x core_w float64 (host)
 *   h*_lo/hi  halo cells around the core; the block is
 *             (hy_lo + core_h + hy_hi) x (hx_lo + core_w + hx_hi)
 *   x, n      the rank's transfers; sends/receives run as one grouped
 *             ncclSend/ncclRecv over xGMI, halo rectangles are packed into a
 *             contiguous staging buffer first
 * On return *z_dev is the float64 device block (owned by the context), ready
 * for sc_set_dem_device.
 */
int sc_halo_exchange(sc_ctx* ctx, const double* core, int core_h, int core_w,
                     int hy_lo, int hy_hi, int hx_lo, int hx_hi,
                     const sc_xfer* x, int n, void** z_dev);
/*
 * Final gather of a tiled search (results are disjoint rectangles): every rank
 * sends the float32 record of its core - amplitude, SNR, template id: 12 bytes
 * per cell, three grouped ncclSend - to `root` over RCCL; root receives all ranks
 * at once, converts each record like sc_get_result (the id tables are the same on
 * every rank) and places the four float64 planes in out = 4 x ny x nx doubles (host).
 *   cores   nranks x 4 ints: [cy0, cy1, cx0, cx1) of every rank, same on all ranks
 *   out     root only (ignored elsewhere)
 * Collective: all ranks of the communicator call it.  Without a communicator
 * (single context) it is sc_get_result into the core's place.
 */
int sc_gather_result(sc_ctx* ctx, int root, const int32_t* cores, int ny, int nx,
                     const double* param_of_id, const double* angle_of_id, int n_ids,
                     double* out);
/*
 * Fold of an orientation-sharded search: every rank holds the WHOLE DEM and searched its share
 * of the templates, numbered globally in fold order (the reference's own parallelism: a pool
 * over orientations, core.py:180-183, folded by compare(), core.py:198-243).  On return every
 * rank's running-best record is the fold of all ranks' records: per cell the greatest SNR
 * wins, equal SNRs go to the smaller id (the earlier template of the fold order - what a
 * single context folding all templates keeps), a NaN SNR beats every number (sc_match's
 * sticky NaN).  Two all-reduces over RCCL/xGMI: ncclMax on the 64-bit key
 * (SNR bits << 32 | ~id), ncclSum on the amplitude (zeroed on the ranks that lost the cell).
 * Collective: all ranks of the communicator call it, with the same core.  No communicator:
 * nothing to do.
 */
int sc_fold_ranks(sc_ctx* ctx);
/* What RCCL reports for this context's communicator: ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice, and the PCI bus id of the context's device (bus_id: at least 16 bytes, may
 * be NULL).  Without a communicator *nranks = 0, *rank = -1. */
int sc_comm_info(sc_ctx* ctx, int* nranks, int* rank, int* device, char* bus_id, int bus_id_len);
int sc_comm_destroy(sc_ctx* ctx);

/* (The TIFF LZW decoder of the GeoTIFF reader moved to libscarplet_host.so in round 3:
 * include/scarplet_host.h - reading a DEM must not need the HIP and RCCL runtimes.) */

#ifdef __cplusplus
}
#endif
#endif /* SCARPLET_HIP_H */
