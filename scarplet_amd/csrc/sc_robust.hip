// sc_fit_profiles_robust* : the fit of sc_fit_profiles with a weight on every point and a robust loss (docs/profiles.md,
// "Weights and robust fits").
//
// The same wave per cell as k_pf_fit, PF_WAVES cells per workgroup, the same erf table (sc_pf_table) in LDS up to
// PF_TAB_LDS bytes - where the workgroup's LDS still holds it beside the profiles - and in global memory beyond.
//   rb_cut       lanes over the points j: the profile p_j and, with a weight plane, its own samples u_j at the same
//                positions go to the wave's slice of LDS (a point whose u is not > 0 is a missing point)
//   iterate 0    lanes over the AGES: rb_moments, rb_solve (two sweeps) and rb_loss with q = u - the weighted least
//                squares fit of every age, four sweeps as k_pf_fit's; pf_choose on its sse gives ls_index
//   the scale    lane ls_index hands its (c0, b, a) to the wave; the lanes run over the POINTS and rb_select takes the
//                element of rank (n - 1) / 2 of |r_j| by integer counts: sigma = 1.4826 times it, or the caller's value
//   iterates     T times per age, lanes over the ages again: three sweeps, each of which recomputes q_j = u_j f(|r_j|)
//                from the previous iterate's (c0, b, a) in the lane's registers.  The robust weights are stored
//                nowhere: 64 ages times 2h + 1 points do not fit LDS.  An age that loses its support (fewer than
//                min_samples points with q > 0 on a side, or See not > 0) is dead: its loss is NaN
//   the loss     a fourth sweep over the last iterate's residuals: sum u rho(r), the explicit sum u r^2 and the points
//                with f < 1; pf_choose on the loss curve
// Every sum is a plain loop over ascending j in one lane, the order statistic is integer work: no atomics, no float sum
// across lanes, the same bytes on every run and for every order of the cells.  Plain C++ throughout.
// The host side is the table set-up, the kernel choice and one call of sc_pf_chunks (sc_profile.hip).  k_rb_fit keeps
// its own loop head: in pf_each_cell the Tukey fit measured 1.4 % slower (profiles/fit_frame_refactor.txt).
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

#define RB_LDS_BYTES (160 * 1024)        // the LDS of a CU
#define RB_MAD 1.4826

// a row without a fit: status 1, or 1 | 32 where every age died
__device__ __forceinline__ void rb_row_unfit(sc_profile_robust_fit* out, long long cell, int n, int status, double scale) {
    pf_row_unfit(out, cell, n);
    out->status = status;
    out->loss = __builtin_nan("");
    out->scale = scale;
    out->n_down = 0;
    out->ls_index = -1;
}

template <bool TAB_LDS, bool WT, int LOSS>
__global__ __launch_bounds__(PF_THREADS) void k_rb_fit(const double* __restrict__ z, const double* __restrict__ wt, int ny,
                                                       int nx, const long long* __restrict__ cells,
                                                       const double* __restrict__ dir, long long K,
                                                       const double* __restrict__ ages, int A, int h, int w, double de,
                                                       double delta, int min_samples, double tuning, int iterations,
                                                       double scale_in, const double* __restrict__ tab_g,
                                                       sc_profile_robust_fit* __restrict__ rows, double* __restrict__ curve) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (a wave's slice: the profile, then its weights)
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, WT ? 2 * np : np, np, A);
    double* prof = L.prof;
    double* u = WT ? L.prof + np : nullptr;
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double* col = L.tab + ia;
    const double nan = __builtin_nan("");
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        long long cell = 0;
        if (act) {
            cell = cells[kc];
            if (WT) rb_cut(z, wt, ny, nx, cell, dir, kc, h, w, lane, prof, u);
            else pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, prof, nullptr);
        }
        __syncthreads();
        if (act) {
            sc_profile_robust_fit* out = rows + kc;
            const rb_prev none = {0.0, 0.0, 0.0, 0.0};
            const rb_mom mo = rb_moments<0, WT>(prof, u, np, h, de, col, A, none);
            const int dof = mo.n - 3;
            bool done = false;
            if (mo.n_neg < min_samples || mo.n_pos < min_samples) {
                if (lane == 0) rb_row_unfit(out, cell, mo.n, 1, nan);
                pf_unfit_planes(kc, lane, A, curve, nullptr);
                done = true;
            }
            rb_prev v = none;
            double sse = nan, loss = nan, sigma = nan;
            int n_down = 0, ls = -1, flag = 0;
            if (!done) {
                // iterate 0: weighted least squares of every age
                rb_solve<0, WT>(prof, u, np, h, de, col, A, none, mo, v);
                rb_loss<0, WT>(prof, u, np, h, de, col, A, v, sse, loss, n_down);
                if (__ballot(lane < A && sse == sse) == 0ull) {
                    if (lane == 0) rb_row_unfit(out, cell, mo.n, 1 | 32, nan);
                    pf_unfit_planes(kc, lane, A, curve, nullptr);
                    done = true;
                }
            }
            if (!done && LOSS) {
                ls = pf_choose(sse, lane, A, delta, dof).best;
                sigma = scale_in;
                if (!(scale_in > 0.0)) {
                    rb_prev at;
                    at.c0 = __shfl(v.c0, ls, 64);
                    at.b = __shfl(v.b, ls, 64);
                    at.a = __shfl(v.a, ls, 64);
                    at.c = 0.0;
                    sigma = RB_MAD * rb_select(prof, np, h, de, L.tab + ls, A, at, lane, (mo.n - 1) / 2);
                }
                if (!(sigma > 0.0)) {
                    flag = 16;                           // no scale: the row of iterate 0
                } else {
                    v.c = tuning * sigma;
                    bool dead = false;
                    for (int t = 0; t < iterations; ++t) {
                        const rb_mom mq = rb_moments<LOSS, WT>(prof, u, np, h, de, col, A, v);
                        dead = dead || mq.n_neg < min_samples || mq.n_pos < min_samples;
                        rb_prev next;
                        dead = !rb_solve<LOSS, WT>(prof, u, np, h, de, col, A, v, mq, next) || dead;
                        v = next;
                    }
                    rb_loss<LOSS, WT>(prof, u, np, h, de, col, A, v, sse, loss, n_down);
                    if (dead) loss = nan;
                    if (__ballot(lane < A && loss == loss) == 0ull) {
                        if (lane == 0) rb_row_unfit(out, cell, mo.n, 1 | 32, sigma);
                        pf_unfit_planes(kc, lane, A, curve, nullptr);
                        done = true;
                    }
                }
            }
            if (!done) {
                if (curve && lane < A) curve[kc * A + lane] = loss;
                const pf_pick k = pf_choose(loss, lane, A, delta, dof);
                if (lane == k.best) {
                    pf_row_fit(out, cell, mo.n, k, pf_open(k, A) + flag, ages, v.a, v.b, v.c0, sse, dof);
                    out->rmse = sqrt(loss / (double)dof);
                    out->loss = loss;
                    out->scale = sigma;
                    out->n_down = flag ? 0 : n_down;
                    out->ls_index = LOSS ? ls : k.best;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
typedef void (*rb_kernel)(const double*, const double*, int, int, const long long*, const double*, long long, const double*, int,
                          int, int, double, double, int, double, int, double, const double*, sc_profile_robust_fit*, double*);

template <bool TAB_LDS, bool WT>
static rb_kernel rb_pick_loss(int loss) {
    return loss == SC_ROBUST_HUBER ? k_rb_fit<TAB_LDS, WT, 1> : loss == SC_ROBUST_TUKEY ? k_rb_fit<TAB_LDS, WT, 2> : k_rb_fit<TAB_LDS, WT, 0>;
}

static rb_kernel rb_pick(bool tab_lds, bool wt, int loss) {
    if (tab_lds) return wt ? rb_pick_loss<true, true>(loss) : rb_pick_loss<true, false>(loss);
    return wt ? rb_pick_loss<false, true>(loss) : rb_pick_loss<false, false>(loss);
}

int sc_rb_check(sc_ctx* ctx, const char* who, int loss, double tuning, int iterations, double scale) {
    if (loss != SC_ROBUST_NONE && loss != SC_ROBUST_HUBER && loss != SC_ROBUST_TUKEY)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: the loss must be SC_ROBUST_NONE, _HUBER or _TUKEY", who);
    if (loss == SC_ROBUST_NONE) return SC_OK;
    if (!(isfinite(tuning) && tuning > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the tuning constant must be finite and > 0", who);
    if (iterations < 1) return sc_fail(ctx, SC_ERR_INVALID, "%s: needs at least one iteration", who);
    if (iterations > SC_ROBUST_MAX_ITER)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d iterations, more than %d", who, iterations, SC_ROBUST_MAX_ITER);
    if (!(isfinite(scale) && scale >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the scale must be finite and >= 0 (0: estimated)", who);
    return SC_OK;
}

static int rb_run(sc_ctx* ctx, const double* z, const double* wt, int ny, int nx, const long long* cells, const double* sa,
                  const double* ca, long long K, const double* ages, int A, int h, int w, double de, double delta,
                  int min_samples, int loss, double tuning, int iterations, double scale, sc_profile_robust_fit* out_rows,
                  double* out_loss) {
    const int np = 2 * h + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)np * A;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;

    // (the profiles and their weights come first: the table goes to LDS only where the CU still holds it beside them)
    const int np2 = wt ? 2 * np : np;
    const bool tab_lds = tab_bytes <= PF_TAB_LDS && pf_lds_bytes(np2, np, A, false, true) <= RB_LDS_BYTES;
    const size_t lds = pf_lds_bytes(np2, np, A, false, tab_lds);
    const rb_kernel kern = rb_pick(tab_lds, wt != nullptr, loss);
    if ((rc = sc_lds_attr(ctx, (const void*)kern, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sc_pf_table(ctx, d_ages, A, h, de, d_tab))) return rc;

    const pf_plane curve = {out_loss, &ctx->pf_sse, sizeof(double) * (size_t)A}, none = {nullptr, nullptr, 0};
    return sc_pf_chunks(ctx, cells, sa, ca, K, PF_CHUNK, sizeof(sc_profile_robust_fit), out_rows, curve, none,
                        [&](const pf_chunk& d, long long m) {
        kern<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, wt, ny, nx, d.cells, d.dir, m, d_ages, A, h, w, de, delta, min_samples,
                                                          tuning, iterations, scale, d_tab, (sc_profile_robust_fit*)d.rows,
                                                          (double*)d.plane[0]);
    });
}

// The two calls after their null checks: the argument checks, then the fit on z - ny x nx on the host, uploaded - or on
// the context's DEM (z null); the weight plane, where there is one, is uploaded either way.
static int rb_call(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                   long long K, const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                   const double* weights, int loss, double tuning, int iterations, double scale,
                   sc_profile_robust_fit* out_rows, double* out_loss) {
    const char* who = "sc_fit_profiles_robust";
    int rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if ((rc = sc_rb_check(ctx, who, loss, tuning, iterations, scale))) return rc;
    if (K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    const double* w_dev = nullptr;
    if (weights) {
        if ((rc = sc_pf_upload(ctx, ctx->pf_wt, weights, ny, nx))) return rc;
        w_dev = (const double*)ctx->pf_wt.p;
    }
    return rb_run(ctx, z_dev, w_dev, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, loss, tuning, iterations,
                  scale, out_rows, out_loss);
}

extern "C" int sc_fit_profiles_robust(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                      const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                                      const double* weights, int loss, double tuning, int iterations, double scale,
                                      sc_profile_robust_fit* out_rows, double* out_loss) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_profiles_robust");
    if (rc) return rc;
    return rb_call(ctx, nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, weights, loss, tuning,
                   iterations, scale, out_rows, out_loss);
}

// (reports as sc_fit_profiles_robust)
extern "C" int sc_fit_profiles_robust_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                          const double* ca, long long K, const double* ages, int A, int h, int w, double de,
                                          double delta, int min_samples, const double* weights, int loss, double tuning,
                                          int iterations, double scale, sc_profile_robust_fit* out_rows, double* out_loss) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return rb_call(ctx, z, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, weights, loss, tuning, iterations, scale,
                   out_rows, out_loss);
}
