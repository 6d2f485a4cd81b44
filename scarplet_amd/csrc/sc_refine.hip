// sc_fit_profiles_refine* : continuous scarp ages (docs/profiles.md, "Continuous ages").
//
// The fit of sc_fit_profiles, and after it up to 3 R rounds of 64 candidate ages of the cell's OWN bracket: R for the
// minimum, R for either end of the interval.  The pieces are those of sc_fit.h.
//   k_pf_refine  k_pf_fit's shape and k_pf_fit's grid fit, helper for helper: one wave per cell, pf_cut into the wave's
//                LDS, the lanes over the AGES with the table's column.  The shared fields are written from the same
//                registers by the same calls: they are k_pf_fit's bytes.
//     a round    the lanes run over the 64 CANDIDATES of a bracket [p, q].  No table can hold their columns - the
//                bracket is the cell's -, so a lane takes its column through rf_col, which evaluates
//                erf((double)j de / (2 sqrt(x))) for the lane's own age x where pf_at would read the table (sc_fit.h), and runs
//                pf_candidate on it with the pf_lin of the grid fit.  The column is RECOMPUTED in each of pf_candidate's
//                four sweeps: staged, the 64 columns of a wave are 64 (2h + 1) doubles - 103 KB at h = 100, 52 KB with
//                erf(-x) = -erf(x) on the symmetric s_j, for each of the PF_WAVES cells of a workgroup and beside the
//                56 KB table of the grid fit, on a CU of 160 KB - and registers cannot hold 2h + 1 doubles a lane.  What
//                the choice costs is measured in profiles/refine_fit.txt: the erf is 61 to 65 % of a round, and the
//                saturated tails (RF_SAT, sc_fit.h) are 17 to 19 % of the call on a scarp of age 10.
//     the picks  an argmin by shuffles on (sse, l) for the minimum, a ballot of sse <= thr for an end; the next bracket
//                is two lanes' x, read by shuffle.  Every lane holds the same p, q, thr and result: the control flow is
//                uniform over the wave.
// One code site serves the three searches (the loop over `ph`), so pf_candidate and its four erf are instantiated once.
// No atomics, no float sum across lanes, no scratch.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_refine(const double* __restrict__ z, int ny, int nx,
                                                          const long long* __restrict__ cells,
                                                          const double* __restrict__ dir, long long K,
                                                          const double* __restrict__ ages, int A, int h, int w, int R,
                                                          double de, double delta, int min_samples,
                                                          const double* __restrict__ tab_g,
                                                          sc_profile_fine_fit* __restrict__ rows,
                                                          double* __restrict__ curve) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, np, np, A);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double* col = L.tab + ia;
    pf_each_cell(
        cells, K, [&](long long kc, long long cell) { pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, L.prof, nullptr); },
        [&](long long kc, long long cell) {
            const pf_mom mo = pf_moments<true>(L.prof, np, h, de, col, A);
            sc_profile_fine_fit* out = rows + kc;
            if (mo.n_neg < min_samples || mo.n_pos < min_samples) {
                if (lane == 0) {
                    const double nan = __builtin_nan("");
                    pf_row_unfit(out, cell, mo.n);
                    out->kt_fine = nan; out->kt_lo_fine = nan; out->kt_hi_fine = nan;
                    out->a_fine = nan; out->b_fine = nan; out->c0_fine = nan;
                    out->sse_fine = nan; out->rmse_fine = nan; out->height_fine = nan;
                    out->status_fine = 1;
                }
                pf_unfit_planes(kc, lane, A, curve, nullptr);
                return;
            }
            // the grid fit: k_pf_fit's calls in k_pf_fit's order
            pf_col t;
            const pf_lin f = pf_line<true>(L.prof, np, h, de, mo, col, A, t);
            pf_rest(L.prof, np, h, de, f, pf_at(col, A), t);
            const double a = t.Sep / t.See;
            double b, c0;
            pf_slope(f.sbar, f.pbar, f.beta, t.ebar, t.gamma, a, b, c0);
            const double sse = pf_sse(L.prof, np, h, de, pf_at(col, A), a, b, c0);
            if (curve && lane < A) curve[kc * A + lane] = sse;
            const int dof = mo.n - 3;
            const pf_pick k = pf_choose(sse, lane, A, delta, dof);
            if (lane == k.best) pf_row_fit(out, cell, mo.n, k, pf_open(k, A), ages, a, b, c0, sse, dof);

            // the fine fields start as the grid's best, in every lane
            const int i = k.best;
            double fx = ages[i], fa = __shfl(a, i, 64), fb = __shfl(b, i, 64), fc = __shfl(c0, i, 64), fs = __shfl(sse, i, 64);
            double lo_x = ages[k.lo], hi_x = ages[k.hi], thr = 0.0;
            int st = pf_open(k, A);
            unsigned long long okm = 0;
            for (int ph = 0; ph < 3 && R > 0; ++ph) {    // 0: the minimum; 1: the lower end; 2: the upper end
                double p, q;
                if (ph == 0) {
                    p = ages[max(i - 1, 0)];
                    q = ages[min(i + 1, A - 1)];
                } else if (ph == 1) {
                    const unsigned long long le = __ballot(lane < A && ages[ia] <= fx);
                    const int g = le ? 63 - __clzll((long long)le) : 0;
                    int j = g;
                    while (j >= 0 && ((okm >> j) & 1ull)) --j;
                    if (j < 0) {
                        lo_x = ages[0];
                        st |= 2;
                        continue;
                    }
                    p = ages[j];
                    q = j + 1 <= g ? ages[j + 1] : fx;
                } else {
                    const unsigned long long ge = __ballot(lane < A && ages[ia] >= fx);
                    const int g = ge ? __ffsll((unsigned long long)ge) - 1 : A - 1;
                    int j = g;
                    while (j <= A - 1 && ((okm >> j) & 1ull)) ++j;
                    if (j > A - 1) {
                        hi_x = ages[A - 1];
                        st |= 4;
                        continue;
                    }
                    q = ages[j];
                    p = j - 1 >= g ? ages[j - 1] : fx;
                }
                double bx = 0.0, ba = 0.0, bb = 0.0, bc = 0.0, bs = 0.0;
                for (int r = 0; r < R; ++r) {
                    const double x = rf_x(p, q, lane);
                    pf_col tc;
                    double ca, cb, cc;
                    const double cs = pf_candidate(L.prof, np, h, de, f, rf_col{2.0 * sqrt(x), de, h}, tc, ca, cb, cc);
                    if (ph == 0) {
                        double m = cs == cs ? cs : INFINITY;
                        int mi = lane;
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) {
                            const double om = __shfl_xor(m, o, 64);
                            const int oi = __shfl_xor(mi, o, 64);
                            if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
                        }
                        if (r == R - 1) {
                            bx = __shfl(x, mi, 64); ba = __shfl(ca, mi, 64); bb = __shfl(cb, mi, 64);
                            bc = __shfl(cc, mi, 64); bs = __shfl(cs, mi, 64);
                        }
                        p = __shfl(x, max(mi - 1, 0), 64);
                        q = __shfl(x, min(mi + 1, 63), 64);
                    } else if (ph == 1) {
                        const unsigned long long in = __ballot(lane >= 1 && (cs <= thr || lane == 63));
                        const int l = __ffsll(in) - 1;
                        p = __shfl(x, l - 1, 64);
                        q = __shfl(x, l, 64);
                    } else {
                        const unsigned long long in = __ballot(lane <= 62 && (cs <= thr || lane == 0));
                        const int l = 63 - __clzll((long long)in);
                        p = __shfl(x, l, 64);
                        q = __shfl(x, l + 1, 64);
                    }
                }
                if (ph == 0) {
                    if (bs <= fs) { fx = bx; fa = ba; fb = bb; fc = bc; fs = bs; }
                    thr = fs * (1.0 + delta / (double)dof);
                    okm = __ballot(lane < A && sse <= thr);
                    st = 0;
                } else if (ph == 1) {
                    lo_x = q;
                } else {
                    hi_x = p;
                }
            }
            if (lane == 0) {
                out->kt_fine = fx; out->kt_lo_fine = lo_x; out->kt_hi_fine = hi_x;
                out->a_fine = fa; out->b_fine = fb; out->c0_fine = fc;
                out->sse_fine = fs; out->rmse_fine = sqrt(fs / (double)dof); out->height_fine = 2.0 * fa;
                out->status_fine = st;
            }
        });
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int rf_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, const double* ages, int A, int h, int w, int R, double de, double delta, int min_samples,
                  sc_profile_fine_fit* out_rows, double* out_sse) {
    const int np = 2 * h + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)np * A;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;

    const bool tab_lds = tab_bytes <= PF_TAB_LDS;
    const size_t lds = pf_lds_bytes(np, np, A, false, tab_lds);
    const auto kern = tab_lds ? k_pf_refine<true> : k_pf_refine<false>;
    if ((rc = sc_lds_attr(ctx, (const void*)kern, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sc_pf_table(ctx, d_ages, A, h, de, d_tab))) return rc;

    const pf_plane curve = {out_sse, &ctx->pf_sse, sizeof(double) * (size_t)A}, none = {nullptr, nullptr, 0};
    return sc_pf_chunks(ctx, cells, sa, ca, K, PF_CHUNK, sizeof(sc_profile_fine_fit), out_rows, curve, none,
                        [&](const pf_chunk& d, long long m) {
        kern<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, d_ages, A, h, w, R, de, delta, min_samples,
                                                          d_tab, (sc_profile_fine_fit*)d.rows, (double*)d.plane[0]);
    });
}

// The two calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null).
static int rf_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const double* ages, int A, int h, int w, int R, double de, double delta,
                   int min_samples, sc_profile_fine_fit* out_rows, double* out_sse) {
    int rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if (R < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the refinement must be >= 0 levels", who);
    if (R > SC_PROFILE_MAX_REFINE)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d levels of refinement, more than %d", who, R, SC_PROFILE_MAX_REFINE);
    if (K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    return rf_run(ctx, z_dev, ny, nx, cells, sa, ca, K, ages, A, h, w, R, de, delta, min_samples, out_rows, out_sse);
}

extern "C" int sc_fit_profiles_refine(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                      const double* ages, int A, int h, int w, int R, double de, double delta,
                                      int min_samples, sc_profile_fine_fit* out_rows, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_profiles_refine");
    if (rc) return rc;
    return rf_call(ctx, "sc_fit_profiles_refine", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, ages, A, h, w, R, de, delta,
                   min_samples, out_rows, out_sse);
}

extern "C" int sc_fit_profiles_refine_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                          const double* sa, const double* ca, long long K, const double* ages, int A, int h,
                                          int w, int R, double de, double delta, int min_samples,
                                          sc_profile_fine_fit* out_rows, double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return rf_call(ctx, "sc_fit_profiles_refine_dem", z, ny, nx, cells, sa, ca, K, ages, A, h, w, R, de, delta, min_samples,
                   out_rows, out_sse);
}
