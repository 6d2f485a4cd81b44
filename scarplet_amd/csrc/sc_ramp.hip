// sc_fit_profiles_ramp* : the initial slope of sl.fit_profiles (docs/profiles.md, "The initial slope").
//
// The scarp starts as a ramp of half-width L = m de and diffuses for kt: z(s) = c0 + b s + a g(s; kt, L) with
// g = (F(s + L) - F(s - L)) / (2 L), F(x) = x erf(x / (2 sqrt(kt))) + 2 sqrt(kt / pi) exp(-x^2 / (4 kt)).  For a whole
// number of cells m the column of every point is a difference of two rows of ONE table per age, so the search over
// m costs table look-ups and no transcendental.  The pieces are those of sc_fit.h.
//   k_rp_table   F over x = -(h + M)..(h + M) and the ages, age-minor: one erf and one exp per entry
//   k_pf_ramp    k_pf_shift's shape: one wave per cell, PF_WAVES cells per workgroup, pf_cut into the wave's LDS;
//                pf_moments and pf_line without a column, once; then the lanes run over the (m, age) pairs
//                (rp_search), whose winners per age come back in the wave's slot of LDS, and pf_choose runs on sse*.
// The table of F sits in LDS when it fits PF_TAB_LDS bytes (35 ages, h = 100, M = 8: 60.8 KB) and in global memory
// otherwise (pf_stage).  The erf table of the m = 0 pairs - the plain call's, by the plain call's launch - stays in
// global memory: a second LDS table does not fit beside F at the default shape, the m = 0 pairs are A of the
// A (M + 1) and every wave of the device reads the same 56 KB, which the L2 holds.  No atomics at all.
// The host side is the table set-up, the kernel choice and one call of sc_pf_chunks (sc_profile.hip).  k_pf_ramp keeps
// its own loop head: in pf_each_cell the given-slope search measured 1 % slower (profiles/fit_frame_refactor.txt).
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(256) void k_rp_table(const double* __restrict__ ages, int A, int ht, double de,
                                                  double* __restrict__ tab) {
    const int total = (2 * ht + 1) * A;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int xx = idx / A, i = idx - xx * A;
        const double X = (double)(xx - ht) * de, kt = ages[i];
        tab[idx] = X * erf(X / (2.0 * sqrt(kt))) + (2.0 * sqrt(kt / M_PI)) * exp(-(X * X) / (4.0 * kt));
    }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_ramp(const double* __restrict__ z, int ny, int nx,
                                                        const long long* __restrict__ cells,
                                                        const double* __restrict__ dir, long long K,
                                                        const double* __restrict__ ages, int A, int h, int w, int M,
                                                        int mode, double slope, double de, double delta,
                                                        int min_samples, const double* __restrict__ etab,
                                                        const double* __restrict__ ftab_g,
                                                        sc_profile_ramp_fit* __restrict__ rows,
                                                        double* __restrict__ curve, signed char* __restrict__ widths) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, true>(ftab_g, np, 2 * (h + M) + 1, A);
    const double* slot = L.slot;
    const int* sm = (const int*)(slot + (size_t)SH_TERMS * A);
    const bool given = mode == SC_RAMP_SLOPE;
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        long long cell = 0;
        if (act) {
            cell = cells[kc];
            pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, L.prof, nullptr);
        }
        __syncthreads();
        if (act) {
            // what depends on neither the age nor the half-width, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, A);
            const int dof = mo.n - 3 - (!given && M > 0 ? 1 : 0);
            sc_profile_ramp_fit* out = rows + kc;
            if (mo.n_neg < min_samples || mo.n_pos < min_samples || dof < 1) {
                if (lane == 0) {
                    pf_row_unfit(out, cell, mo.n);
                    out->width_index = 0;
                    out->width = __builtin_nan("");
                    out->initial_slope = __builtin_nan("");
                }
                pf_unfit_planes(kc, lane, A, curve, widths);
            } else {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, A, t);
                rp_search(L.prof, etab, L.tab, np, h, A, M, given, slope, de, lane, f, L.slot);
                // lane i takes age i's winner
                const double sse = slot[A + ia];
                const int m = sm[ia];
                if (curve && lane < A) curve[kc * A + lane] = sse;
                if (widths && lane < A) widths[kc * A + lane] = (signed char)m;
                const pf_pick k = pf_choose(sse, lane, A, delta, dof);
                if (lane == k.best) {
                    const double a = slot[2 * A + ia], b = slot[3 * A + ia], c0 = slot[4 * A + ia];
                    pf_row_fit(out, cell, mo.n, k, pf_open(k, A) + (M > 0 && m == M ? 8 : 0), ages, a, b, c0, sse, dof);
                    out->width_index = m;
                    out->width = (double)m * de;
                    out->initial_slope = m ? rp_slope_of(a, b, m, de) : copysign(INFINITY, a);
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int sc_rp_check(sc_ctx* ctx, const char* who, int h, int M, int mode, double slope, int min_samples) {
    if (M < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the width range must be >= 0 cells", who);
    if (M > SC_PROFILE_MAX_WIDTH)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a half-width of %d cells, more than %d", who, M, SC_PROFILE_MAX_WIDTH);
    if (M > h - min_samples)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: a half-width of %d cells, more than h - min_samples = %d", who, M, h - min_samples);
    if (mode != SC_RAMP_FREE && mode != SC_RAMP_SLOPE)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: the mode must be SC_RAMP_FREE or SC_RAMP_SLOPE", who);
    if (mode == SC_RAMP_SLOPE) {
        if (M < 1) return sc_fail(ctx, SC_ERR_INVALID, "%s: a given slope needs a width range of at least one cell", who);
        if (!(isfinite(slope) && slope > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the slope must be finite and > 0", who);
    }
    return SC_OK;
}

int sc_rp_table(sc_ctx* ctx, const double* d_ages, int A, int ht, double de, double* d_ftab) {
    sc_prof_begin(ctx, SC_K_PROFILE);
    k_rp_table<<<std::max(1, std::min(256, ((2 * ht + 1) * A + 255) / 256)), 256, 0, ctx->stream>>>(d_ages, A, ht, de, d_ftab);
    SC_HIP(ctx, hipGetLastError());
    sc_prof_end(ctx, 1);
    return SC_OK;
}

static int rp_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, const double* ages, int A, int h, int w, int M, int mode, double slope, double de, double delta,
                  int min_samples, sc_profile_ramp_fit* out_rows, double* out_sse, int8_t* out_width) {
    const int np = 2 * h + 1, ht = h + M, nt = 2 * ht + 1;
    const size_t etab_bytes = sizeof(double) * (size_t)np * A, ftab_bytes = sizeof(double) * (size_t)nt * A;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, etab_bytes))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ftab, ftab_bytes))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_etab = (double*)ctx->pf_tab.p;
    double* d_ftab = (double*)ctx->pf_ftab.p;

    const bool tab_lds = ftab_bytes <= PF_TAB_LDS;
    const size_t lds = pf_lds_bytes(np, nt, A, true, tab_lds);
    const auto kern = tab_lds ? k_pf_ramp<true> : k_pf_ramp<false>;
    if ((rc = sc_lds_attr(ctx, (const void*)kern, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    // (the erf table of the m = 0 pairs is the plain call's, by its launch: the same bits)
    if ((rc = sc_pf_table(ctx, d_ages, A, h, de, d_etab))) return rc;
    if ((rc = sc_rp_table(ctx, d_ages, A, ht, de, d_ftab))) return rc;

    const pf_plane curve = {out_sse, &ctx->pf_sse, sizeof(double) * (size_t)A}, widths = {out_width, &ctx->pf_shift, (size_t)A};
    return sc_pf_chunks(ctx, cells, sa, ca, K, PF_CHUNK, sizeof(sc_profile_ramp_fit), out_rows, curve, widths,
                        [&](const pf_chunk& d, long long m) {
        kern<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, d_ages, A, h, w, M, mode, slope, de, delta,
                                                          min_samples, d_etab, d_ftab, (sc_profile_ramp_fit*)d.rows,
                                                          (double*)d.plane[0], (signed char*)d.plane[1]);
    });
}

// The two calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null).
static int rp_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const double* ages, int A, int h, int w, int M, int mode, double slope,
                   double de, double delta, int min_samples, sc_profile_ramp_fit* out_rows, double* out_sse,
                   int8_t* out_width) {
    int rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if ((rc = sc_rp_check(ctx, who, h, M, mode, slope, min_samples))) return rc;
    if (K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    return rp_run(ctx, z_dev, ny, nx, cells, sa, ca, K, ages, A, h, w, M, mode, slope, de, delta, min_samples, out_rows, out_sse,
                  out_width);
}

extern "C" int sc_fit_profiles_ramp(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                    const double* ages, int A, int h, int w, int M, int mode, double slope, double de,
                                    double delta, int min_samples, sc_profile_ramp_fit* out_rows, double* out_sse,
                                    int8_t* out_width) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_profiles_ramp");
    if (rc) return rc;
    return rp_call(ctx, "sc_fit_profiles_ramp", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, ages, A, h, w, M, mode, slope, de,
                   delta, min_samples, out_rows, out_sse, out_width);
}

extern "C" int sc_fit_profiles_ramp_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                        const double* sa, const double* ca, long long K, const double* ages, int A, int h,
                                        int w, int M, int mode, double slope, double de, double delta, int min_samples,
                                        sc_profile_ramp_fit* out_rows, double* out_sse, int8_t* out_width) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return rp_call(ctx, "sc_fit_profiles_ramp_dem", z, ny, nx, cells, sa, ca, K, ages, A, h, w, M, mode, slope, de, delta,
                   min_samples, out_rows, out_sse, out_width);
}
