// sc_channel_profiles* : channel depth and width across a trace (docs/channels.md).
//
// The Channel search's window, the Ricker wavelet, is a multiple of the second derivative of exp(-(pi f x)^2): the
// elevation model it assumes is a Gaussian trough across the strike,
//   z(s) = c0 + b s + a exp(-(pi f (s - d de))^2),   a < 0: a channel, a > 0: a ridge
// - linear in (c0, b, a) for a fixed (frequency f, centre shift d), which is the structure sc_fit_profiles_shift fits.
// The pieces are those of sc_fit.h; the search has its own text because a pair can be dead (ch_search, sc_channel.h,
// which the joint fit of sc_channel_segment.hip shares with this file).
//   k_ch_table   G over x = -(h + D)..(h + D) and the frequencies, frequency-minor: one exp per entry
//   k_ch_terms   what a pair's column leaves against (1, s) on a profile WITHOUT a missing point - ebar, gamma, See -
//                depends on (i, d, h, de) alone: one thread per pair runs the loops of pf_moments, pf_line and
//                pf_column over a profile of zeros, once per call, into three planes of F (2D + 1) doubles in global
//                memory (14 KB at 35 frequencies and D = 8: every wave reads the same lines, which the L2 holds;
//                beside G in LDS they would cost the second workgroup of a CU)
//   k_ch_fit     k_pf_shift's shape: one wave per cell, PF_WAVES cells per workgroup, pf_cut into the wave's LDS;
//                pf_moments and pf_line without a column, once; then the lanes run over the (shift, frequency) pairs
//                (ch_search), whose winners per frequency come back in the wave's slot of LDS, and pf_choose runs on
//                sse*.  A wave whose profile is complete takes (ebar, gamma, See) of its pair from k_ch_terms' planes
//                and runs two sweeps - Sep, then the residuals - for pf_candidate's four; a wave with a missing
//                point runs pf_candidate.  The branch is uniform per wave, the sums are the same operations in the
//                same order, and the library is built with -ffp-contract=off: both routes return the same bytes
//                (option "channel_terms" 0 switches the planes off; tests/test_gpu_channels.py compares).
// G sits in LDS when it fits PF_TAB_LDS bytes (35 frequencies, h = 100, D = 8: 60.8 KB) and in global memory otherwise
// (pf_stage).  No atomics at all, no float sum across lanes.  The host side is the table set-up, the kernel choice and
// one call of sc_pf_chunks (sc_profile.hip).
#include "sc_channel.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(256) void k_ch_table(const double* __restrict__ freqs, int F, int ht, double de,
                                                  double* __restrict__ tab) {
    const int total = (2 * ht + 1) * F;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int xx = idx / F, i = idx - xx * F;
        const double X = (double)(xx - ht) * de;
        const double u = (M_PI * freqs[i]) * X;
        tab[idx] = exp(-(u * u));
    }
}

// zeros: np doubles, all 0 - the complete profile; terms: ebar, gamma, See, a plane of P = F (2D + 1) each
__global__ __launch_bounds__(256) void k_ch_terms(const double* __restrict__ tab, const double* __restrict__ zeros, int F,
                                                  int h, int D, double de, double* __restrict__ terms) {
    const int np = 2 * h + 1, P = F * (2 * D + 1);
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int r = q / F, i = q - r * F;
    const pf_mom mo = pf_moments<false>(zeros, np, h, de, nullptr, F);
    pf_col t;
    const pf_lin L = pf_line<false>(zeros, np, h, de, mo, nullptr, F, t);
    t = pf_column(zeros, np, h, de, L, ch_col(tab, F, D, r, i));
    terms[q] = t.ebar;
    terms[(size_t)P + q] = t.gamma;
    terms[2 * (size_t)P + q] = t.See;
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_ch_fit(const double* __restrict__ z, int ny, int nx,
                                                       const long long* __restrict__ cells,
                                                       const double* __restrict__ dir, long long K,
                                                       const double* __restrict__ freqs, int F, int h, int w, int D,
                                                       double de, double delta, int min_samples,
                                                       const double* __restrict__ tab_g, const double* __restrict__ terms,
                                                       sc_profile_shift_fit* __restrict__ rows,
                                                       double* __restrict__ curve, signed char* __restrict__ shifts) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63;
    const pf_lds L = pf_stage<TAB_LDS, true>(tab_g, np, 2 * (h + D) + 1, F);
    const double* slot = L.slot;
    const int* srank = (const int*)(slot + (size_t)SH_TERMS * F);
    const int ia = min(lane, F - 1);                     // lanes beyond the frequencies repeat the last one and are ignored
    pf_each_cell(
        cells, K, [&](long long kc, long long cell) { pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, L.prof, nullptr); },
        [&](long long kc, long long cell) {
            // what depends on neither the frequency nor the shift, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, F);
            const int dof = mo.n - 3 - (D > 0 ? 1 : 0);
            sc_profile_shift_fit* out = rows + kc;
            int unfit = (mo.n_neg < min_samples || mo.n_pos < min_samples || dof < 1) ? 1 : 0;
            double sse = 0.0;
            int d = 0;
            if (!unfit) {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, F, t);
                ch_search(L.prof, L.tab, mo.n == np ? terms : nullptr, np, h, F, D, de, lane, f, L.slot);
                // lane i takes frequency i's winner
                sse = slot[F + ia];
                d = sh_shift_of(srank[ia]);
                if (!__ballot(lane < F && sse == sse)) unfit = 1 | 32;         // no frequency has a live pair
            }
            if (unfit) {
                if (lane == 0) {
                    pf_row_unfit(out, cell, mo.n);
                    out->status = unfit;
                    out->shift_index = 0;
                    out->shift = __builtin_nan("");
                }
                pf_unfit_planes(kc, lane, F, curve, shifts);
            } else {
                if (curve && lane < F) curve[kc * F + lane] = sse;
                if (shifts && lane < F) shifts[kc * F + lane] = (signed char)d;
                const pf_pick k = pf_choose(sse, lane, F, delta, dof);
                if (lane == k.best) {
                    pf_row_fit(out, cell, mo.n, k, pf_open(k, F) + (D > 0 && (d == D || d == -D) ? 8 : 0), freqs,
                               slot[2 * F + ia], slot[3 * F + ia], slot[4 * F + ia], sse, dof);
                    out->shift_index = d;
                    out->shift = (double)d * de;
                }
            }
        });
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int sc_ch_tables(sc_ctx* ctx, const double* d_freqs, int F, int h, int D, double de, double* d_tab, const double** d_terms) {
    const int np = 2 * h + 1, ht = h + D, nt = 2 * ht + 1, P = F * (2 * D + 1);
    int rc;
    // (the profile of zeros, then the three planes)
    if ((rc = sc_ensure(ctx, ctx->pf_terms, sizeof(double) * ((size_t)np + 3 * (size_t)P)))) return rc;
    double* d_zeros = (double*)ctx->pf_terms.p;
    double* terms = ctx->channel_terms ? d_zeros + np : nullptr;
    if (terms) SC_HIP(ctx, hipMemsetAsync(d_zeros, 0, sizeof(double) * (size_t)np, ctx->stream));
    sc_prof_begin(ctx, SC_K_PROFILE);
    k_ch_table<<<std::max(1, std::min(256, (nt * F + 255) / 256)), 256, 0, ctx->stream>>>(d_freqs, F, ht, de, d_tab);
    if (terms) k_ch_terms<<<(P + 255) / 256, 256, 0, ctx->stream>>>(d_tab, d_zeros, F, h, D, de, terms);
    SC_HIP(ctx, hipGetLastError());
    sc_prof_end(ctx, terms ? 2 : 1);
    *d_terms = terms;
    return SC_OK;
}

static int ch_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, const double* freqs, int F, int h, int w, int D, double de, double delta, int min_samples,
                  sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    const int np = 2 * h + 1, ht = h + D, nt = 2 * ht + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)nt * F;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * F))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    double* d_freqs = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;
    const double* d_terms;

    const bool tab_lds = tab_bytes <= PF_TAB_LDS;
    const size_t lds = pf_lds_bytes(np, nt, F, true, tab_lds);
    const auto kern = tab_lds ? k_ch_fit<true> : k_ch_fit<false>;
    if ((rc = sc_lds_attr(ctx, (const void*)kern, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_freqs, freqs, sizeof(double) * F, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sc_ch_tables(ctx, d_freqs, F, h, D, de, d_tab, &d_terms))) return rc;

    const pf_plane curve = {out_sse, &ctx->pf_sse, sizeof(double) * (size_t)F}, shifts = {out_shift, &ctx->pf_shift, (size_t)F};
    return sc_pf_chunks(ctx, cells, sa, ca, K, PF_CHUNK, sizeof(sc_profile_shift_fit), out_rows, curve, shifts,
                        [&](const pf_chunk& d, long long m) {
        kern<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, d_freqs, F, h, w, D, de, delta, min_samples,
                                                          d_tab, d_terms, (sc_profile_shift_fit*)d.rows, (double*)d.plane[0],
                                                          (signed char*)d.plane[1]);
    });
}

// what a channel call checks of its frequencies ahead of its frame's checks ...
int sc_ch_check_freqs(sc_ctx* ctx, const char* who, const double* freqs, int F) {
    if (!freqs) return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (F < 1) return sc_fail(ctx, SC_ERR_INVALID, "%s: needs F >= 1", who);
    if (F > SC_CHANNEL_MAX_FREQS)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d frequencies, more than %d", who, F, SC_CHANNEL_MAX_FREQS);
    for (int i = 0; i < F; ++i)
        if (!(isfinite(freqs[i]) && freqs[i] > 0.0 && (i == 0 || freqs[i] > freqs[i - 1])))
            return sc_fail(ctx, SC_ERR_INVALID, "%s: frequencies must be finite, positive and strictly increasing", who);
    return SC_OK;
}

// ... and behind them (the largest frequency is the last one)
int sc_ch_check_arg(sc_ctx* ctx, const char* who, const double* freqs, int F, double de) {
    if (!((M_PI * freqs[F - 1]) * de <= SC_CHANNEL_MAX_ARG))
        return sc_fail(ctx, SC_ERR_INVALID, "%s: pi f de = %g at the last frequency, more than %g: narrower than a cell shows", who,
                       (M_PI * freqs[F - 1]) * de, SC_CHANNEL_MAX_ARG);
    return SC_OK;
}

// The two calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null).
static int ch_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const double* freqs, int F, int h, int w, int D, double de, double delta,
                   int min_samples, sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    int rc = sc_ch_check_freqs(ctx, who, freqs, F);
    if (rc) return rc;
    if ((rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, freqs, F, h, w, de, delta, min_samples, out_rows))) return rc;
    if ((rc = sc_pf_check_shift(ctx, who, h, D, min_samples))) return rc;
    if ((rc = sc_ch_check_arg(ctx, who, freqs, F, de))) return rc;
    if (K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    return ch_run(ctx, z_dev, ny, nx, cells, sa, ca, K, freqs, F, h, w, D, de, delta, min_samples, out_rows, out_sse, out_shift);
}

extern "C" int sc_channel_profiles(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                   const double* frequencies, int F, int h, int w, int D, double de, double delta,
                                   int min_samples, sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_channel_profiles");
    if (rc) return rc;
    return ch_call(ctx, "sc_channel_profiles", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, frequencies, F, h, w, D, de, delta,
                   min_samples, out_rows, out_sse, out_shift);
}

extern "C" int sc_channel_profiles_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                       const double* ca, long long K, const double* frequencies, int F, int h, int w, int D,
                                       double de, double delta, int min_samples, sc_profile_shift_fit* out_rows,
                                       double* out_sse, int8_t* out_shift) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return ch_call(ctx, "sc_channel_profiles_dem", z, ny, nx, cells, sa, ca, K, frequencies, F, h, w, D, de, delta, min_samples,
                   out_rows, out_sse, out_shift);
}
