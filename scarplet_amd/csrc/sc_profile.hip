// sc_fit_profiles / sc_fit_profiles_dem: scarp-profile dating across a trace (docs/profiles.md).
//
// For each cell a profile of 2h + 1 points is cut across the strike (each point the mean of up to 2w + 1 bilinear
// samples along the strike), and z(s) = c0 + b s + a erf(s / (2 sqrt(kt))) is fitted to it for each of A ages.
//   k_pf_table   the erf column of every (point, age): it depends on the cell in no way, so it is a table of
//                (2h + 1) x A float64, age-minor, built once per call
//   k_pf_fit     one wave per cell, PF_WAVES cells per workgroup, workgroups striding over the cells so that the
//                cells in flight are neighbours of the input order (cells of one trace share their samples' lines)
//     sampling   lanes over the points j, the 2w + 1 samples of a point summed in ascending k; the profile goes to
//                the wave's slice of LDS, NaN marking a point without a valid sample
//     fit        lanes over the AGES: lane i walks the whole profile for age i - the profile is an LDS broadcast,
//                the table row j is A consecutive doubles - in four passes (sums and means; the centred s against
//                p and e; the residual column e'' against the detrended p; the explicit residuals).  Every sum is a
//                plain loop over ascending j in one lane: no cross-lane reduction, the same bits every run, and a
//                profile with missing points is the same code as a complete one.
//     choice     argmin over the lanes (ties to the smaller age index), a ballot of sse <= thr for the interval
// The table sits in LDS when it fits PF_TAB_LDS bytes (35 ages at h = 100: 56 KB) and in global memory otherwise.
// No atomics at all.
#include "sc_internal.h"
#include <math.h>
#include <algorithm>

#define PF_WAVES 4                       // cells in flight per workgroup
#define PF_THREADS (64 * PF_WAVES)
#define PF_TAB_LDS 65536                 // the table goes to LDS up to this many bytes
#define PF_CHUNK (1ll << 19)             // cells per launch: bounds the call's buffers (96 B a row, 8 A B a curve)
#define PF_MAX_GRID 2048

__global__ __launch_bounds__(256) void k_pf_table(const double* __restrict__ ages, int A, int h, double de,
                                                  double* __restrict__ tab) {
    const int total = (2 * h + 1) * A;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int jj = idx / A, i = idx - jj * A;
        const double s = (double)(jj - h) * de;
        tab[idx] = erf(s / (2.0 * sqrt(ages[i])));
    }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_fit(const double* __restrict__ z, int ny, int nx,
                                                       const long long* __restrict__ cells,
                                                       const double* __restrict__ dir, long long K,
                                                       const double* __restrict__ ages, int A, int h, int w, double de,
                                                       double delta, int min_samples, const double* __restrict__ tab_g,
                                                       sc_profile_fit* __restrict__ rows, double* __restrict__ curve) {
    extern __shared__ double pf_lds[];
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* prof = pf_lds + (size_t)wave * np;
    const double* tab = tab_g;
    if (TAB_LDS) {
        double* t = pf_lds + (size_t)PF_WAVES * np;
        for (int idx = threadIdx.x; idx < np * A; idx += PF_THREADS) t[idx] = tab_g[idx];
        tab = t;
    }
    __syncthreads();
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        long long cell = 0;
        if (act) {
            cell = cells[kc];
            const double sa = dir[2 * kc], ca = dir[2 * kc + 1];
            const double r = (double)(cell / nx), c = (double)(cell % nx);
            for (int jj = lane; jj < np; jj += 64) {
                const double j = (double)(jj - h);
                const double jsa = j * sa, jca = j * ca;
                double acc = 0.0;
                int cnt = 0;
                for (int kk = -w; kk <= w; ++kk) {
                    const double k = (double)kk;
                    const double rr = r + (k * ca - jsa), cc = c + (jca + k * sa);
                    double v;
                    if (pf_sample(z, ny, nx, rr, cc, v)) {
                        acc += v;
                        ++cnt;
                    }
                }
                prof[jj] = cnt ? acc / (double)cnt : nan;
            }
        }
        __syncthreads();
        if (act) {
            // pass 0: counts, sums of s, p and this lane's e over the valid points
            int n = 0, n_neg = 0, n_pos = 0;
            double Ss = 0.0, Sp = 0.0, Se = 0.0;
            for (int jj = 0; jj < np; ++jj) {
                const double p = prof[jj];
                if (p != p) continue;
                ++n;
                n_neg += jj < h ? 1 : 0;
                n_pos += jj > h ? 1 : 0;
                Ss += (double)(jj - h) * de;
                Sp += p;
                Se += tab[(size_t)jj * A + ia];
            }
            sc_profile_fit* out = rows + kc;
            if (n_neg < min_samples || n_pos < min_samples) {
                if (lane == 0) {
                    out->cell = cell;
                    out->n = n;
                    out->kt_index = -1;
                    out->lo_index = -1;
                    out->hi_index = -1;
                    out->status = 1;
                    out->kt = nan; out->kt_lo = nan; out->kt_hi = nan;
                    out->a = nan; out->b = nan; out->c0 = nan;
                    out->sse = nan; out->rmse = nan;
                }
                if (curve && lane < A) curve[kc * A + lane] = nan;
            } else {
                const double dn = (double)n;
                const double sbar = Ss / dn, pbar = Sp / dn, ebar = Se / dn;
                // pass 1: the centred s against itself, p and e
                double Sss = 0.0, Sps = 0.0, Ses = 0.0;
                for (int jj = 0; jj < np; ++jj) {
                    const double p = prof[jj];
                    if (p != p) continue;
                    const double sc = (double)(jj - h) * de - sbar;
                    Sss += sc * sc;
                    Sps += sc * (p - pbar);
                    Ses += sc * (tab[(size_t)jj * A + ia] - ebar);
                }
                const double beta = Sps / Sss, gamma = Ses / Sss;
                // pass 2: what is left of e after 1 and s, against what is left of p
                double See = 0.0, Sep = 0.0;
                for (int jj = 0; jj < np; ++jj) {
                    const double p = prof[jj];
                    if (p != p) continue;
                    const double sc = (double)(jj - h) * de - sbar;
                    const double e2 = (tab[(size_t)jj * A + ia] - ebar) - gamma * sc;
                    const double p2 = (p - pbar) - beta * sc;
                    See += e2 * e2;
                    Sep += e2 * p2;
                }
                const double a = Sep / See;
                const double b = beta - a * gamma;
                const double c0 = (pbar - a * ebar) - b * sbar;
                // pass 3: the explicit residuals
                double sse = 0.0;
                for (int jj = 0; jj < np; ++jj) {
                    const double p = prof[jj];
                    if (p != p) continue;
                    const double s = (double)(jj - h) * de;
                    const double res = p - ((c0 + b * s) + a * tab[(size_t)jj * A + ia]);
                    sse += res * res;
                }
                if (curve && lane < A) curve[kc * A + lane] = sse;
                // argmin over the ages, ties to the smaller index (a NaN never wins)
                double m = lane < A ? sse : INFINITY;
                if (m != m) m = INFINITY;
                int mi = lane;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double om = __shfl_xor(m, o, 64);
                    const int oi = __shfl_xor(mi, o, 64);
                    if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
                }
                const int best = min(mi, A - 1);
                const double thr = m * (1.0 + delta / (double)(n - 3));
                const unsigned long long ok = __ballot(lane < A && sse <= thr);
                int lo = best, hi = best;
                while (lo > 0 && ((ok >> (lo - 1)) & 1ull)) --lo;
                while (hi < A - 1 && ((ok >> (hi + 1)) & 1ull)) ++hi;
                if (lane == best) {
                    out->cell = cell;
                    out->n = n;
                    out->kt_index = best;
                    out->lo_index = lo;
                    out->hi_index = hi;
                    out->status = (lo == 0 ? 2 : 0) + (hi == A - 1 ? 4 : 0);
                    out->kt = ages[best]; out->kt_lo = ages[lo]; out->kt_hi = ages[hi];
                    out->a = a; out->b = b; out->c0 = c0;
                    out->sse = sse; out->rmse = sqrt(sse / (double)(n - 3));
                }
            }
        }
        __syncthreads();
    }
}

// sc_fit_profiles_shift: the same wave per cell, sampling and LDS profile; the table covers j = -(h + D)..(h + D) and
// the lanes run over the (shift, age) pairs (sh_search, sc_internal.h), whose winners per age come back in the wave's
// slot of LDS.  The choice over the ages is k_pf_fit's, on sse*.
template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_shift(const double* __restrict__ z, int ny, int nx,
                                                         const long long* __restrict__ cells,
                                                         const double* __restrict__ dir, long long K,
                                                         const double* __restrict__ ages, int A, int h, int w, int D,
                                                         double de, double delta, int min_samples,
                                                         const double* __restrict__ tab_g,
                                                         sc_profile_shift_fit* __restrict__ rows,
                                                         double* __restrict__ curve, signed char* __restrict__ shifts) {
    extern __shared__ double pf_lds[];
    const int np = 2 * h + 1, nt = 2 * (h + D) + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* prof = pf_lds + (size_t)wave * np;
    double* slot = pf_lds + (size_t)PF_WAVES * np + (size_t)wave * sh_slot_doubles(A);
    const double* tab = tab_g;
    if (TAB_LDS) {
        double* t = pf_lds + (size_t)PF_WAVES * (np + sh_slot_doubles(A));
        for (int idx = threadIdx.x; idx < nt * A; idx += PF_THREADS) t[idx] = tab_g[idx];
        tab = t;
    }
    __syncthreads();
    const int* srank = (const int*)(slot + (size_t)SH_TERMS * A);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        long long cell = 0;
        if (act) {
            cell = cells[kc];
            const double sa = dir[2 * kc], ca = dir[2 * kc + 1];
            const double r = (double)(cell / nx), c = (double)(cell % nx);
            for (int jj = lane; jj < np; jj += 64) prof[jj] = pf_point(z, ny, nx, r, c, sa, ca, jj, h, w);
        }
        __syncthreads();
        if (act) {
            // what depends on neither the age nor the shift, once: pass 0's counts and sums of s and p
            int n = 0, n_neg = 0, n_pos = 0;
            double Ss = 0.0, Sp = 0.0;
            for (int jj = 0; jj < np; ++jj) {
                const double p = prof[jj];
                if (p != p) continue;
                ++n;
                n_neg += jj < h ? 1 : 0;
                n_pos += jj > h ? 1 : 0;
                Ss += (double)(jj - h) * de;
                Sp += p;
            }
            const int dof = n - 3 - (D > 0 ? 1 : 0);
            sc_profile_shift_fit* out = rows + kc;
            if (n_neg < min_samples || n_pos < min_samples || dof < 1) {
                if (lane == 0) {
                    out->cell = cell;
                    out->n = n;
                    out->kt_index = -1;
                    out->lo_index = -1;
                    out->hi_index = -1;
                    out->status = 1;
                    out->kt = nan; out->kt_lo = nan; out->kt_hi = nan;
                    out->a = nan; out->b = nan; out->c0 = nan;
                    out->sse = nan; out->rmse = nan;
                    out->shift_index = 0;
                    out->shift = nan;
                }
                if (curve && lane < A) curve[kc * A + lane] = nan;
                if (shifts && lane < A) shifts[kc * A + lane] = 0;
            } else {
                const double dn = (double)n;
                const double sbar = Ss / dn, pbar = Sp / dn;
                // ... and pass 1's centred s against itself and p
                double Sss = 0.0, Sps = 0.0;
                for (int jj = 0; jj < np; ++jj) {
                    const double p = prof[jj];
                    if (p != p) continue;
                    const double sc = (double)(jj - h) * de - sbar;
                    Sss += sc * sc;
                    Sps += sc * (p - pbar);
                }
                const double beta = Sps / Sss;
                sh_search(prof, tab, np, h, A, D, de, lane, dn, sbar, pbar, Sss, beta, slot);
                // lane i takes age i's winner
                const double sse = slot[ia];
                const int d = sh_shift_of(srank[ia]);
                if (curve && lane < A) curve[kc * A + lane] = sse;
                if (shifts && lane < A) shifts[kc * A + lane] = (signed char)d;
                // argmin over the ages, ties to the smaller index (a NaN never wins)
                double m = lane < A ? sse : INFINITY;
                if (m != m) m = INFINITY;
                int mi = lane;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double om = __shfl_xor(m, o, 64);
                    const int oi = __shfl_xor(mi, o, 64);
                    if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
                }
                const int best = min(mi, A - 1);
                const double thr = m * (1.0 + delta / (double)dof);
                const unsigned long long ok = __ballot(lane < A && sse <= thr);
                int lo = best, hi = best;
                while (lo > 0 && ((ok >> (lo - 1)) & 1ull)) --lo;
                while (hi < A - 1 && ((ok >> (hi + 1)) & 1ull)) ++hi;
                if (lane == best) {
                    const double ebar = slot[3 * A + ia], gamma = slot[4 * A + ia];
                    const double a = slot[2 * A + ia] / slot[A + ia];
                    const double b = beta - a * gamma;
                    const double c0 = (pbar - a * ebar) - b * sbar;
                    out->cell = cell;
                    out->n = n;
                    out->kt_index = best;
                    out->lo_index = lo;
                    out->hi_index = hi;
                    out->status = (lo == 0 ? 2 : 0) + (hi == A - 1 ? 4 : 0) + (D > 0 && (d == D || d == -D) ? 8 : 0);
                    out->kt = ages[best]; out->kt_lo = ages[lo]; out->kt_hi = ages[hi];
                    out->a = a; out->b = b; out->c0 = c0;
                    out->sse = sse; out->rmse = sqrt(sse / (double)dof);
                    out->shift_index = d;
                    out->shift = (double)d * de;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// (shared with sc_fit_segments: `who` names the call in the messages)
int sc_pf_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const double* ages, int A, int h, int w, double de, double delta,
                int min_samples, const void* out_rows) {
    if (K < 0 || (K > 0 && (!cells || !sa || !ca || !out_rows)) || !ages)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (ny < 2 || nx < 2) return sc_fail(ctx, SC_ERR_INVALID, "%s: the grid must be at least 2 x 2", who);
    if (A < 1 || h < 1 || w < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: needs A >= 1, h >= 1, w >= 0", who);
    if (A > SC_PROFILE_MAX_AGES) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d ages, more than %d", who, A, SC_PROFILE_MAX_AGES);
    if (h > SC_PROFILE_MAX_HALF) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: half-length %d cells, more than %d", who, h, SC_PROFILE_MAX_HALF);
    if (w > SC_PROFILE_MAX_SWATH) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: swath %d cells, more than %d", who, w, SC_PROFILE_MAX_SWATH);
    if (K > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %lld cells, more than 2^31 - 1", who, K);
    if (min_samples < 2 || min_samples > h)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: min_samples must lie in 2..h", who);
    if (!(isfinite(delta) && delta >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: delta must be finite and >= 0", who);
    if (!(isfinite(de) && de > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the cell size must be finite and > 0", who);
    for (int i = 0; i < A; ++i)
        if (!(isfinite(ages[i]) && ages[i] > 0.0 && (i == 0 || ages[i] > ages[i - 1])))
            return sc_fail(ctx, SC_ERR_INVALID, "%s: ages must be finite, positive and strictly increasing", who);
    const long long nc = ny * nx;
    for (long long k = 0; k < K; ++k) {
        if (cells[k] < 0 || cells[k] >= nc) return sc_fail(ctx, SC_ERR_INVALID, "%s: cell %lld outside the grid", who, cells[k]);
        if (!(isfinite(sa[k]) && isfinite(ca[k]))) return sc_fail(ctx, SC_ERR_INVALID, "%s: sa / ca not finite at cell %lld", who, k);
    }
    return SC_OK;
}

int sc_pf_table(sc_ctx* ctx, const double* d_ages, int A, int h, double de, double* d_tab) {
    const int np = 2 * h + 1;
    sc_prof_begin(ctx, SC_K_PROFILE);
    k_pf_table<<<std::max(1, std::min(256, (np * A + 255) / 256)), 256, 0, ctx->stream>>>(d_ages, A, h, de, d_tab);
    SC_HIP(ctx, hipGetLastError());
    sc_prof_end(ctx, 1);
    return SC_OK;
}

static int pf_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                  sc_profile_fit* out_rows, double* out_sse) {
    if (K == 0) return SC_OK;
    const int np = 2 * h + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)np * A;
    const long long chunk = std::min<long long>(K, PF_CHUNK);
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_cells, sizeof(long long) * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_dir, sizeof(double) * 2 * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_rows, sizeof(sc_profile_fit) * (size_t)chunk))) return rc;
    if (out_sse && (rc = sc_ensure(ctx, ctx->pf_sse, sizeof(double) * (size_t)A * (size_t)chunk))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;
    long long* d_cells = (long long*)ctx->pf_cells.p;
    double* d_dir = (double*)ctx->pf_dir.p;
    sc_profile_fit* d_rows = (sc_profile_fit*)ctx->pf_rows.p;
    double* d_sse = out_sse ? (double*)ctx->pf_sse.p : nullptr;

    const bool tab_lds = tab_bytes <= PF_TAB_LDS;
    const size_t lds = sizeof(double) * (size_t)PF_WAVES * np + (tab_lds ? tab_bytes : 0);
    const void* fn = tab_lds ? (const void*)k_pf_fit<true> : (const void*)k_pf_fit<false>;
    if ((rc = sc_lds_attr(ctx, fn, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sc_pf_table(ctx, d_ages, A, h, de, d_tab))) return rc;

    std::vector<double> dir;
    for (long long k0 = 0; k0 < K; k0 += chunk) {
        const long long m = std::min(chunk, K - k0);
        dir.resize(2 * (size_t)m);
        for (long long k = 0; k < m; ++k) {
            dir[2 * k] = sa[k0 + k];
            dir[2 * k + 1] = ca[k0 + k];
        }
        SC_HIP(ctx, hipMemcpyAsync(d_cells, cells + k0, sizeof(long long) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(d_dir, dir.data(), sizeof(double) * 2 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        // (the rows' padding is part of what the caller compares: cleared, the kernel writes the fields)
        SC_HIP(ctx, hipMemsetAsync(d_rows, 0, sizeof(sc_profile_fit) * (size_t)m, ctx->stream));
        const unsigned grid = (unsigned)std::min<long long>((m + PF_WAVES - 1) / PF_WAVES, PF_MAX_GRID);
        sc_prof_begin(ctx, SC_K_PROFILE);
        if (tab_lds)
            k_pf_fit<true><<<grid, PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d_cells, d_dir, m, d_ages, A, h, w, de, delta,
                                                                   min_samples, d_tab, d_rows, d_sse);
        else
            k_pf_fit<false><<<grid, PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d_cells, d_dir, m, d_ages, A, h, w, de, delta,
                                                                    min_samples, d_tab, d_rows, d_sse);
        SC_HIP(ctx, hipGetLastError());
        sc_prof_end(ctx, 1);
        SC_HIP(ctx, hipMemcpyAsync(out_rows + k0, d_rows, sizeof(sc_profile_fit) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        if (out_sse)
            SC_HIP(ctx, hipMemcpyAsync(out_sse + (size_t)k0 * A, d_sse, sizeof(double) * (size_t)A * (size_t)m,
                                       hipMemcpyDeviceToHost, ctx->stream));
        // (dir is reused by the next chunk, and the caller owns the outputs on return)
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SC_OK;
}

extern "C" int sc_fit_profiles(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                               const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                               sc_profile_fit* out_rows, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const Geom& g = ctx->g;
    if (g.ly != g.ny || g.lx != g.nx || g.gy0 != 0 || g.gx0 != 0 || g.cy0 != 0 || g.cx0 != 0 || g.cy1 != g.ny || g.cx1 != g.nx)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_fit_profiles: the context holds a block of a larger grid");
    int rc = sc_pf_check(ctx, "sc_fit_profiles", g.ny, g.nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return pf_run(ctx, ctx->z_dev, g.ny, g.nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows, out_sse);
}

extern "C" int sc_fit_profiles_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                   const double* ca, long long K, const double* ages, int A, int h, int w, double de,
                                   double delta, int min_samples, sc_profile_fit* out_rows, double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    int rc = sc_pf_check(ctx, "sc_fit_profiles", ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if (K == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * (size_t)ny * (size_t)nx;
    if ((rc = sc_ensure(ctx, ctx->pf_z, bytes))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->pf_z.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    return pf_run(ctx, (const double*)ctx->pf_z.p, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows,
                  out_sse);
}

// ---------------------------------------------------------------------------------------------------------------
// the centre shift
// ---------------------------------------------------------------------------------------------------------------
// (shared with sc_fit_segments_shift)
int sc_pf_check_shift(sc_ctx* ctx, const char* who, int h, int D, int min_samples) {
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    if (D > SC_PROFILE_MAX_SHIFT) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a shift of %d cells, more than %d", who, D, SC_PROFILE_MAX_SHIFT);
    if (D > h - min_samples)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: a shift of %d cells, more than h - min_samples = %d", who, D, h - min_samples);
    return SC_OK;
}

static int pf_shift_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                        const double* ca, long long K, const double* ages, int A, int h, int w, int D, double de,
                        double delta, int min_samples, sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (K == 0) return SC_OK;
    const int np = 2 * h + 1, nt = 2 * (h + D) + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)nt * A;
    const long long chunk = std::min<long long>(K, PF_CHUNK);
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_cells, sizeof(long long) * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_dir, sizeof(double) * 2 * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_rows, sizeof(sc_profile_shift_fit) * (size_t)chunk))) return rc;
    if (out_sse && (rc = sc_ensure(ctx, ctx->pf_sse, sizeof(double) * (size_t)A * (size_t)chunk))) return rc;
    if (out_shift && (rc = sc_ensure(ctx, ctx->pf_shift, (size_t)A * (size_t)chunk))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;
    long long* d_cells = (long long*)ctx->pf_cells.p;
    double* d_dir = (double*)ctx->pf_dir.p;
    sc_profile_shift_fit* d_rows = (sc_profile_shift_fit*)ctx->pf_rows.p;
    double* d_sse = out_sse ? (double*)ctx->pf_sse.p : nullptr;
    signed char* d_shift = out_shift ? (signed char*)ctx->pf_shift.p : nullptr;

    const bool tab_lds = tab_bytes <= PF_TAB_LDS;
    const size_t lds = sizeof(double) * (size_t)PF_WAVES * (np + sh_slot_doubles(A)) + (tab_lds ? tab_bytes : 0);
    const void* fn = tab_lds ? (const void*)k_pf_shift<true> : (const void*)k_pf_shift<false>;
    if ((rc = sc_lds_attr(ctx, fn, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    // (rows -h..h of the table over h + D are the bits of the table over h: s = (double)j * de either way)
    if ((rc = sc_pf_table(ctx, d_ages, A, h + D, de, d_tab))) return rc;

    std::vector<double> dir;
    for (long long k0 = 0; k0 < K; k0 += chunk) {
        const long long m = std::min(chunk, K - k0);
        dir.resize(2 * (size_t)m);
        for (long long k = 0; k < m; ++k) {
            dir[2 * k] = sa[k0 + k];
            dir[2 * k + 1] = ca[k0 + k];
        }
        SC_HIP(ctx, hipMemcpyAsync(d_cells, cells + k0, sizeof(long long) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(d_dir, dir.data(), sizeof(double) * 2 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        // (the rows' padding is part of what the caller compares: cleared, the kernel writes the fields)
        SC_HIP(ctx, hipMemsetAsync(d_rows, 0, sizeof(sc_profile_shift_fit) * (size_t)m, ctx->stream));
        const unsigned grid = (unsigned)std::min<long long>((m + PF_WAVES - 1) / PF_WAVES, PF_MAX_GRID);
        sc_prof_begin(ctx, SC_K_PROFILE);
        if (tab_lds)
            k_pf_shift<true><<<grid, PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d_cells, d_dir, m, d_ages, A, h, w, D, de, delta,
                                                                     min_samples, d_tab, d_rows, d_sse, d_shift);
        else
            k_pf_shift<false><<<grid, PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d_cells, d_dir, m, d_ages, A, h, w, D, de, delta,
                                                                      min_samples, d_tab, d_rows, d_sse, d_shift);
        SC_HIP(ctx, hipGetLastError());
        sc_prof_end(ctx, 1);
        SC_HIP(ctx, hipMemcpyAsync(out_rows + k0, d_rows, sizeof(sc_profile_shift_fit) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        if (out_sse)
            SC_HIP(ctx, hipMemcpyAsync(out_sse + (size_t)k0 * A, d_sse, sizeof(double) * (size_t)A * (size_t)m,
                                       hipMemcpyDeviceToHost, ctx->stream));
        if (out_shift)
            SC_HIP(ctx, hipMemcpyAsync(out_shift + (size_t)k0 * A, d_shift, (size_t)A * (size_t)m, hipMemcpyDeviceToHost,
                                       ctx->stream));
        // (dir is reused by the next chunk, and the caller owns the outputs on return)
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SC_OK;
}

extern "C" int sc_fit_profiles_shift(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                     const double* ages, int A, int h, int w, int D, double de, double delta,
                                     int min_samples, sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (!ctx) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const Geom& g = ctx->g;
    if (g.ly != g.ny || g.lx != g.nx || g.gy0 != 0 || g.gx0 != 0 || g.cy0 != 0 || g.cx0 != 0 || g.cy1 != g.ny || g.cx1 != g.nx)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_fit_profiles_shift: the context holds a block of a larger grid");
    int rc = sc_pf_check(ctx, "sc_fit_profiles_shift", g.ny, g.nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if ((rc = sc_pf_check_shift(ctx, "sc_fit_profiles_shift", h, D, min_samples))) return rc;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    return pf_shift_run(ctx, ctx->z_dev, g.ny, g.nx, cells, sa, ca, K, ages, A, h, w, D, de, delta, min_samples, out_rows,
                        out_sse, out_shift);
}

extern "C" int sc_fit_profiles_shift_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                         const double* sa, const double* ca, long long K, const double* ages, int A, int h,
                                         int w, int D, double de, double delta, int min_samples,
                                         sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (!ctx || !z) return SC_ERR_INVALID;
    int rc = sc_pf_check(ctx, "sc_fit_profiles_shift_dem", ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if ((rc = sc_pf_check_shift(ctx, "sc_fit_profiles_shift_dem", h, D, min_samples))) return rc;
    if (K == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * (size_t)ny * (size_t)nx;
    if ((rc = sc_ensure(ctx, ctx->pf_z, bytes))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->pf_z.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    return pf_shift_run(ctx, (const double*)ctx->pf_z.p, ny, nx, cells, sa, ca, K, ages, A, h, w, D, de, delta, min_samples,
                        out_rows, out_sse, out_shift);
}
