// sc_fit_strike*: joint scarp fits in windows along the strike of a segment (docs/strike.md).
//
// A window is a contiguous range [lo, hi) of its segment's cells, which arrive sorted along the strike; the ranges are
// integers cut on the host - no float is compared here to cut a window.  The model is sc_fit_segments' on the window's
// usable profiles: a shared amplitude a and age, an intercept and a slope per profile.  With the orthogonalised terms
// stage one parks (sc_sg_stage_*, sc_segment.hip: k_sg_partial or k_sg_shift, k_sg_rank), the pooled sse at age i is
// SSpp - SSep_i^2 / SSee_i, where Spp_c - the profile's squared residuals about its own line, pf_sse with a = 0 - does
// not depend on the age: no residual pass.  After stage one
//   k_st_spp   one wave per usable cell: the parked profile 64 points at a time, lanes over the points for the squared
//              residuals, which are then added in ascending order - the bits of pf_sse with a = 0, b = beta,
//              c0 = pbar - beta sbar
//   k_st_fit   one wave per window, lanes over the ages, the windows of a workgroup consecutive stations: (SSee_i, SSep_i),
//              SSpp and the integer n over the window's usable profiles in hand-over order - runs of 64 in sequence from
//              the first, then the run sums in sequence from the first; one profile is no addition at all.
//              Q_i = SSep_i^2 / SSee_i, a butterfly argmax with the smallest index winning a tie (a NaN never wins),
//              a = SSep / SSee there; sse_i = max(SSpp - Q_i, 0); pf_walk from that age; the row and the optional curve
// No float atomics, no float sum across lanes: the same bytes on every run.
// The host side is the windows of one chunk, cut to the chunk's cells and segments, and the launches after stage one,
// handed to sc_sg_chunks (sc_segment.hip): the rows and the curves run over the windows, the call's second CSR array.
// sc_channel_strike.hip shares the checks of the window arrays, the windows of a chunk and k_st_spp (sc_strike.h).
#include "sc_strike.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(ST_THREADS) void k_st_spp(const double* __restrict__ prof_g, const int* __restrict__ used,
                                                       const double* __restrict__ scal, long long K, int h, double de,
                                                       double* __restrict__ spp) {
    __shared__ double r2[ST_WAVES][64];
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long rounds = (K + ST_WAVES - 1) / ST_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {
        const long long kc = g * ST_WAVES + wave;
        if (kc >= K || used[kc] == 0) continue;          // (per wave: nothing below waits for another wave)
        const double sbar = scal[3 * kc], pbar = scal[3 * kc + 1], b = scal[3 * kc + 2];
        const double c0 = pbar - b * sbar;
        const double* prof = prof_g + (size_t)kc * np;
        double sse = 0.0;
        for (int j0 = 0; j0 < np; j0 += 64) {
            const int jj = j0 + lane;
            const double p = jj < np ? prof[jj] : __builtin_nan("");
            const double s = (double)(jj - h) * de;
            const double res = p - (c0 + b * s);
            r2[wave][lane] = res * res;
            const unsigned long long valid = __ballot(p == p);
            // (one wave: every lane reads what the others wrote, and the next round overwrites what these lanes read)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nk = min(64, np - j0);
            for (int j = 0; j < nk; ++j)
                if ((valid >> j) & 1ull) sse += r2[wave][j];          // (the same in every lane)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (lane == 0) spp[kc] = sse;
    }
}

// win: (lo, hi, segment) of every window, cells and segments counted within the chunk; wstart: the segments' CSR array
// over the windows.  D = 0: the call without a shift, shifts null
__global__ __launch_bounds__(ST_THREADS) void k_st_fit(const int* __restrict__ win, const int* __restrict__ wstart,
                                                       const int* __restrict__ label, long long NW,
                                                       const int* __restrict__ cn, const int* __restrict__ used,
                                                       const double* __restrict__ see, const double* __restrict__ sep,
                                                       const double* __restrict__ spp,
                                                       const signed char* __restrict__ shifts,
                                                       const double* __restrict__ ages, int A, int D, double delta,
                                                       int min_profiles, sc_strike_fit* __restrict__ rows,
                                                       double* __restrict__ curve) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const long long rounds = (NW + ST_WAVES - 1) / ST_WAVES;
    for (long long r = blockIdx.x; r < rounds; r += gridDim.x) {
        const long long g = r * ST_WAVES + wave;
        if (g >= NW) continue;                           // (per wave: no barrier in this kernel)
        const int lo = win[3 * g], hi = win[3 * g + 1], s = win[3 * g + 2];
        double tS = 0.0, tP = 0.0, tQ = 0.0, rS = 0.0, rP = 0.0, rQ = 0.0;
        int nr = 0, m = 0, n = 0;
        bool first = true;
        for (int k = lo; k < hi; ++k) {
            if (used[k] == 0) continue;                  // (the same in every lane)
            const size_t o = (size_t)k * A + ia;
            const double vS = see[o], vP = sep[o], vQ = spp[k];
            ++m;
            n += cn[k];
            if (nr == 0) { rS = vS; rP = vP; rQ = vQ; } else { rS += vS; rP += vP; rQ += vQ; }
            if (++nr == ST_RUN) {
                if (first) { tS = rS; tP = rP; tQ = rQ; first = false; } else { tS += rS; tP += rP; tQ += rQ; }
                nr = 0;
            }
        }
        if (nr) {
            if (first) { tS = rS; tP = rP; tQ = rQ; } else { tS += rS; tP += rP; tQ += rQ; }
        }
        const int dof = sg_dof(m, n, D);
        bool fitted = sg_fitted(m, dof, min_profiles);
        int best = -1;
        double sse = nan, a = nan;
        if (fitted) {
            // not fitted either: a sum of See that is 0 or not finite at any age
            const bool bad = lane < A && !(tS > 0.0 && tS < INFINITY);
            const double Q = tP * tP / tS;
            double q = Q;
            if (lane >= A || q != q) q = -INFINITY;      // (a NaN never wins)
            int qi = lane;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double oq = __shfl_xor(q, o, 64);
                const int oi = __shfl_xor(qi, o, 64);
                if (oq > q || (oq == q && oi < qi)) { q = oq; qi = oi; }
            }
            // (no age with a number for Q: not fitted)
            fitted = __ballot(bad) == 0ull && q > -INFINITY;
            if (fitted) {
                best = qi;
                a = tP / tS;
                const double d = tQ - Q;
                sse = d < 0.0 ? 0.0 : d;                 // (a NaN stays one)
            }
        }
        pf_pick k = {-1, -1, -1, nan};
        int status = 1;
        double a_best = nan, sse_best = nan;
        if (fitted) {
            a_best = __shfl(a, best, 64);
            sse_best = __shfl(sse, best, 64);
            k = pf_walk(sse, lane, A, best, sse_best, delta, dof);
            // a usable profile of the window whose shift at the best age sits at the end of the range
            bool at_end = false;
            if (shifts && D > 0)
                for (int c = lo + lane; c < hi; c += 64) {
                    const int d = shifts[(size_t)c * A + best];
                    at_end = at_end || (used[c] != 0 && (d == D || d == -D));
                }
            status = pf_open(k, A) + (__ballot(at_end) != 0ull ? 8 : 0);
        }
        if (curve && lane < A) curve[(size_t)g * A + lane] = sse;
        if (lane == 0) {
            // (the rows were cleared)
            sc_strike_fit* out = rows + g;
            out->label = label[s];
            out->station = (int)(g - wstart[s]);
            out->n_cells = hi - lo;
            out->n_profiles = m;
            out->n = n;
            out->dof = dof;
            out->kt_index = k.best;
            out->lo_index = k.lo;
            out->hi_index = k.hi;
            out->status = status;
            out->kt = fitted ? ages[k.best] : nan;
            out->kt_lo = fitted ? ages[k.lo] : nan;
            out->kt_hi = fitted ? ages[k.hi] : nan;
            out->a = a_best;
            out->sse = sse_best;
            out->rmse = fitted ? sqrt(sse_best / (double)dof) : nan;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int sc_st_check(sc_ctx* ctx, const char* who, const long long* seg_start, long long S, const long long* seg_win_start,
                const long long* win_lo, const long long* win_hi, long long NW, const void* out_rows) {
    if (!seg_win_start || (NW > 0 && (!win_lo || !win_hi || !out_rows)))
        return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (NW < 0 || NW > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_INVALID, "%s: NW must lie in 0..2^31 - 1", who);
    if (seg_win_start[0] != 0 || seg_win_start[S] != NW)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_win_start must run from 0 to NW", who);
    for (long long s = 0; s < S; ++s)
        if (seg_win_start[s + 1] < seg_win_start[s] || seg_win_start[s + 1] > NW)
            return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_win_start decreases or leaves 0..NW at segment %lld", who, s);
    for (long long s = 0; s < S; ++s)
        for (long long g = seg_win_start[s]; g < seg_win_start[s + 1]; ++g)
            if (!(seg_start[s] <= win_lo[g] && win_lo[g] <= win_hi[g] && win_hi[g] <= seg_start[s + 1]))
                return sc_fail(ctx, SC_ERR_INVALID, "%s: window %lld does not lie in the cells of segment %lld", who, g, s);
    return SC_OK;
}

// the windows of one chunk, cut to the chunk's cells and segments, on their way up (sc_strike.h)
int sc_st_windows(sc_ctx* ctx, const sg_chunk& k, const long long* seg_win_start, const long long* win_lo,
                  const long long* win_hi, bool spp, st_windows& w) {
    const long long Sc = k.st.Sc, g0 = seg_win_start[k.s0];
    const long long NWc = seg_win_start[k.s1] - g0;
    int rc;
    w.NWc = NWc;
    w.win.resize(3 * (size_t)NWc);
    w.wstart.resize((size_t)Sc + 1);
    for (long long s = 0; s <= Sc; ++s) w.wstart[s] = (int)(seg_win_start[k.s0 + s] - g0);
    for (long long s = 0; s < Sc; ++s)
        for (long long g = w.wstart[s]; g < w.wstart[s + 1]; ++g) {
            w.win[3 * g] = (int)(win_lo[g0 + g] - k.k0);
            w.win[3 * g + 1] = (int)(win_hi[g0 + g] - k.k0);
            w.win[3 * g + 2] = (int)s;
        }
    if ((rc = sc_ensure(ctx, ctx->st_win, sizeof(int) * 3 * (size_t)NWc))) return rc;
    if ((rc = sc_ensure(ctx, ctx->st_wstart, sizeof(int) * ((size_t)Sc + 1)))) return rc;
    if (spp && (rc = sc_ensure(ctx, ctx->st_spp, sizeof(double) * (size_t)k.st.m))) return rc;
    w.d_win = (int*)ctx->st_win.p;
    w.d_wstart = (int*)ctx->st_wstart.p;
    w.d_spp = spp ? (double*)ctx->st_spp.p : nullptr;
    if (NWc) SC_HIP(ctx, hipMemcpyAsync(w.d_win, w.win.data(), sizeof(int) * 3 * (size_t)NWc, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(w.d_wstart, w.wstart.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
    return SC_OK;
}

void sc_st_spp_launch(sc_ctx* ctx, const sg_stage& st, int h, double de, double* d_spp) {
    k_st_spp<<<st_grid(st.m), ST_THREADS, 0, ctx->stream>>>(st.prof, st.used, st.scal, st.m, h, de, d_spp);
}

static int st_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                  const long long* win_lo, const long long* win_hi, const double* ages, int A, int h, int w, int D, double de,
                  double delta, int min_samples, int min_profiles, sc_strike_fit* out_rows, double* out_sse) {
    if (S == 0) return SC_OK;
    const int Ds = D > 0 ? D : -1;                       // D = 0 is the call without a shift: its kernel, its park
    const int ht = h + (D > 0 ? D : 0);
    int rc;
    if ((rc = sc_sg_stage_attr(ctx, A, h, Ds))) return rc;

    // (a chunk holds as many whole segments as fit the parked bytes and the windows' outputs)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, ht, de, sg_park_plain(A, h, Ds >= 0), ST_MAX_SEGS, seg_win_start,
                 ST_MAX_WIN, 0};
    c.out = {{out_rows, &ctx->st_rows, sizeof(sc_strike_fit), SG_AUX, true}, {out_sse, &ctx->st_sse, sizeof(double) * A, SG_AUX}};
    st_windows W;
    c.prepare = [&](const sg_chunk& k) { return sc_st_windows(ctx, k, seg_win_start, win_lo, win_hi, true, W); };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mA = (size_t)st.m * A;
        int launches = sc_sg_stage_launch(ctx, z, ny, nx, A, h, w, Ds, de, min_samples, k.tab, st);
        if (st.m && W.NWc) {
            sc_st_spp_launch(ctx, st, h, de, W.d_spp);
            ++launches;
        }
        if (W.NWc) {
            k_st_fit<<<st_grid(W.NWc), ST_THREADS, 0, ctx->stream>>>(W.d_win, W.d_wstart, st.label, W.NWc, st.cn, st.used,
                                                                    st.planes + 2 * mA, st.planes + 3 * mA, W.d_spp, st.shift,
                                                                    k.ages, A, D, delta, min_profiles, (sc_strike_fit*)k.out[0],
                                                                    (double*)k.out[1]);
            ++launches;
        }
        return launches;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal, then the fit on the context's DEM (z null) or on z, uploaded
static int st_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                   const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                   sc_strike_fit* out_rows, double* out_sse) {
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    // (the park of a shifted call counts d_ci whatever D is: the limit of sc_fit_segments_shift)
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, D, de, delta, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_st_check(ctx, who, seg_start, S, seg_win_start, win_lo, win_hi, NW, out_rows))) return rc;
    if (z && (S == 0 || NW == 0)) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    if (NW == 0) return SC_OK;
    return st_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_win_start, win_lo, win_hi, ages, A, h, w, D,
                  de, delta, min_samples, min_profiles, out_rows, out_sse);
}

extern "C" int sc_fit_strike(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                             const long long* seg_start, const int32_t* seg_label, long long S,
                             const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                             const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples,
                             int min_profiles, sc_strike_fit* out_rows, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_strike");
    if (rc) return rc;
    return st_call(ctx, "sc_fit_strike", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                   seg_win_start, win_lo, win_hi, NW, ages, A, h, w, D, de, delta, min_samples, min_profiles, out_rows, out_sse);
}

extern "C" int sc_fit_strike_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                 const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                 long long S, const long long* seg_win_start, const long long* win_lo,
                                 const long long* win_hi, long long NW, const double* ages, int A, int h, int w, int D,
                                 double de, double delta, int min_samples, int min_profiles, sc_strike_fit* out_rows,
                                 double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return st_call(ctx, "sc_fit_strike_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_win_start, win_lo,
                   win_hi, NW, ages, A, h, w, D, de, delta, min_samples, min_profiles, out_rows, out_sse);
}
