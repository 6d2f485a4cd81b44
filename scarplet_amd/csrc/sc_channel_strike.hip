// sc_channel_strike*: a channel's width in windows along the strike of a reach (docs/channels.md, "Width along a reach").
//
// What sc_fit_strike (sc_strike.hip) is to sc_fit_segments_shift, for sc_channel_segments: a window is a contiguous range
// [lo, hi) of its reach's cells, which arrive sorted along the strike; the ranges are integers cut on the host - no float
// is compared here to cut a window.  Stage one is sc_channel_segments' own (sc_cs_stage_launch, sc_channel_segment.hip:
// k_cs_stage, k_sg_rank): every usable profile c keeps at every frequency i its own shift d_ci, which is not re-fitted
// per window, and what the mode sums
//   SC_CHANNEL_DEPTH_PROFILE  (sse*_ci, a_ci): sse_i = SSse_i, f_index = argmin, a = SA / n_profiles there.  No subtraction
//   SC_CHANNEL_DEPTH_SEGMENT  (See_ci, Sep_ci) and Spp_c (k_st_spp, sc_strike.hip, on the parked profiles): frequency i is
//                             live when SSee_i > 0 and finite and Q_i = SSep_i^2 / SSee_i is a number; f_index = argmax
//                             Q_i over the live ones, a = SSep / SSee there, sse_i = max(SSpp - Q_i, 0)
//   k_cw_fit   one wave per window, lanes over the frequencies, the windows of a workgroup consecutive stations: the sums
//              and the integers n and n_profiles over the window's usable profiles in hand-over order - runs of 64 in
//              sequence from the first, then the run sums in sequence from the first; one profile is no addition at all.
//              NaN propagates: a frequency that is dead in one usable profile of the window is dead for the window.  A
//              butterfly choice with the smallest index winning a tie (a dead frequency never wins), pf_walk from it; then
//              lanes over the window's cells for status bit 8 and the integer sum of d_ci at the best frequency; the
//              row and the optional curve
// No atomics, no float sum across lanes: the same bytes on every run.  The host side is st_run's (sc_strike.hip): the
// windows of one chunk and the launches after stage one, handed to sc_sg_chunks with the windows as the second CSR array.
#include "sc_channel.h"
#include "sc_strike.h"
#include <math.h>
#include <algorithm>

// win: (lo, hi, reach) of every window, cells and reaches counted within the chunk; wstart: the reaches' CSR array over
// the windows.  x, y: the two planes the mode sums - (sse*, a) or (See, Sep); spp: Spp of every cell, segment mode
__global__ __launch_bounds__(ST_THREADS) void k_cw_fit(const int* __restrict__ win, const int* __restrict__ wstart,
                                                       const int* __restrict__ label, long long NW,
                                                       const int* __restrict__ cn, const int* __restrict__ used,
                                                       const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ spp,
                                                       const signed char* __restrict__ shifts,
                                                       const double* __restrict__ freqs, int F, int D, double delta,
                                                       int min_profiles, int mode, sc_strike_fit* __restrict__ rows,
                                                       double* __restrict__ curve, int* __restrict__ shift_sum) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ia = min(lane, F - 1);                     // lanes beyond the frequencies repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;   // (the same in every wave of the launch)
    const long long rounds = (NW + ST_WAVES - 1) / ST_WAVES;
    for (long long r = blockIdx.x; r < rounds; r += gridDim.x) {
        const long long g = r * ST_WAVES + wave;
        if (g >= NW) continue;                           // (per wave: no barrier in this kernel)
        const int lo = win[3 * g], hi = win[3 * g + 1], s = win[3 * g + 2];
        double tX = 0.0, tY = 0.0, tQ = 0.0, rX = 0.0, rY = 0.0, rQ = 0.0;
        int nr = 0, m = 0, n = 0;
        bool first = true;
        for (int k = lo; k < hi; ++k) {
            if (used[k] == 0) continue;                  // (the same in every lane)
            const size_t o = (size_t)k * F + ia;
            const double vX = x[o], vY = y[o], vQ = own ? 0.0 : spp[k];
            ++m;
            n += cn[k];
            if (nr == 0) { rX = vX; rY = vY; rQ = vQ; } else { rX += vX; rY += vY; rQ += vQ; }
            if (++nr == ST_RUN) {
                if (first) { tX = rX; tY = rY; tQ = rQ; first = false; } else { tX += rX; tY += rY; tQ += rQ; }
                nr = 0;
            }
        }
        if (nr) {
            if (first) { tX = rX; tY = rY; tQ = rQ; } else { tX += rX; tY += rY; tQ += rQ; }
        }
        const int dof = cs_dof(mode, m, n, D);
        const bool fitted = sg_fitted(m, dof, min_profiles);
        pf_pick k = {-1, -1, -1, nan};
        int status = 1, dsum = 0;
        double a = nan, sse = nan, sse_best = nan;
        if (fitted) {
            bool live;
            if (own) {
                sse = tX;
                a = tY / (double)m;
                live = lane < F && sse == sse;
            } else {
                const double Q = tY * tY / tX;
                live = lane < F && tX > 0.0 && tX < INFINITY && Q == Q;
                a = tY / tX;
                const double d = tQ - Q;
                sse = live ? (d < 0.0 ? 0.0 : d) : nan;  // (a NaN of SSpp stays one)
                // the argmax of Q over the live frequencies, the smallest index winning a tie
                double q = live ? Q : -INFINITY;
                int qi = lane;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double oq = __shfl_xor(q, o, 64);
                    const int oi = __shfl_xor(qi, o, 64);
                    if (oq > q || (oq == q && oi < qi)) { q = oq; qi = oi; }
                }
                k.best = qi;
            }
            if (!__ballot(live)) {
                status = 1 | 32;                         // every frequency is dead
                k.best = -1;
                a = nan;
                sse = nan;
            } else {
                if (own) {
                    k = pf_choose(sse, lane, F, delta, dof);
                    sse_best = k.sse_min;
                } else {
                    sse_best = __shfl(sse, k.best, 64);
                    k = pf_walk(sse, lane, F, k.best, sse_best, delta, dof);
                }
                a = __shfl(a, k.best, 64);
                // the window's usable profiles at the best frequency: a shift at the end of its range, and the sum of the shifts
                bool at_end = false;
                if (D > 0) {
                    for (int c = lo + lane; c < hi; c += 64) {
                        if (used[c] == 0) continue;
                        const int d = shifts[(size_t)c * F + k.best];
                        at_end = at_end || d == D || d == -D;
                        dsum += d;
                    }
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) dsum += __shfl_xor(dsum, o, 64);          // (integers: exact in any order)
                }
                status = pf_open(k, F) + (__ballot(at_end) != 0ull ? 8 : 0);
            }
        }
        const bool alive = k.best >= 0;
        if (curve && lane < F) curve[(size_t)g * F + lane] = sse;
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
            out->kt = alive ? freqs[k.best] : nan;
            out->kt_lo = alive ? freqs[k.lo] : nan;
            out->kt_hi = alive ? freqs[k.hi] : nan;
            out->a = alive ? a : nan;
            out->sse = sse_best;
            out->rmse = alive ? sqrt(sse_best / (double)dof) : nan;
            if (shift_sum) shift_sum[g] = dsum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int cw_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                  const long long* win_lo, const long long* win_hi, const double* freqs, int F, int h, int w, int D, int mode,
                  double de, double delta, int min_samples, int min_profiles, sc_strike_fit* out_rows, double* out_sse,
                  int32_t* out_shift_sum) {
    if (S == 0) return SC_OK;
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;
    cs_stage_plan plan;
    int rc;
    if ((rc = sc_cs_stage_attr(ctx, F, h, D, &plan))) return rc;

    // (a chunk holds as many whole reaches as fit the parked bytes - SC_CHANNEL_SEGMENT_PARK a cell - and the windows' outputs)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, freqs, F, h + D, de, sg_park_plain(F, h, true), ST_MAX_SEGS, seg_win_start,
                 ST_MAX_WIN, 0};
    c.out = {{out_rows, &ctx->st_rows, sizeof(sc_strike_fit), SG_AUX, true},
             {out_sse, &ctx->st_sse, sizeof(double) * F, SG_AUX},
             {out_shift_sum, &ctx->cw_shift, sizeof(int32_t), SG_AUX}};
    const double* d_terms = nullptr;
    // (the frame's table over h + D has the size of G, which takes its place: k.tab is G from here on)
    c.tables = [&](const double* d_freqs) { return sc_ch_tables(ctx, d_freqs, F, h, D, de, (double*)ctx->sg_tab.p, &d_terms); };
    st_windows W;
    c.prepare = [&](const sg_chunk& k) { return sc_st_windows(ctx, k, seg_win_start, win_lo, win_hi, !own, W); };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mF = (size_t)st.m * F;
        // (segment mode parks the profiles: Spp is formed on them)
        int launches = sc_cs_stage_launch(ctx, plan, z, ny, nx, F, h, w, D, de, min_samples, mode, k.tab, d_terms, !own, st);
        if (!own && st.m && W.NWc) {
            sc_st_spp_launch(ctx, st, h, de, W.d_spp);
            ++launches;
        }
        if (W.NWc) {
            const double* x = own ? st.planes : st.planes + 2 * mF;
            k_cw_fit<<<st_grid(W.NWc), ST_THREADS, 0, ctx->stream>>>(W.d_win, W.d_wstart, st.label, W.NWc, st.cn, st.used, x, x + mF,
                                                                    W.d_spp, st.shift, k.ages, F, D, delta, min_profiles, mode,
                                                                    (sc_strike_fit*)k.out[0], (double*)k.out[1], (int*)k.out[2]);
            ++launches;
        }
        return launches;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal - sc_channel_segments', then sc_fit_strike's of the window arrays -,
// then the fit on the context's DEM (z null) or on z, uploaded
static int cw_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                   const double* freqs, int F, int h, int w, int D, int mode, double de, double delta, int min_samples,
                   int min_profiles, sc_strike_fit* out_rows, double* out_sse, int32_t* out_shift_sum) {
    int rc = sc_cs_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, freqs, F, h, w, D, mode, de, delta,
                         min_samples, min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_st_check(ctx, who, seg_start, S, seg_win_start, win_lo, win_hi, NW, out_rows))) return rc;
    if (z && (S == 0 || NW == 0)) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    if (NW == 0) return SC_OK;
    return cw_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_win_start, win_lo, win_hi, freqs, F, h, w, D,
                  mode, de, delta, min_samples, min_profiles, out_rows, out_sse, out_shift_sum);
}

extern "C" int sc_channel_strike(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                 const long long* seg_start, const int32_t* seg_label, long long S,
                                 const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                                 const double* frequencies, int F, int h, int w, int D, int mode, double de, double delta,
                                 int min_samples, int min_profiles, sc_strike_fit* out_rows, double* out_sse,
                                 int32_t* out_shift_sum) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_channel_strike");
    if (rc) return rc;
    return cw_call(ctx, "sc_channel_strike", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                   seg_win_start, win_lo, win_hi, NW, frequencies, F, h, w, D, mode, de, delta, min_samples, min_profiles, out_rows,
                   out_sse, out_shift_sum);
}

extern "C" int sc_channel_strike_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                     const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                     long long S, const long long* seg_win_start, const long long* win_lo,
                                     const long long* win_hi, long long NW, const double* frequencies, int F, int h, int w,
                                     int D, int mode, double de, double delta, int min_samples, int min_profiles,
                                     sc_strike_fit* out_rows, double* out_sse, int32_t* out_shift_sum) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return cw_call(ctx, "sc_channel_strike_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_win_start, win_lo,
                   win_hi, NW, frequencies, F, h, w, D, mode, de, delta, min_samples, min_profiles, out_rows, out_sse,
                   out_shift_sum);
}
