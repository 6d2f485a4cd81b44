// sc_channel_strike_bootstrap*: block-bootstrap intervals of a channel's width, depth and area at every station along the
// strike of a reach (docs/channels.md, "Intervals per station").
//
// What sc_strike_bootstrap (sc_strike_bootstrap.hip) is to sc_fit_strike, for sc_channel_strike: hand-over, stations and
// windows are sc_channel_strike's, the blocks of a window are cut on the host and arrive as integers (win_blk_start, blk_hi:
// sc_strike_bootstrap's arrays) - no float is compared here.  Stage one is sc_channel_segments' own (sc_cs_stage_launch,
// sc_channel_segment.hip: k_cs_stage, k_sg_rank): every usable profile keeps at every frequency its own shift d_ci, which is
// not re-fitted per window or per replicate.  There is no residual pass and no Spp in either mode: a replicate is
// sc_channel_bootstrap's (sc_channel_bootstrap.hip),
//   SC_CHANNEL_DEPTH_SEGMENT  the argmax of Q_i = SSep_i^2 / SSee_i over the drawn blocks' sums, a = SSep / SSee there
//   SC_CHANNEL_DEPTH_PROFILE  the argmin of SSse_i, a = SA_i / M there, M the usable profiles drawn, with multiplicity
// and a frequency that is dead in a drawn profile (NaN terms) is dead for that replicate only.  Then one kernel, a workgroup
// per window:
//   k_cwb_window  1. block terms: waves over the window's blocks, lanes over the frequencies: (sum See_ci, sum Sep_ci) or
//                    (sum sse*_ci, sum a_ci) over the block's usable profiles in hand-over order - runs of 64 in sequence
//                    from the first, then the run sums in sequence from the first - into LDS, with m_b, the block's usable
//                    profiles, in profile mode; a block without a usable profile keeps (0, 0) and m_b = 0; n_profiles
//                    counted in integers
//                 2. replicates: waves over the replicates 0..R, replicate 0 every block once; the draws of the others are
//                    sc_strike_bootstrap's - keyed by seed, label and station, formed 64 at a time, one per lane, and read
//                    back lane by lane into scalar registers (bs_sums_counted, sc_bootstrap.h) -, the sums in draw order
//                    from LDS, M in integers; k_cb_reps' butterfly argmin on (key, index) - key = -Q or SSse, +inf and
//                    64 + lane where the frequency is not live - with the smallest index winning a tie; (index int8, a)
//                    of every replicate stays in LDS in replicate order
//                 3. summary: an integer histogram of the indices in LDS, the ranks walked along it by one thread, a_mean
//                    and a_sd summed in replicate order by one thread, a copy of the a sorted bitonically in a second
//                    array, padded to a power of two, for a_lo and a_hi; that array filled again with the areas -a_r /
//                    (sqrt(pi) f[index_r]) from the unsorted (index, a), their mean and sd in replicate order, and sorted
//                    again; the row and the optional histogram
// Per-replicate outputs are not built: they would be NW x (R + 1) values.
// No float atomics, no float sum across lanes: the same bytes on every run, for every "fit_chunk", and whatever other
// reaches the call holds.
// The host side is sb_run's (sc_strike_bootstrap.hip): the windows and the blocks of one chunk (sc_sb_windows, sc_strike.h)
// and the launch after stage one, handed to sc_sg_chunks (sc_segment.hip) with the windows as the second CSR array.
#include "sc_bootstrap.h"
#include "sc_channel.h"
#include "sc_strike.h"
#include <math.h>
#include <algorithm>

#define CWB_WAVES 4                      // 256 threads: at R = 1000 and ten blocks of 35 frequencies 23 KB of LDS a workgroup,
#define CWB_THREADS (64 * CWB_WAVES)     // seven workgroups a CU, by LDS and - 71 VGPRs - by registers alike
#define CWB_LDS_TERMS 65536              // a window's block terms must fit this many bytes
#define CWB_MAX_GRID 65536
#define CWB_MAX_SEGS (1ll << 20)
#define CWB_MAX_WIN (1ll << 21)          // windows of a chunk

// Dynamic LDS of a window of up to nb blocks: the block terms, the a of replicates 1..R and the array that is sorted, both
// padded to the sort, m_b in profile mode, the indices.  The ONE place where the bound is computed; at the top of the
// accepted range - 64 KiB of terms at F = 1, R = 4096, profile mode - 148 KiB of gfx950's 160
static size_t cwb_lds_bytes(int nb, int F, int R, bool own) {
    return sizeof(double2) * (size_t)nb * F + (2 * sizeof(double) + 1) * (size_t)sb_sort_len(R) + (own ? sizeof(int) * (size_t)nb : 0);
}

// the bitonic sort of v[0..P2) ascending by the whole workgroup (+inf sorts behind every number)
__device__ __forceinline__ void cwb_sort(double* v, int P2, int tid) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += CWB_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const double x = v[i], y = v[p];
                    if ((x > y) == ((i & k) == 0)) { v[i] = y; v[p] = x; }
                }
            }
            __syncthreads();
        }
}

// the mean and the sd of the valid replicates' values in replicate order (one thread); n_ok >= 1 of them
__device__ __forceinline__ void cwb_moments(const double* v, const signed char* idx, int R, int n_ok, double& mean, double& sd) {
    double sum = 0.0;
    for (int r = 0; r < R; ++r)
        if (idx[r] >= 0) sum += v[r];
    mean = sum / (double)n_ok;
    if (n_ok > 1) {
        double ss = 0.0;
        for (int r = 0; r < R; ++r)
            if (idx[r] >= 0) {
                const double d = v[r] - mean;
                ss += d * d;
            }
        sd = sqrt(ss / (double)(n_ok - 1));
    }
}

// win: (lo, hi, reach) of every window, cells and reaches counted within the chunk; wstart: the reaches' CSR array over the
// windows; wblk: the windows' CSR array over the blocks; bhi: the end cell of every block, within the chunk.  x, y: the two
// planes the mode sums - (sse*, a) or (See, Sep).  nb_lds: the blocks the launch's LDS holds - no window of the chunk has
// more; rpi: sqrt(pi), the host's
template <bool OWN>
__global__ __launch_bounds__(CWB_THREADS) void k_cwb_window(const int* __restrict__ win, const int* __restrict__ wstart,
                                                            const int* __restrict__ wblk, const int* __restrict__ bhi,
                                                            const int* __restrict__ label, long long NW,
                                                            const int* __restrict__ used, const double* __restrict__ x,
                                                            const double* __restrict__ y, const double* __restrict__ freqs,
                                                            int F, int R, double level, double rpi, unsigned long long seed,
                                                            int min_blocks, int min_profiles, int nb_lds,
                                                            sc_channel_strike_boot* __restrict__ rows,
                                                            int* __restrict__ out_hist) {
    extern __shared__ double2 cwb_lds[];
    __shared__ int hist[64];
    __shared__ int cnt[CWB_WAVES];
    __shared__ int idx0;
    __shared__ double amp0;
    const int P2 = sb_sort_len(R);
    double2* T = cwb_lds;
    double* v = (double*)(cwb_lds + (size_t)nb_lds * F);                // the a of replicates 1..R, in replicate order
    double* u = v + P2;                                                  // what is sorted: the a, then the areas
    int* mb = (int*)(u + P2);                                            // (profile mode)
    signed char* idx = (signed char*)(mb + (OWN ? nb_lds : 0));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ia = min(lane, F - 1);                     // lanes beyond the frequencies repeat the last one and are ignored
    const double nan = __builtin_nan("");
    for (long long g = blockIdx.x; g < NW; g += gridDim.x) {          // (uniform per workgroup: the barriers below)
        const int lo = win[3 * g], hi = win[3 * g + 1], s = win[3 * g + 2];
        const int b0 = wblk[g], nb = min(wblk[g + 1] - b0, nb_lds);   // (the host refused a window of more)
        const int station = (int)(g - wstart[s]);
        __syncthreads();                                 // (the window before is written)
        // 1. the block terms
        int m_wave = 0;
        for (int b = wave; b < nb; b += CWB_WAVES) {
            const int k0 = b == 0 ? lo : bhi[b0 + b - 1], k1 = bhi[b0 + b];
            double tX = 0.0, tY = 0.0, rX = 0.0, rY = 0.0;
            int nr = 0, m = 0;
            bool first = true;
            for (int k = k0; k < k1; ++k) {
                if (used[k] == 0) continue;              // (the same in every lane)
                const size_t o = (size_t)k * F + ia;
                const double vX = x[o], vY = y[o];
                ++m;
                if (nr == 0) { rX = vX; rY = vY; } else { rX += vX; rY += vY; }
                if (++nr == BS_RUN) {
                    if (first) { tX = rX; tY = rY; first = false; } else { tX += rX; tY += rY; }
                    nr = 0;
                }
            }
            if (nr) {
                if (first) { tX = rX; tY = rY; } else { tX += rX; tY += rY; }
            }
            if (lane < F) T[b * F + lane] = make_double2(tX, tY);
            if (OWN && lane == 0) mb[b] = m;
            m_wave += m;
        }
        if (lane == 0) cnt[wave] = m_wave;
        if (tid < 64) hist[tid] = 0;
        __syncthreads();
        int m = 0;
        for (int i = 0; i < CWB_WAVES; ++i) m += cnt[i];
        const bool boot = bs_boot(nb, m, min_blocks, min_profiles);
        // 2. the replicates (boot is the workgroup's: every lane of every wave reaches the butterfly)
        for (int i = tid; i < P2; i += CWB_THREADS) {    // what no replicate writes: failed, or the padding of the sort
            v[i] = INFINITY;
            idx[i] = -1;
        }
        if (tid == 0) {
            idx0 = -1;
            amp0 = nan;
        }
        __syncthreads();
        if (boot) {
            const unsigned long long key = sb_mix(seed ^ ((unsigned long long)(unsigned)label[s] * 0x9E3779B97F4A7C15ull) ^
                                                  ((unsigned long long)(unsigned)station * 0xD1B54A32D192ED03ull));
            for (int r = wave; r <= R; r += CWB_WAVES) {
                double X, Y;
                int M;
                bs_sums_counted<OWN>(T, mb, nb, F, ia, lane, r, key, X, Y, M);
                // the smallest key among the live frequencies: SSse, or -Q for the largest Q
                double q, a;
                bool live;
                if (OWN) {
                    q = X;
                    a = Y / (double)M;
                    live = M > 0 && X == X;
                } else {
                    const double Q = Y * Y / X;
                    q = -Q;
                    a = Y / X;
                    live = X > 0.0 && X < INFINITY && Q == Q;
                }
                live = live && lane < F;
                if (!live) q = INFINITY;
                int qi = live ? lane : 64 + lane;        // (a live +inf still beats a frequency that is not)
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double oq = __shfl_xor(q, o, 64);
                    const int oi = __shfl_xor(qi, o, 64);
                    if (oq < q || (oq == q && oi < qi)) { q = oq; qi = oi; }
                }
                if (qi < 64) {                           // (no live frequency: failed)
                    a = __shfl(a, qi, 64);
                    if (lane == 0) {
                        if (r == 0) {
                            idx0 = qi;
                            amp0 = a;
                        } else {
                            idx[r - 1] = (signed char)qi;
                            v[r - 1] = a;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // 3. the summary
        for (int i = tid; i < R; i += CWB_THREADS) {
            const int k = idx[i];
            if (k >= 0) atomicAdd(&hist[k], 1);          // (integers: any order)
        }
        for (int i = tid; i < P2; i += CWB_THREADS) u[i] = v[i];
        __syncthreads();
        if (out_hist && tid < F) out_hist[(size_t)g * F + tid] = hist[tid];
        double mean[2] = {nan, nan}, sd[2] = {nan, nan}, vlo[2] = {nan, nan}, vhi[2] = {nan, nan};          // (thread 0's)
        int n_ok = 0, ilo = -1, ihi = -1, klo = 0, khi = 0;
        if (tid == 0) {
            for (int i = 0; i < F; ++i) n_ok += hist[i];
            if (n_ok > 0) {
                const double q = (1.0 - level) / 2.0;
                klo = min(max((int)floor(q * (double)n_ok), 0), n_ok - 1);
                khi = min(max((int)ceil((1.0 - q) * (double)n_ok) - 1, 0), n_ok - 1);
                int c = 0;
                for (int i = 0; i < F; ++i) {            // x[k] = the first index whose cumulative count passes k
                    c += hist[i];
                    if (ilo < 0 && c > klo) ilo = i;
                    if (ihi < 0 && c > khi) ihi = i;
                }
                cwb_moments(v, idx, R, n_ok, mean[0], sd[0]);
            }
        }
        // the a of the valid replicates ascending, the others (+inf) behind them
        cwb_sort(u, P2, tid);
        if (tid == 0 && n_ok > 0) {
            vlo[0] = u[klo];
            vhi[0] = u[khi];
        }
        __syncthreads();                                 // (thread 0 has read the ranks of the a)
        for (int i = tid; i < P2; i += CWB_THREADS) {
            const int k = idx[i];
            u[i] = k >= 0 ? -v[i] / (rpi * freqs[k]) : INFINITY;
        }
        __syncthreads();
        if (tid == 0 && n_ok > 0) cwb_moments(u, idx, R, n_ok, mean[1], sd[1]);
        __syncthreads();
        cwb_sort(u, P2, tid);
        if (tid == 0) {
            // (the rows were cleared)
            sc_channel_strike_boot* out = rows + g;
            const bool done = boot && n_ok > 0;
            const int r0 = boot ? idx0 : -1;
            const int i0 = done ? r0 : -1;
            const double a0 = i0 >= 0 ? amp0 : nan;
            out->label = label[s];
            out->station = station;
            out->n_cells = hi - lo;
            out->n_profiles = m;
            out->n_blocks = nb;
            out->replicates = R;
            out->n_failed = boot ? R - n_ok : 0;
            out->f_index0 = i0;
            out->lo_index = done ? ilo : -1;
            out->hi_index = done ? ihi : -1;
            out->status = done ? (ilo == 0 ? 2 : 0) + (ihi == F - 1 ? 4 : 0) : (boot && r0 < 0 ? 1 | 32 : 1);
            out->f0 = i0 >= 0 ? freqs[i0] : nan;
            out->f_lo = done ? freqs[ilo] : nan;
            out->f_hi = done ? freqs[ihi] : nan;
            out->a0 = a0;
            out->a_mean = done ? mean[0] : nan;
            out->a_sd = done ? sd[0] : nan;
            out->a_lo = done ? vlo[0] : nan;
            out->a_hi = done ? vhi[0] : nan;
            out->area0 = i0 >= 0 ? -a0 / (rpi * freqs[i0]) : nan;
            out->area_mean = done ? mean[1] : nan;
            out->area_sd = done ? sd[1] : nan;
            out->area_lo = done ? u[klo] : nan;
            out->area_hi = done ? u[khi] : nan;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int cwb_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                   const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                   const long long* win_lo, const long long* win_hi, long long NW, const long long* win_blk_start,
                   const long long* blk_hi, const double* freqs, int F, int h, int w, int D, int mode, double de,
                   int min_samples, int min_profiles, int min_blocks, int R, double level, unsigned long long seed,
                   sc_channel_strike_boot* out_rows, int32_t* out_hist) {
    if (S == 0) return SC_OK;
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;
    const double rpi = sqrt(M_PI);
    const auto k_window = own ? k_cwb_window<true> : k_cwb_window<false>;
    cs_stage_plan plan;
    int rc;
    if ((rc = sc_cs_stage_attr(ctx, F, h, D, &plan))) return rc;
    // the dynamic LDS of the call's largest window, raised once
    long long nb_call = 0;
    for (long long g = 0; g < NW; ++g) nb_call = std::max(nb_call, win_blk_start[g + 1] - win_blk_start[g]);
    if ((rc = sc_lds_attr(ctx, (const void*)k_window, cwb_lds_bytes((int)nb_call, F, R, own)))) return rc;

    // (a chunk holds as many whole reaches as fit the parked bytes - SC_CHANNEL_SEGMENT_PARK a cell - and the windows' outputs)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, freqs, F, h + D, de, sg_park_plain(F, h, true), CWB_MAX_SEGS, seg_win_start,
                 CWB_MAX_WIN, 0};
    c.out = {{out_rows, &ctx->sb_rows, sizeof(sc_channel_strike_boot), SG_AUX, true},
             {out_hist, &ctx->sb_hist, sizeof(int) * F, SG_AUX}};
    const double* d_terms = nullptr;
    // (the frame's table over h + D has the size of G, which takes its place: k.tab is G from here on)
    c.tables = [&](const double* d_freqs) { return sc_ch_tables(ctx, d_freqs, F, h, D, de, (double*)ctx->sg_tab.p, &d_terms); };
    sb_windows W;
    c.prepare = [&](const sg_chunk& k) { return sc_sb_windows(ctx, k, seg_win_start, win_lo, win_hi, win_blk_start, blk_hi, W); };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mF = (size_t)st.m * F;
        // (no residual pass and no Spp: neither mode parks a profile)
        int launches = sc_cs_stage_launch(ctx, plan, z, ny, nx, F, h, w, D, de, min_samples, mode, k.tab, d_terms, false, st);
        if (W.NWc) {
            const unsigned grid = (unsigned)std::min<long long>(W.NWc, CWB_MAX_GRID);
            const double* x = own ? st.planes : st.planes + 2 * mF;
            k_window<<<grid, CWB_THREADS, cwb_lds_bytes(W.nb_chunk, F, R, own), ctx->stream>>>(
                W.d_win, W.d_wstart, W.d_wblk, W.d_bhi, st.label, W.NWc, st.used, x, x + mF, k.ages, F, R, level, rpi, seed, min_blocks,
                min_profiles, W.nb_chunk, (sc_channel_strike_boot*)k.out[0], (int*)k.out[1]);
            ++launches;
        }
        return launches;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal - sc_channel_strike's, then the block arrays' and the resampling's -,
// then the bootstrap on the context's DEM (z null) or on z, uploaded
static int cwb_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                    const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                    const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                    const double* freqs, int F, int h, int w, int D, int mode, double de, int min_samples, int min_profiles,
                    const long long* win_blk_start, const long long* blk_hi, long long NWB, int min_blocks, int R, double level,
                    unsigned long long seed, sc_channel_strike_boot* out_rows, int32_t* out_hist) {
    int rc = sc_cs_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, freqs, F, h, w, D, mode, de, 0.0, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_sb_check(ctx, who, seg_start, S, seg_win_start, win_lo, win_hi, NW, win_blk_start, blk_hi, NWB, F, min_blocks, R,
                          level, out_rows, CWB_LDS_TERMS)))
        return rc;
    if (z && (S == 0 || NW == 0)) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    if (NW == 0) return SC_OK;
    return cwb_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_win_start, win_lo, win_hi, NW, win_blk_start,
                   blk_hi, freqs, F, h, w, D, mode, de, min_samples, min_profiles, min_blocks, R, level, seed, out_rows, out_hist);
}

extern "C" int sc_channel_strike_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                           const long long* seg_start, const int32_t* seg_label, long long S,
                                           const long long* seg_win_start, const long long* win_lo, const long long* win_hi,
                                           long long NW, const double* frequencies, int F, int h, int w, int D, int mode,
                                           double de, int min_samples, int min_profiles, const long long* win_blk_start,
                                           const long long* blk_hi, long long NWB, int min_blocks, int R, double level,
                                           uint64_t seed, sc_channel_strike_boot* out_rows, int32_t* out_hist) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_channel_strike_bootstrap");
    if (rc) return rc;
    return cwb_call(ctx, "sc_channel_strike_bootstrap", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                    seg_win_start, win_lo, win_hi, NW, frequencies, F, h, w, D, mode, de, min_samples, min_profiles, win_blk_start,
                    blk_hi, NWB, min_blocks, R, level, seed, out_rows, out_hist);
}

extern "C" int sc_channel_strike_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                               const double* sa, const double* ca, long long K, const long long* seg_start,
                                               const int32_t* seg_label, long long S, const long long* seg_win_start,
                                               const long long* win_lo, const long long* win_hi, long long NW,
                                               const double* frequencies, int F, int h, int w, int D, int mode, double de,
                                               int min_samples, int min_profiles, const long long* win_blk_start,
                                               const long long* blk_hi, long long NWB, int min_blocks, int R, double level,
                                               uint64_t seed, sc_channel_strike_boot* out_rows, int32_t* out_hist) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return cwb_call(ctx, "sc_channel_strike_bootstrap_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_win_start,
                    win_lo, win_hi, NW, frequencies, F, h, w, D, mode, de, min_samples, min_profiles, win_blk_start, blk_hi, NWB,
                    min_blocks, R, level, seed, out_rows, out_hist);
}
