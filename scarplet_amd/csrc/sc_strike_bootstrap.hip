// sc_strike_bootstrap*: block-bootstrap intervals of the offset and the age at every station along the strike of a segment
// (docs/strike.md, "Intervals per station").
//
// Hand-over, stations and windows are sc_fit_strike's: a window is a contiguous range [lo, hi) of its segment's cells,
// which arrive sorted along the strike.  The blocks of a window are cut on the host too - block floor((t_c - t_first) /
// block_length) of the window's cells, the blocks that hold a cell numbered along the strike - and arrive as integers: the
// CSR array win_blk_start over the blocks and blk_hi, the end cell of every block; a window's first block begins at lo and
// every other where the one before ends.  No float is compared here.  Stage one is sc_fit_segments' own (sc_sg_stage_*,
// sc_segment.hip: k_sg_partial or k_sg_shift, k_sg_rank); there is no residual pass and no Spp: a replicate is the argmax
// of Q_i = SSep_i^2 / SSee_i with nothing subtracted (sc_bootstrap.hip).  Then one kernel, a workgroup per window:
//   k_sb_window   1. block terms: waves over the window's blocks, lanes over the ages: (sum See_ci, sum Sep_ci) over the
//                    block's usable profiles in hand-over order - runs of 64 in sequence from the first, then the run
//                    sums in sequence from the first - into LDS; a block without a usable profile keeps (0, 0);
//                    n_profiles counted in integers
//                 2. replicates: waves over the replicates 0..R, replicate 0 every block once; the draws of the others
//                    are formed 64 at a time, one per lane, and read back lane by lane into scalar registers:
//                    key = mix(seed ^ (L * 0x9E3779B97F4A7C15) ^ (station * 0xD1B54A32D192ED03)), u = mix(key +
//                    ((r << 32) | k)), block = ((u >> 32) * nb) >> 32 - station 0 has sc_bootstrap_segments' key; the
//                    sums in draw order from LDS; failed where SSee_i is 0 or not finite at any age; a butterfly argmax
//                    on (Q, index) with the smallest index winning a tie (a NaN never wins); (index, a) of every
//                    replicate stays in LDS
//                 3. summary: an integer histogram of the indices in LDS, the ranks walked along it by one thread, a_mean
//                    and a_sd summed in replicate order by one thread, a bitonic sort of the a in LDS, padded to a power
//                    of two, for a_lo and a_hi; the row and the optional histogram
// Per-replicate outputs are not built: they would be NW x (R + 1) values.
// No float atomics, no float sum across lanes: the same bytes on every run, for every "fit_chunk", and whatever other
// segments the call holds.
// The host side is the windows and the blocks of one chunk, cut to the chunk's cells and segments, and the launch after
// stage one, handed to sc_sg_chunks (sc_segment.hip): the rows and the histograms run over the windows, the call's second
// CSR array.
#include "sc_fit.h"
#include "sc_strike.h"
#include <math.h>
#include <algorithm>

#define SB_RUN 64                        // usable profiles per run of a block's sum: sc_fit_segments' SG_BLOCK
#define SB_WAVES 4                       // 256 threads: at R = 1000 and ten blocks of twenty ages 15 KB of LDS a workgroup,
#define SB_THREADS (64 * SB_WAVES)       // eight workgroups - every wave slot of a CU - before LDS bounds the occupancy
#define SB_LDS_TERMS 65536               // a window's block terms must fit this many bytes
#define SB_MAX_GRID 65536
#define SB_MAX_SEGS (1ll << 20)
#define SB_MAX_WIN (1ll << 21)           // windows of a chunk

// dynamic LDS: the block terms of a window of up to nb blocks, the a of replicates 1..R padded to the sort, their indices
static size_t sb_lds_bytes(int nb, int A, int R) {
    return sizeof(double2) * (size_t)nb * A + (sizeof(double) + 1) * (size_t)sb_sort_len(R);
}

// the sums of one replicate over its drawn blocks, in draw order; T: the window's block terms in LDS, nb rows of A
__device__ __forceinline__ void sb_sums(const double2* T, int nb, int A, int ia, int lane, int r, unsigned long long key,
                                        double& S, double& P) {
    S = 0.0;
    P = 0.0;
    if (r == 0) {                                        // the anchor: every block once
        for (int k = 0; k < nb; ++k) {
            const double2 v = T[k * A + ia];
            S += v.x;
            P += v.y;
        }
        return;
    }
    for (int k0 = 0; k0 < nb; k0 += 64) {
        // 64 draws at once, one per lane (a lane past the end forms a draw nobody reads)
        const unsigned long long u = sb_mix(key + (((unsigned long long)(unsigned)r << 32) | (unsigned)(k0 + lane)));
        const int b = (int)(((u >> 32) * (unsigned long long)(unsigned)nb) >> 32);
        const int nk = min(64, nb - k0);
        for (int j = 0; j < nk; ++j) {
            const int bj = __builtin_amdgcn_readlane(b, j);          // (< nb: the product's high word)
            const double2 v = T[bj * A + ia];
            S += v.x;
            P += v.y;
        }
    }
}

// win: (lo, hi, segment) of every window, cells and segments counted within the chunk; wstart: the segments' CSR array
// over the windows; wblk: the windows' CSR array over the blocks; bhi: the end cell of every block, within the chunk.
// nb_lds: the blocks the launch's LDS holds - no window of the chunk has more
__global__ __launch_bounds__(SB_THREADS) void k_sb_window(const int* __restrict__ win, const int* __restrict__ wstart,
                                                          const int* __restrict__ wblk, const int* __restrict__ bhi,
                                                          const int* __restrict__ label, long long NW,
                                                          const int* __restrict__ used, const double* __restrict__ see,
                                                          const double* __restrict__ sep, const double* __restrict__ ages,
                                                          int A, int R, double level, unsigned long long seed,
                                                          int min_blocks, int min_profiles, int nb_lds,
                                                          sc_strike_boot* __restrict__ rows, int* __restrict__ out_hist) {
    extern __shared__ double2 sb_lds[];
    __shared__ int hist[64];
    __shared__ int cnt[SB_WAVES];
    __shared__ int idx0;
    __shared__ double amp0;
    const int P2 = sb_sort_len(R);
    double2* T = sb_lds;
    double* v = (double*)(sb_lds + (size_t)nb_lds * A);
    signed char* idx = (signed char*)(v + P2);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double nan = __builtin_nan("");
    for (long long g = blockIdx.x; g < NW; g += gridDim.x) {          // (uniform per workgroup: the barriers below)
        const int lo = win[3 * g], hi = win[3 * g + 1], s = win[3 * g + 2];
        const int b0 = wblk[g], nb = min(wblk[g + 1] - b0, nb_lds);   // (the host refused a window of more)
        const int station = (int)(g - wstart[s]);
        __syncthreads();                                 // (the window before is written)
        // 1. the block terms
        int m_wave = 0;
        for (int b = wave; b < nb; b += SB_WAVES) {
            const int k0 = b == 0 ? lo : bhi[b0 + b - 1], k1 = bhi[b0 + b];
            double tS = 0.0, tP = 0.0, rS = 0.0, rP = 0.0;
            int nr = 0;
            bool first = true;
            for (int k = k0; k < k1; ++k) {
                if (used[k] == 0) continue;              // (the same in every lane)
                const size_t o = (size_t)k * A + ia;
                const double vS = see[o], vP = sep[o];
                ++m_wave;
                if (nr == 0) { rS = vS; rP = vP; } else { rS += vS; rP += vP; }
                if (++nr == SB_RUN) {
                    if (first) { tS = rS; tP = rP; first = false; } else { tS += rS; tP += rP; }
                    nr = 0;
                }
            }
            if (nr) {
                if (first) { tS = rS; tP = rP; } else { tS += rS; tP += rP; }
            }
            if (lane < A) T[b * A + lane] = make_double2(tS, tP);
        }
        if (lane == 0) cnt[wave] = m_wave;
        if (tid < 64) hist[tid] = 0;
        __syncthreads();
        int m = 0;
        for (int i = 0; i < SB_WAVES; ++i) m += cnt[i];
        const bool boot = nb >= min_blocks && m >= min_profiles;
        // 2. the replicates (boot is the workgroup's: every lane of every wave reaches the butterfly)
        for (int i = tid; i < P2; i += SB_THREADS) {     // what no replicate writes: failed, or the padding of the sort
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
            for (int r = wave; r <= R; r += SB_WAVES) {
                double SS, SP;
                sb_sums(T, nb, A, ia, lane, r, key, SS, SP);
                // failed: a sum of See that is 0 or not finite at any age
                const bool bad = lane < A && !(SS > 0.0 && SS < INFINITY);
                double q = SP * SP / SS;
                if (lane >= A || q != q) q = -INFINITY;  // (a NaN never wins)
                int qi = lane;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double oq = __shfl_xor(q, o, 64);
                    const int oi = __shfl_xor(qi, o, 64);
                    if (oq > q || (oq == q && oi < qi)) { q = oq; qi = oi; }
                }
                // (no age with a number for Q: failed too)
                if (__ballot(bad) == 0ull && q > -INFINITY) {
                    const double a = __shfl(SP / SS, qi, 64);
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
        for (int i = tid; i < R; i += SB_THREADS) {
            const int k = idx[i];
            if (k >= 0) atomicAdd(&hist[k], 1);          // (integers: any order)
        }
        __syncthreads();
        if (out_hist && tid < A) out_hist[(size_t)g * A + tid] = hist[tid];
        double a_mean = nan, a_sd = nan;
        int n_ok = 0, ilo = -1, ihi = -1, klo = 0, khi = 0;           // (thread 0's)
        if (tid == 0) {
            for (int i = 0; i < A; ++i) n_ok += hist[i];
            if (n_ok > 0) {
                const double q = (1.0 - level) / 2.0;
                klo = min(max((int)floor(q * (double)n_ok), 0), n_ok - 1);
                khi = min(max((int)ceil((1.0 - q) * (double)n_ok) - 1, 0), n_ok - 1);
                int c = 0;
                for (int i = 0; i < A; ++i) {            // x[k] = the first index whose cumulative count passes k
                    c += hist[i];
                    if (ilo < 0 && c > klo) ilo = i;
                    if (ihi < 0 && c > khi) ihi = i;
                }
                double sum = 0.0;
                for (int r = 0; r < R; ++r)
                    if (idx[r] >= 0) sum += v[r];
                a_mean = sum / (double)n_ok;
                if (n_ok > 1) {
                    double ss = 0.0;
                    for (int r = 0; r < R; ++r)
                        if (idx[r] >= 0) {
                            const double d = v[r] - a_mean;
                            ss += d * d;
                        }
                    a_sd = sqrt(ss / (double)(n_ok - 1));
                }
            }
        }
        __syncthreads();
        // the a of the valid replicates ascending, the others (+inf) behind them
        for (int k = 2; k <= P2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P2; i += SB_THREADS) {
                    const int p = i ^ j;
                    if (p > i) {
                        const double x = v[i], y = v[p];
                        if ((x > y) == ((i & k) == 0)) { v[i] = y; v[p] = x; }
                    }
                }
                __syncthreads();
            }
        if (tid == 0) {
            // (the rows were cleared)
            sc_strike_boot* out = rows + g;
            const bool done = boot && n_ok > 0;
            const int i0 = done ? idx0 : -1;
            out->label = label[s];
            out->station = station;
            out->n_cells = hi - lo;
            out->n_profiles = m;
            out->n_blocks = nb;
            out->replicates = R;
            out->n_failed = boot ? R - n_ok : 0;
            out->kt_index0 = i0;
            out->lo_index = done ? ilo : -1;
            out->hi_index = done ? ihi : -1;
            out->status = done ? (ilo == 0 ? 2 : 0) + (ihi == A - 1 ? 4 : 0) : 1;
            out->kt0 = i0 >= 0 ? ages[i0] : nan;
            out->kt_lo = done ? ages[ilo] : nan;
            out->kt_hi = done ? ages[ihi] : nan;
            out->a0 = done ? amp0 : nan;
            out->a_mean = done ? a_mean : nan;
            out->a_sd = done ? a_sd : nan;
            out->a_lo = done ? v[klo] : nan;
            out->a_hi = done ? v[khi] : nan;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int sb_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_win_start,
                  const long long* win_lo, const long long* win_hi, long long NW, const long long* win_blk_start,
                  const long long* blk_hi, const double* ages, int A, int h, int w, int D, double de, int min_samples,
                  int min_profiles, int min_blocks, int R, double level, unsigned long long seed, sc_strike_boot* out_rows,
                  int32_t* out_hist) {
    if (S == 0) return SC_OK;
    const int Ds = D > 0 ? D : -1;                       // D = 0 is the call without a shift: its kernel, its park
    const int ht = h + (D > 0 ? D : 0);
    int rc;
    if ((rc = sc_sg_stage_attr(ctx, A, h, Ds))) return rc;
    // the dynamic LDS of the call's largest window, raised once
    long long nb_call = 0;
    for (long long g = 0; g < NW; ++g) nb_call = std::max(nb_call, win_blk_start[g + 1] - win_blk_start[g]);
    if ((rc = sc_lds_attr(ctx, (const void*)k_sb_window, sb_lds_bytes((int)nb_call, A, R)))) return rc;

    // (a chunk holds as many whole segments as fit the parked bytes and the windows' outputs)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, ht, de, sg_park_plain(A, h, Ds >= 0), SB_MAX_SEGS, seg_win_start,
                 SB_MAX_WIN, 0};
    c.out = {{out_rows, &ctx->sb_rows, sizeof(sc_strike_boot), SG_AUX, true}, {out_hist, &ctx->sb_hist, sizeof(int) * A, SG_AUX}};
    sb_windows W;
    c.prepare = [&](const sg_chunk& k) { return sc_sb_windows(ctx, k, seg_win_start, win_lo, win_hi, win_blk_start, blk_hi, W); };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mA = (size_t)st.m * A;
        int launches = sc_sg_stage_launch(ctx, z, ny, nx, A, h, w, Ds, de, min_samples, k.tab, st);
        if (W.NWc) {
            const unsigned grid = (unsigned)std::min<long long>(W.NWc, SB_MAX_GRID);
            k_sb_window<<<grid, SB_THREADS, sb_lds_bytes(W.nb_chunk, A, R), ctx->stream>>>(
                W.d_win, W.d_wstart, W.d_wblk, W.d_bhi, st.label, W.NWc, st.used, st.planes + 2 * mA, st.planes + 3 * mA, k.ages, A, R,
                level, seed, min_blocks, min_profiles, W.nb_chunk, (sc_strike_boot*)k.out[0], (int*)k.out[1]);
            ++launches;
        }
        return launches;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal, then the bootstrap on the context's DEM (z null) or on z, uploaded
static int sb_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                   const double* ages, int A, int h, int w, int D, double de, int min_samples, int min_profiles,
                   const long long* win_blk_start, const long long* blk_hi, long long NWB, int min_blocks, int R, double level,
                   unsigned long long seed, sc_strike_boot* out_rows, int32_t* out_hist) {
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    // (the park of a shifted call counts d_ci whatever D is: the limit of sc_fit_segments_shift)
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, D, de, 0.0, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_sb_check(ctx, who, seg_start, S, seg_win_start, win_lo, win_hi, NW, win_blk_start, blk_hi, NWB, A, min_blocks, R,
                          level, out_rows, SB_LDS_TERMS)))
        return rc;
    if (z && (S == 0 || NW == 0)) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    if (NW == 0) return SC_OK;
    return sb_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_win_start, win_lo, win_hi, NW, win_blk_start,
                  blk_hi, ages, A, h, w, D, de, min_samples, min_profiles, min_blocks, R, level, seed, out_rows, out_hist);
}

extern "C" int sc_strike_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                   const long long* seg_start, const int32_t* seg_label, long long S,
                                   const long long* seg_win_start, const long long* win_lo, const long long* win_hi,
                                   long long NW, const double* ages, int A, int h, int w, int D, double de, int min_samples,
                                   int min_profiles, const long long* win_blk_start, const long long* blk_hi, long long NWB,
                                   int min_blocks, int R, double level, uint64_t seed, sc_strike_boot* out_rows,
                                   int32_t* out_hist) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_strike_bootstrap");
    if (rc) return rc;
    return sb_call(ctx, "sc_strike_bootstrap", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                   seg_win_start, win_lo, win_hi, NW, ages, A, h, w, D, de, min_samples, min_profiles, win_blk_start, blk_hi, NWB,
                   min_blocks, R, level, seed, out_rows, out_hist);
}

extern "C" int sc_strike_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                       const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                       long long S, const long long* seg_win_start, const long long* win_lo,
                                       const long long* win_hi, long long NW, const double* ages, int A, int h, int w, int D,
                                       double de, int min_samples, int min_profiles, const long long* win_blk_start,
                                       const long long* blk_hi, long long NWB, int min_blocks, int R, double level,
                                       uint64_t seed, sc_strike_boot* out_rows, int32_t* out_hist) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return sb_call(ctx, "sc_strike_bootstrap_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_win_start, win_lo,
                   win_hi, NW, ages, A, h, w, D, de, min_samples, min_profiles, win_blk_start, blk_hi, NWB, min_blocks, R, level,
                   seed, out_rows, out_hist);
}
