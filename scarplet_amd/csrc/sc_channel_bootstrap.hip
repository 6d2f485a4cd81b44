// sc_channel_bootstrap*: block-bootstrap intervals of a reach's width, depth and area (docs/channels.md, "Intervals per
// reach").
//
// What sc_bootstrap_segments (sc_bootstrap.hip) is to sc_fit_segments, for sc_channel_segments: the blocks, the hand-over
// and the draws are its own, stage one is sc_channel_segments' (k_cs_stage, k_sg_rank: the same samples and the same d_ci
// per profile and frequency, on either route of the search), and there is no residual pass in either mode:
//   SC_CHANNEL_DEPTH_SEGMENT  Spp depends on neither the frequency nor the shifts, so the best frequency of a replicate is
//                             the argmax of Q_i = SSep_i^2 / SSee_i over the drawn blocks' sums and a = SSep / SSee there
//   SC_CHANNEL_DEPTH_PROFILE  the pooled sse is the sum of the profiles' own sse*_ci: the argmin of SSse_i, and a =
//                             SA_i / M there, M the usable profiles drawn, with multiplicity
// A frequency that is dead in a drawn profile (NaN terms) is dead for that replicate only and never wins; a replicate
// fails only when no frequency is live.  Then
//   (k_bs_terms, sc_bootstrap.hip: segment mode's block terms, on the parked See and Sep)
//   k_cb_terms    profile mode's: one wave per block, lanes over the frequencies: (sum sse*_ci, sum a_ci) over the block's
//                 usable profiles in hand-over order - runs of 64 in sequence from the first, then the run sums in sequence
//                 from the first, k_bs_terms' order - and m_b, their number
//   k_cb_reps     k_bs_reps' shape: lanes over the frequencies, waves over (reach, replicate), BS_TILE replicates to a wave;
//                 the draws of a replicate are formed 64 at a time, one per lane, and read back lane by lane into scalar
//                 registers; a reach's block terms are staged in LDS where they fit BS_LDS_MAX and read as rows of global
//                 memory otherwise; M in integers; a butterfly argmin on (key, index) - key = -Q or SSse, +inf and an
//                 index past the frequencies where the frequency is not live - with the smallest index winning a tie;
//                 (f_index int8, a) per replicate
//   k_cb_summary  one workgroup per reach: an integer histogram of the indices in LDS, the ranks walked along it, and twice
//                 over the same array of R doubles - first the a, then the areas -a_r / (sqrt(pi) f[index_r]) - the mean
//                 and the sd summed in replicate order by one thread and a bitonic sort for the two ranks
// No float atomics, no float sum across lanes: the same bytes on every run, whatever other reaches the call holds.
// The host side is bs_run's: the caller's blocks of one chunk, cut to the chunk's cells, and the launches after stage one,
// handed to sc_sg_chunks (sc_segment.hip).
#include "sc_bootstrap.h"
#include "sc_channel.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(64) void k_cb_terms(const int* __restrict__ used, const double* __restrict__ sse,
                                                 const double* __restrict__ amp, const int* __restrict__ blk_start,
                                                 long long NB, int F, double2* __restrict__ terms, int* __restrict__ mb) {
    const int lane = threadIdx.x;
    const int ia = min(lane, F - 1);                     // lanes beyond the frequencies repeat the last one and are ignored
    for (long long g = blockIdx.x; g < NB; g += gridDim.x) {
        const int k0 = blk_start[g], k1 = blk_start[g + 1];
        double tS = 0.0, tA = 0.0, rS = 0.0, rA = 0.0;
        int nr = 0, m = 0;
        bool first = true;
        for (int k = k0; k < k1; ++k) {
            if (used[k] == 0) continue;                  // (the same in every lane)
            const size_t o = (size_t)k * F + ia;
            const double vS = sse[o], vA = amp[o];
            ++m;
            if (nr == 0) { rS = vS; rA = vA; } else { rS += vS; rA += vA; }
            if (++nr == BS_RUN) {
                if (first) { tS = rS; tA = rA; first = false; } else { tS += rS; tA += rA; }
                nr = 0;
            }
        }
        if (nr) {
            if (first) { tS = rS; tA = rA; } else { tS += rS; tA += rA; }
        }
        if (lane < F) terms[(size_t)g * F + lane] = make_double2(tS, tA);
        if (lane == 0) mb[g] = m;
    }
}

template <bool OWN>
__global__ __launch_bounds__(BS_THREADS) void k_cb_reps(const int* __restrict__ seg_blk, const int* __restrict__ label,
                                                        const int* __restrict__ cnt, const double2* __restrict__ terms,
                                                        const int* __restrict__ mb, long long S, int F, int R,
                                                        unsigned long long seed, int min_blocks, int min_profiles,
                                                        int lds_blocks, signed char* __restrict__ out_index,
                                                        double* __restrict__ out_a) {
    extern __shared__ double2 cb_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ia = min(lane, F - 1);
    const double nan = __builtin_nan("");
    const int tiles = (R + 1 + BS_WAVES * BS_TILE - 1) / (BS_WAVES * BS_TILE);
    const long long items = S * tiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {    // (uniform per workgroup: the barriers below)
        const long long s = it / tiles;
        const int t = (int)(it - s * tiles);
        const int b0 = seg_blk[s], nb = seg_blk[s + 1] - b0;
        const bool boot = bs_boot(nb, cnt[2 * s], min_blocks, min_profiles);
        const bool in_lds = boot && nb <= lds_blocks;
        const double2* T = terms + (size_t)b0 * F;
        __syncthreads();                                 // (the waves of the item before have read their terms)
        if (in_lds)
            for (int idx = threadIdx.x; idx < nb * F; idx += BS_THREADS) cb_lds[idx] = T[idx];
        __syncthreads();
        const unsigned long long key = bs_key(seed, label[s]);
        const int r0 = t * (BS_WAVES * BS_TILE) + wave * BS_TILE;
        for (int r = r0; r < min(r0 + BS_TILE, R + 1); ++r) {
            int best = -1;
            double a = nan;
            if (boot) {
                double X, Y;
                int M;
                // (bs_sums' draws and order of additions, with the drawn blocks' usable profiles counted in profile mode)
                if (in_lds) bs_sums_counted<OWN>(cb_lds, mb + b0, nb, F, ia, lane, r, key, X, Y, M);
                else bs_sums_counted<OWN>(T, mb + b0, nb, F, ia, lane, r, key, X, Y, M);
                // the smallest key among the live frequencies: SSse, or -Q for the largest Q
                double q, v;
                bool live;
                if (OWN) {
                    q = X;
                    v = Y / (double)M;
                    live = M > 0 && X == X;
                } else {
                    const double Q = Y * Y / X;
                    q = -Q;
                    v = Y / X;
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
                    best = qi;
                    a = __shfl(v, qi, 64);
                }
            }
            if (lane == 0) {
                const size_t o = (size_t)s * (R + 1) + r;
                out_index[o] = (signed char)best;
                out_a[o] = a;
            }
        }
    }
}

// rpi: sqrt(pi), the host's
__global__ __launch_bounds__(BS_THREADS) void k_cb_summary(const int* __restrict__ seg_start, const int* __restrict__ seg_blk,
                                                           const int* __restrict__ label, const int* __restrict__ cnt,
                                                           const double* __restrict__ freqs, long long S, int F, int R,
                                                           double level, double rpi, int min_blocks, int min_profiles,
                                                           const signed char* __restrict__ index,
                                                           const double* __restrict__ amp, int* __restrict__ out_hist,
                                                           sc_channel_boot* __restrict__ rows) {
    __shared__ double v[SC_BOOT_MAX_REPLICATES];
    __shared__ signed char okr[SC_BOOT_MAX_REPLICATES];
    __shared__ int hist[64];
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    int P2 = 2;                                          // the sort's length: a power of two >= R
    while (P2 < R) P2 <<= 1;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int nb = seg_blk[s + 1] - seg_blk[s], m = cnt[2 * s];
        const bool boot = bs_boot(nb, m, min_blocks, min_profiles);
        const size_t base = (size_t)s * (R + 1);
        __syncthreads();                                 // (the reach before is written)
        if (tid < 64) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < R; i += BS_THREADS) {
            const int idx = boot ? (int)index[base + 1 + i] : -1;
            if (idx >= 0) atomicAdd(&hist[idx], 1);      // (integers: any order)
            okr[i] = idx >= 0 ? 1 : 0;
        }
        __syncthreads();
        if (tid < F) out_hist[s * F + tid] = hist[tid];
        int n_ok = 0, lo = -1, hi = -1, klo = 0, khi = 0;            // (thread 0's)
        if (tid == 0) {
            for (int i = 0; i < F; ++i) n_ok += hist[i];
            if (n_ok > 0) {
                const double q = (1.0 - level) / 2.0;
                klo = min(max((int)floor(q * (double)n_ok), 0), n_ok - 1);
                khi = min(max((int)ceil((1.0 - q) * (double)n_ok) - 1, 0), n_ok - 1);
                int c = 0;
                for (int i = 0; i < F; ++i) {            // x[k] = the first index whose cumulative count passes k
                    c += hist[i];
                    if (lo < 0 && c > klo) lo = i;
                    if (hi < 0 && c > khi) hi = i;
                }
            }
        }
        // the same array twice: the a of the valid replicates, then their areas
        double mean[2] = {nan, nan}, sd[2] = {nan, nan}, vlo[2] = {nan, nan}, vhi[2] = {nan, nan};         // (thread 0's)
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();                             // (thread 0 has read the ranks of the pass before)
            for (int i = tid; i < P2; i += BS_THREADS) {
                double x = INFINITY;
                if (i < R && okr[i]) {
                    x = amp[base + 1 + i];
                    if (pass) x = -x / (rpi * freqs[(int)index[base + 1 + i]]);
                }
                v[i] = x;
            }
            __syncthreads();
            if (tid == 0 && n_ok > 0) {
                double sum = 0.0;
                for (int r = 0; r < R; ++r)
                    if (okr[r]) sum += v[r];
                mean[pass] = sum / (double)n_ok;
                if (n_ok > 1) {
                    double ss = 0.0;
                    for (int r = 0; r < R; ++r)
                        if (okr[r]) {
                            const double d = v[r] - mean[pass];
                            ss += d * d;
                        }
                    sd[pass] = sqrt(ss / (double)(n_ok - 1));
                }
            }
            __syncthreads();
            // the values of the valid replicates ascending, the others (+inf) behind them
            for (int k = 2; k <= P2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < P2; i += BS_THREADS) {
                        const int p = i ^ j;
                        if (p > i) {
                            const double x = v[i], y = v[p];
                            if ((x > y) == ((i & k) == 0)) { v[i] = y; v[p] = x; }
                        }
                    }
                    __syncthreads();
                }
            if (tid == 0 && n_ok > 0) {
                vlo[pass] = v[klo];
                vhi[pass] = v[khi];
            }
        }
        if (tid == 0) {
            // (the rows were cleared)
            sc_channel_boot* out = rows + s;
            const bool done = boot && n_ok > 0;
            const int r0 = boot ? (int)index[base] : -1;
            const int i0 = done ? r0 : -1;
            const double a0 = i0 >= 0 ? amp[base] : nan;
            out->label = label[s];
            out->n_cells = seg_start[s + 1] - seg_start[s];
            out->n_profiles = m;
            out->n_blocks = nb;
            out->replicates = R;
            out->n_failed = boot ? R - n_ok : 0;
            out->f_index0 = i0;
            out->lo_index = done ? lo : -1;
            out->hi_index = done ? hi : -1;
            out->status = done ? (lo == 0 ? 2 : 0) + (hi == F - 1 ? 4 : 0) : (boot && r0 < 0 ? 1 | 32 : 1);
            out->f0 = i0 >= 0 ? freqs[i0] : nan;
            out->f_lo = done ? freqs[lo] : nan;
            out->f_hi = done ? freqs[hi] : nan;
            out->a0 = a0;
            out->a_mean = done ? mean[0] : nan;
            out->a_sd = done ? sd[0] : nan;
            out->a_lo = done ? vlo[0] : nan;
            out->a_hi = done ? vhi[0] : nan;
            out->area0 = i0 >= 0 ? -a0 / (rpi * freqs[i0]) : nan;
            out->area_mean = done ? mean[1] : nan;
            out->area_sd = done ? sd[1] : nan;
            out->area_lo = done ? vlo[1] : nan;
            out->area_hi = done ? vhi[1] : nan;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int cb_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_blk_start,
                  const long long* blk_start, const double* freqs, int F, int h, int w, int D, int mode, double de,
                  int min_samples, int min_profiles, int min_blocks, int R, double level, unsigned long long seed,
                  sc_channel_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (S == 0) return SC_OK;
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;
    const size_t R1 = (size_t)R + 1;
    const double rpi = sqrt(M_PI);
    const auto k_reps = own ? k_cb_reps<true> : k_cb_reps<false>;
    cs_stage_plan plan;
    int rc;
    if ((rc = sc_cs_stage_attr(ctx, F, h, D, &plan))) return rc;

    // a chunk holds as many whole reaches as fit the parked bytes and the replicates' outputs
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, freqs, F, h + D, de, sg_park_plain(F, h, true),
                 std::min<long long>(BS_MAX_SEGS, BS_MAX_OUT / (long long)R1), nullptr, 0, 0};
    // (the kernels write the histogram, the indices and the amplitudes whether or not they are asked for)
    c.out = {{out_rows, &ctx->cb_rows, sizeof(sc_channel_boot), SG_SEGS, true},
             {out_hist, &ctx->bs_hist, sizeof(int) * F, SG_SEGS, false, true},
             {out_index, &ctx->bs_index, R1, SG_SEGS, false, true},
             {out_a, &ctx->bs_a, sizeof(double) * R1, SG_SEGS, false, true}};
    const double* d_pairs = nullptr;
    // (the frame's table over h + D has the size of G, which takes its place: k.tab is G from here on)
    c.tables = [&](const double* d_freqs) { return sc_ch_tables(ctx, d_freqs, F, h, D, de, (double*)ctx->sg_tab.p, &d_pairs); };
    std::vector<int> blk, sblk;
    const int lds_fit = (int)(BS_LDS_MAX / (sizeof(double2) * (size_t)F));      // blocks of a reach that LDS holds
    int *d_blk, *d_sblk, *d_mb, lds_blocks;
    double2* d_terms;
    long long NBc;
    size_t lds;
    c.prepare = [&](const sg_chunk& k) {
        const long long Sc = k.st.Sc, b0 = seg_blk_start[k.s0];
        NBc = seg_blk_start[k.s1] - b0;
        blk.resize((size_t)NBc + 1);
        sblk.resize((size_t)Sc + 1);
        lds_blocks = 0;
        for (long long b = 0; b <= NBc; ++b) blk[b] = (int)(blk_start[b0 + b] - k.k0);
        for (long long s = 0; s <= Sc; ++s) sblk[s] = (int)(seg_blk_start[k.s0 + s] - b0);
        for (long long s = 0; s < Sc; ++s) {
            const int nb = sblk[s + 1] - sblk[s];
            if (nb <= lds_fit) lds_blocks = std::max(lds_blocks, nb);
        }
        lds = sizeof(double2) * (size_t)lds_blocks * F;
        if ((rc = sc_ensure(ctx, ctx->bs_blk, sizeof(int) * ((size_t)NBc + 1)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->bs_sblk, sizeof(int) * ((size_t)Sc + 1)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->bs_terms, sizeof(double2) * (size_t)NBc * F))) return rc;
        if ((rc = sc_ensure(ctx, ctx->cb_mb, sizeof(int) * ((size_t)NBc + 1)))) return rc;
        if ((rc = sc_lds_attr(ctx, (const void*)k_reps, lds))) return rc;
        d_blk = (int*)ctx->bs_blk.p;
        d_sblk = (int*)ctx->bs_sblk.p;
        d_mb = (int*)ctx->cb_mb.p;
        d_terms = (double2*)ctx->bs_terms.p;
        SC_HIP(ctx, hipMemcpyAsync(d_blk, blk.data(), sizeof(int) * ((size_t)NBc + 1), hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(d_sblk, sblk.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
        return SC_OK;
    };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mF = (size_t)st.m * F;
        const int tiles = (R + 1 + BS_WAVES * BS_TILE - 1) / (BS_WAVES * BS_TILE);
        signed char* d_index = (signed char*)k.out[2];
        double* d_a = (double*)k.out[3];
        // (no residual pass: segment mode parks no profile)
        int launches = sc_cs_stage_launch(ctx, plan, z, ny, nx, F, h, w, D, de, min_samples, mode, k.tab, d_pairs, false, st);
        if (NBc && own) {
            k_cb_terms<<<sg_grid(NBc), 64, 0, ctx->stream>>>(st.used, st.planes, st.planes + mF, d_blk, NBc, F, d_terms, d_mb);
            ++launches;
        } else if (NBc) {
            sc_bs_terms_launch(ctx, st.used, st.planes + 2 * mF, st.planes + 3 * mF, d_blk, NBc, F, d_terms);
            ++launches;
        }
        k_reps<<<bs_grid(st.Sc * tiles), BS_THREADS, lds, ctx->stream>>>(d_sblk, st.label, st.cnt, d_terms, d_mb, st.Sc, F, R, seed,
                                                                        min_blocks, min_profiles, lds_blocks, d_index, d_a);
        k_cb_summary<<<bs_grid(st.Sc), BS_THREADS, 0, ctx->stream>>>(st.seg, d_sblk, st.label, st.cnt, k.ages, st.Sc, F, R, level,
                                                                    rpi, min_blocks, min_profiles, d_index, d_a, (int*)k.out[1],
                                                                    (sc_channel_boot*)k.out[0]);
        return launches + 2;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal - cs_call's, then the block arrays' -, then the bootstrap on the
// context's DEM (z null) or on z, uploaded
static int cb_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const long long* seg_blk_start, const long long* blk_start, long long NB, const double* freqs, int F, int h,
                   int w, int D, int mode, double de, int min_samples, int min_profiles, int min_blocks, int R, double level,
                   unsigned long long seed, sc_channel_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    int rc = sc_cs_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, freqs, F, h, w, D, mode, de, 0.0, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_bs_check(ctx, who, K, seg_start, S, seg_blk_start, blk_start, NB, min_blocks, R, level))) return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return cb_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_blk_start, blk_start, freqs, F, h, w, D, mode,
                  de, min_samples, min_profiles, min_blocks, R, level, seed, out_rows, out_hist, out_index, out_a);
}

extern "C" int sc_channel_bootstrap(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                    const long long* seg_start, const int32_t* seg_label, long long S,
                                    const long long* seg_blk_start, const long long* blk_start, long long NB,
                                    const double* frequencies, int F, int h, int w, int D, int mode, double de,
                                    int min_samples, int min_profiles, int min_blocks, int R, double level, uint64_t seed,
                                    sc_channel_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_channel_bootstrap");
    if (rc) return rc;
    return cb_call(ctx, "sc_channel_bootstrap", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                   seg_blk_start, blk_start, NB, frequencies, F, h, w, D, mode, de, min_samples, min_profiles, min_blocks, R,
                   level, seed, out_rows, out_hist, out_index, out_a);
}

extern "C" int sc_channel_bootstrap_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                        const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                        long long S, const long long* seg_blk_start, const long long* blk_start, long long NB,
                                        const double* frequencies, int F, int h, int w, int D, int mode, double de,
                                        int min_samples, int min_profiles, int min_blocks, int R, double level, uint64_t seed,
                                        sc_channel_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return cb_call(ctx, "sc_channel_bootstrap_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_blk_start,
                   blk_start, NB, frequencies, F, h, w, D, mode, de, min_samples, min_profiles, min_blocks, R, level, seed,
                   out_rows, out_hist, out_index, out_a);
}
