// sc_bootstrap_segments*: block-bootstrap intervals of a segment's age (docs/bootstrap.md).
//
// In the fixed-effects model of docs/segments.md the pooled sse at age i is Spp - (sum_c Sep_ci)^2 / (sum_c See_ci) and
// Spp does not depend on the age, so a replicate that resamples whole profiles needs no residual pass: with the sums
// taken over the drawn blocks, a_i = SSep_i / SSee_i and the best age is the argmax of Q_i = SSep_i^2 / SSee_i.
// Nothing is subtracted.  Stage one is sc_fit_segments' own (sc_sg_stage_*, sc_segment.hip: k_sg_partial or k_sg_shift,
// k_sg_rank); then
//   k_bs_terms    one wave per block, lanes over the ages: (sum See_ci, sum Sep_ci) over the block's usable profiles in
//                 hand-over order - runs of 64 in sequence from the first, then the run sums in sequence from the first
//   k_bs_reps     lanes over the ages, waves over (segment, replicate): the draws of a replicate are formed 64 at a time,
//                 one per lane, and read back lane by lane into scalar registers; a segment's block terms are staged in
//                 LDS where they fit BS_LDS_MAX and read as rows of global memory otherwise; a butterfly argmax with the
//                 smallest index winning a tie; (kt_index int8, a) per replicate
//   k_bs_summary  one workgroup per segment: an integer histogram of the indices in LDS, the ranks walked along it, a_mean
//                 and a_sd summed in replicate order by one thread, a bitonic sort of the a in LDS for a_lo and a_hi
// No float atomics, no float sum across lanes: the same bytes on every run.
// The host side is the caller's blocks of one chunk, cut to the chunk's cells, and the launches after stage one, handed to
// sc_sg_chunks (sc_segment.hip); a replicate output of R + 1 values per segment is a segment output of that item size.
#include "sc_bootstrap.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(64) void k_bs_terms(const int* __restrict__ used, const double* __restrict__ see,
                                                 const double* __restrict__ sep, const int* __restrict__ blk_start,
                                                 long long NB, int A, double2* __restrict__ terms) {
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    for (long long g = blockIdx.x; g < NB; g += gridDim.x) {
        const int k0 = blk_start[g], k1 = blk_start[g + 1];
        double tS = 0.0, tP = 0.0, rS = 0.0, rP = 0.0;
        int nr = 0;
        bool first = true;
        for (int k = k0; k < k1; ++k) {
            if (used[k] == 0) continue;                  // (the same in every lane)
            const size_t o = (size_t)k * A + ia;
            const double vS = see[o], vP = sep[o];
            if (nr == 0) { rS = vS; rP = vP; } else { rS += vS; rP += vP; }
            if (++nr == BS_RUN) {
                if (first) { tS = rS; tP = rP; first = false; } else { tS += rS; tP += rP; }
                nr = 0;
            }
        }
        if (nr) {
            if (first) { tS = rS; tP = rP; } else { tS += rS; tP += rP; }
        }
        if (lane < A) terms[(size_t)g * A + lane] = make_double2(tS, tP);
    }
}

__global__ __launch_bounds__(BS_THREADS) void k_bs_reps(const int* __restrict__ seg_blk, const int* __restrict__ label,
                                                        const int* __restrict__ cnt, const double2* __restrict__ terms,
                                                        long long S, int A, int R, unsigned long long seed, int min_blocks,
                                                        int min_profiles, int lds_blocks, signed char* __restrict__ out_index,
                                                        double* __restrict__ out_a) {
    extern __shared__ double2 bs_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ia = min(lane, A - 1);
    const double nan = __builtin_nan("");
    const int tiles = (R + 1 + BS_WAVES * BS_TILE - 1) / (BS_WAVES * BS_TILE);
    const long long items = S * tiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {    // (uniform per workgroup: the barriers below)
        const long long s = it / tiles;
        const int t = (int)(it - s * tiles);
        const int b0 = seg_blk[s], nb = seg_blk[s + 1] - b0;
        const bool boot = bs_boot(nb, cnt[2 * s], min_blocks, min_profiles);
        const bool in_lds = boot && nb <= lds_blocks;
        const double2* T = terms + (size_t)b0 * A;
        __syncthreads();                                 // (the waves of the item before have read their terms)
        if (in_lds)
            for (int idx = threadIdx.x; idx < nb * A; idx += BS_THREADS) bs_lds[idx] = T[idx];
        __syncthreads();
        const unsigned long long key = bs_mix(seed ^ ((unsigned long long)(unsigned)label[s] * 0x9E3779B97F4A7C15ull));
        const int r0 = t * (BS_WAVES * BS_TILE) + wave * BS_TILE;
        for (int r = r0; r < min(r0 + BS_TILE, R + 1); ++r) {
            int best = -1;
            double a = nan;
            if (boot) {
                double SS, SP;
                if (in_lds) bs_sums(bs_lds, nb, A, ia, lane, r, key, SS, SP);
                else bs_sums(T, nb, A, ia, lane, r, key, SS, SP);
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
                    best = qi;
                    a = __shfl(SP / SS, qi, 64);
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

__global__ __launch_bounds__(BS_THREADS) void k_bs_summary(const int* __restrict__ seg_start, const int* __restrict__ seg_blk,
                                                           const int* __restrict__ label, const int* __restrict__ cnt,
                                                           const double* __restrict__ ages, long long S, int A, int R,
                                                           double level, int min_blocks, int min_profiles,
                                                           const signed char* __restrict__ index,
                                                           const double* __restrict__ amp, int* __restrict__ out_hist,
                                                           sc_segment_boot* __restrict__ rows) {
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
        __syncthreads();                                 // (the segment before is written)
        if (tid < 64) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < P2; i += BS_THREADS) {
            const int idx = (boot && i < R) ? (int)index[base + 1 + i] : -1;
            if (idx >= 0) atomicAdd(&hist[idx], 1);      // (integers: any order)
            if (i < R) okr[i] = idx >= 0 ? 1 : 0;
            v[i] = idx >= 0 ? amp[base + 1 + i] : INFINITY;
        }
        __syncthreads();
        if (tid < A) out_hist[s * A + tid] = hist[tid];
        double a_mean = nan, a_sd = nan;
        int n_ok = 0, lo = -1, hi = -1, klo = 0, khi = 0;           // (thread 0's)
        if (tid == 0) {
            for (int i = 0; i < A; ++i) n_ok += hist[i];
            if (n_ok > 0) {
                const double q = (1.0 - level) / 2.0;
                klo = min(max((int)floor(q * (double)n_ok), 0), n_ok - 1);
                khi = min(max((int)ceil((1.0 - q) * (double)n_ok) - 1, 0), n_ok - 1);
                int c = 0;
                for (int i = 0; i < A; ++i) {            // x[k] = the first index whose cumulative count passes k
                    c += hist[i];
                    if (lo < 0 && c > klo) lo = i;
                    if (hi < 0 && c > khi) hi = i;
                }
                double sum = 0.0;
                for (int r = 0; r < R; ++r)
                    if (okr[r]) sum += v[r];
                a_mean = sum / (double)n_ok;
                if (n_ok > 1) {
                    double ss = 0.0;
                    for (int r = 0; r < R; ++r)
                        if (okr[r]) {
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
                for (int i = tid; i < P2; i += BS_THREADS) {
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
            sc_segment_boot* out = rows + s;
            const bool done = boot && n_ok > 0;
            const int i0 = done ? (int)index[base] : -1;
            out->label = label[s];
            out->n_cells = seg_start[s + 1] - seg_start[s];
            out->n_profiles = m;
            out->n_blocks = nb;
            out->replicates = R;
            out->n_failed = boot ? R - n_ok : 0;
            out->kt_index0 = i0;
            out->lo_index = done ? lo : -1;
            out->hi_index = done ? hi : -1;
            out->status = done ? (lo == 0 ? 2 : 0) + (hi == A - 1 ? 4 : 0) : 1;
            out->kt0 = i0 >= 0 ? ages[i0] : nan;
            out->kt_lo = done ? ages[lo] : nan;
            out->kt_hi = done ? ages[hi] : nan;
            out->a0 = done ? amp[base] : nan;
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
int sc_bs_check(sc_ctx* ctx, const char* who, long long K, const long long* seg_start, long long S,
                const long long* seg_blk_start, const long long* blk_start, long long NB, int min_blocks, int R, double level) {
    if (!seg_blk_start || !blk_start) return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (R < 1 || R > SC_BOOT_MAX_REPLICATES)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: R must lie in 1..%d", who, SC_BOOT_MAX_REPLICATES);
    if (!(level > 0.0 && level < 1.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: level must lie strictly between 0 and 1", who);
    if (min_blocks < 2) return sc_fail(ctx, SC_ERR_INVALID, "%s: min_blocks must be >= 2", who);
    if (NB < 0 || NB > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_INVALID, "%s: NB must lie in 0..2^31 - 1", who);
    if (seg_blk_start[0] != 0 || seg_blk_start[S] != NB)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_blk_start must run from 0 to NB", who);
    if (blk_start[0] != 0 || blk_start[NB] != K) return sc_fail(ctx, SC_ERR_INVALID, "%s: blk_start must run from 0 to K", who);
    for (long long s = 0; s < S; ++s)
        if (seg_blk_start[s + 1] < seg_blk_start[s] || seg_blk_start[s + 1] > NB)
            return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_blk_start decreases or leaves 0..NB at segment %lld", who, s);
    for (long long b = 0; b < NB; ++b)
        if (blk_start[b + 1] < blk_start[b]) return sc_fail(ctx, SC_ERR_INVALID, "%s: blk_start decreases at block %lld", who, b);
    for (long long s = 0; s <= S; ++s)
        if (blk_start[seg_blk_start[s]] != seg_start[s])
            return sc_fail(ctx, SC_ERR_INVALID, "%s: the blocks of segment %lld do not cover its cells", who, std::min(s, S - 1));
    return SC_OK;
}

void sc_bs_terms_launch(sc_ctx* ctx, const int* used, const double* x, const double* y, const int* blk, long long NB, int A,
                        double2* terms) {
    k_bs_terms<<<(unsigned)std::max<long long>(1, std::min<long long>(NB, 65536)), 64, 0, ctx->stream>>>(used, x, y, blk, NB, A,
                                                                                                        terms);
}

static int bs_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const long long* seg_blk_start,
                  const long long* blk_start, const double* ages, int A, int h, int w, int D, double de, int min_samples,
                  int min_profiles, int min_blocks, int R, double level, unsigned long long seed, sc_segment_boot* out_rows,
                  int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (S == 0) return SC_OK;
    const int Ds = D > 0 ? D : -1;                       // D = 0 is the call without a shift: its kernel, its park
    const int ht = h + (D > 0 ? D : 0);
    const size_t R1 = (size_t)R + 1;
    int rc;
    if ((rc = sc_sg_stage_attr(ctx, A, h, Ds))) return rc;

    // a chunk holds as many whole segments as fit the parked bytes and the replicates' outputs
    // (Sc R1 <= BS_MAX_OUT is a bound on the segments: Sc <= BS_MAX_OUT / R1, rounded down)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, ht, de, sg_park_plain(A, h, Ds >= 0),
                 std::min<long long>(BS_MAX_SEGS, BS_MAX_OUT / (long long)R1), nullptr, 0, 0};
    // (the kernels write the histogram, the indices and the amplitudes whether or not they are asked for)
    c.out = {{out_rows, &ctx->bs_rows, sizeof(sc_segment_boot), SG_SEGS, true},
             {out_hist, &ctx->bs_hist, sizeof(int) * A, SG_SEGS, false, true},
             {out_index, &ctx->bs_index, R1, SG_SEGS, false, true},
             {out_a, &ctx->bs_a, sizeof(double) * R1, SG_SEGS, false, true}};
    std::vector<int> blk, sblk;
    const int lds_fit = (int)(BS_LDS_MAX / (sizeof(double2) * (size_t)A));      // blocks of a segment that LDS holds
    int *d_blk, *d_sblk, lds_blocks;
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
        lds = sizeof(double2) * (size_t)lds_blocks * A;
        if ((rc = sc_ensure(ctx, ctx->bs_blk, sizeof(int) * ((size_t)NBc + 1)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->bs_sblk, sizeof(int) * ((size_t)Sc + 1)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->bs_terms, sizeof(double2) * (size_t)NBc * A))) return rc;
        if ((rc = sc_lds_attr(ctx, (const void*)k_bs_reps, lds))) return rc;
        d_blk = (int*)ctx->bs_blk.p;
        d_sblk = (int*)ctx->bs_sblk.p;
        d_terms = (double2*)ctx->bs_terms.p;
        SC_HIP(ctx, hipMemcpyAsync(d_blk, blk.data(), sizeof(int) * ((size_t)NBc + 1), hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(d_sblk, sblk.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
        return SC_OK;
    };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const size_t mA = (size_t)st.m * A;
        const int tiles = (R + 1 + BS_WAVES * BS_TILE - 1) / (BS_WAVES * BS_TILE);
        signed char* d_index = (signed char*)k.out[2];
        double* d_a = (double*)k.out[3];
        int launches = sc_sg_stage_launch(ctx, z, ny, nx, A, h, w, Ds, de, min_samples, k.tab, st);
        if (NBc) {
            sc_bs_terms_launch(ctx, st.used, st.planes + 2 * mA, st.planes + 3 * mA, d_blk, NBc, A, d_terms);
            ++launches;
        }
        k_bs_reps<<<bs_grid(st.Sc * tiles), BS_THREADS, lds, ctx->stream>>>(d_sblk, st.label, st.cnt, d_terms, st.Sc, A, R, seed,
                                                                           min_blocks, min_profiles, lds_blocks, d_index, d_a);
        k_bs_summary<<<bs_grid(st.Sc), BS_THREADS, 0, ctx->stream>>>(st.seg, d_sblk, st.label, st.cnt, k.ages, st.Sc, A, R, level,
                                                                    min_blocks, min_profiles, d_index, d_a, (int*)k.out[1],
                                                                    (sc_segment_boot*)k.out[0]);
        return launches + 2;
    };
    return sc_sg_chunks(ctx, c);
}

// the two calls after their null checks: every refusal, then the bootstrap on the context's DEM (z null) or on z, uploaded
static int bs_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const long long* seg_blk_start, const long long* blk_start, long long NB, const double* ages, int A, int h,
                   int w, int D, double de, int min_samples, int min_profiles, int min_blocks, int R, double level,
                   unsigned long long seed, sc_segment_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    // (the park of a shifted call counts d_ci whatever D is: the limit of sc_fit_segments_shift)
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, D, de, 0.0, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_bs_check(ctx, who, K, seg_start, S, seg_blk_start, blk_start, NB, min_blocks, R, level))) return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return bs_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, seg_blk_start, blk_start, ages, A, h, w, D, de,
                  min_samples, min_profiles, min_blocks, R, level, seed, out_rows, out_hist, out_index, out_a);
}

extern "C" int sc_bootstrap_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                     const long long* seg_start, const int32_t* seg_label, long long S,
                                     const long long* seg_blk_start, const long long* blk_start, long long NB,
                                     const double* ages, int A, int h, int w, int D, double de, int min_samples,
                                     int min_profiles, int min_blocks, int R, double level, uint64_t seed,
                                     sc_segment_boot* out_rows, int32_t* out_hist, int8_t* out_index, double* out_a) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_bootstrap_segments");
    if (rc) return rc;
    return bs_call(ctx, "sc_bootstrap_segments", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S,
                   seg_blk_start, blk_start, NB, ages, A, h, w, D, de, min_samples, min_profiles, min_blocks, R, level, seed,
                   out_rows, out_hist, out_index, out_a);
}

extern "C" int sc_bootstrap_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                         const double* sa, const double* ca, long long K, const long long* seg_start,
                                         const int32_t* seg_label, long long S, const long long* seg_blk_start,
                                         const long long* blk_start, long long NB, const double* ages, int A, int h, int w,
                                         int D, double de, int min_samples, int min_profiles, int min_blocks, int R,
                                         double level, uint64_t seed, sc_segment_boot* out_rows, int32_t* out_hist,
                                         int8_t* out_index, double* out_a) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return bs_call(ctx, "sc_bootstrap_segments_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, seg_blk_start,
                   blk_start, NB, ages, A, h, w, D, de, min_samples, min_profiles, min_blocks, R, level, seed, out_rows,
                   out_hist, out_index, out_a);
}
