// sc_fit_segments_robust*: the joint fit of sc_fit_segments with a weight on every point and a robust loss (docs/segments.md,
// "Weights and robust fits").
//
// The CSR grouping, the usable-profile rule, k_sg_rank and the blocked sum (k_sg_sum1, k_sg_sum2) are sc_segment.hip's;
// every sweep is one of sc_fit.h's weighted ones.  Per cell the park holds the profile, its weights where there is a plane,
// and NINE planes per age: sbar, pbar, beta, ebar, gamma, See, Sep of the profile's latest weighted fit, and (c0, b) of
// the last iterate in which the profile was active.
//   k_sq_partial  one wave per cell: pf_cut / rb_cut (parked), then lanes over the ages: rb_moments and rb_terms with q = u
//   (k_sg_rank, then the blocked sum of See and Sep: a_i of iterate 0)
//   k_sq_loss<0>  one wave per cell: (c0, b) from the segment's a_i, the explicit residuals: sum u r^2 of every age
//   (the blocked sum; loss SC_ROBUST_NONE goes to k_sq_choose from here)
//   k_sq_begin    one wave per segment: ls_index, a_i of iterate 0 kept, the select's state cleared
//   k_sq_hist     8 rounds, most significant digit first: one wave per cell, lanes over the points, |r| at ls_index
//                 recomputed from the park; the digit of every value that carries the prefix found so far is counted in
//                 the wave's LDS histogram and what is not 0 of it added to the segment's 256 bins (integer atomics)
//   k_sq_pick     one wave per segment: the bin that holds the rank, by integer prefix sums; after the last round
//                 sigma = 1.4826 times the value whose bit pattern the eight digits spell
//   k_sq_step     T times, one wave per cell, lanes over the ages: (c0, b) of the previous iterate from the segment's a_i -
//                 a dormant profile keeps its own - then rb_moments and rb_terms with q recomputed in every sweep; a dormant
//                 profile parks +0.0 for See and Sep and NaN for sbar.  An age whose sum See was not > 0 parks NaN: it
//                 stays dead.  (The blocked sum follows every step.)
//   k_sq_loss<L>  (c0, b) of the last iterate, rb_loss: the profile's loss, sum u r^2 and its down-weighted points
//   (the blocked sum of the loss and of sum u r^2)
//   k_sq_choose   one wave per segment: pf_choose on the loss curve, the row, integer sums of n_down and of the dormant
//                 profiles over the segment's cells, the cell table
// No float atomics and no float sum across lanes: the same bytes on every run and for every order of the segments.
// The host side is the park's shape, the kernel choice, and the launches of one chunk handed to sc_sg_chunks
// (sc_segment.hip), with the select's state and histograms as the call's private buffers.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

#define SQ_MAX_SEGS (1ll << 16)          // segments per chunk: bounds the histograms (1 KB a segment)
#define SQ_LDS_BYTES (160 * 1024)        // the LDS of a CU
#define SQ_MAD 1.4826
#define SQ_PLANES SC_SEGMENT_ROBUST_PLANES
// the planes of the park, in units of m A doubles
#define SQ_SBAR 0
#define SQ_PBAR 1
#define SQ_BETA 2
#define SQ_EBAR 3                        // (after the last sweep: the profile's down-weighted points)
#define SQ_GAMMA 4
#define SQ_SEE 5                         // (after a loss sweep: the profile's loss)
#define SQ_SEP 6                         // (after a loss sweep: the profile's sum u r^2)
#define SQ_C0 7
#define SQ_B 8

// the state of a segment between the kernels
struct sq_state {
    double* sigma;                       // NaN until the scale is known
    unsigned long long* prefix;          // the digits found so far, from the top
    int* st;                             // 0: iterating; 1: not fitted; 16: no scale; 33: no age survived iterate 0
    int* ls;                             // ls_index
    int* rank;                           // the rank still looked for among the values that carry the prefix
};

__device__ __forceinline__ void sq_store_terms(double* __restrict__ planes, size_t stride, size_t o, const rb_par& t) {
    planes[SQ_SBAR * stride + o] = t.sbar;
    planes[SQ_PBAR * stride + o] = t.pbar;
    planes[SQ_BETA * stride + o] = t.beta;
    planes[SQ_EBAR * stride + o] = t.ebar;
    planes[SQ_GAMMA * stride + o] = t.gamma;
    planes[SQ_SEE * stride + o] = t.See;
    planes[SQ_SEP * stride + o] = t.Sep;
}

// (c0, b) of a profile's latest fit under the segment's a: formed and parked where the profile was active in it (sbar is
// not NaN), read back where it was dormant
__device__ __forceinline__ void sq_line(double* __restrict__ planes, size_t stride, size_t o, bool write, double a, double& b,
                                        double& c0) {
    const double sbar = planes[SQ_SBAR * stride + o];
    if (sbar == sbar) {
        pf_slope(sbar, planes[SQ_PBAR * stride + o], planes[SQ_BETA * stride + o], planes[SQ_EBAR * stride + o],
                 planes[SQ_GAMMA * stride + o], a, b, c0);
        if (write) {
            planes[SQ_C0 * stride + o] = c0;
            planes[SQ_B * stride + o] = b;
        }
    } else {
        c0 = planes[SQ_C0 * stride + o];
        b = planes[SQ_B * stride + o];
    }
}

template <bool TAB_LDS, bool WT>
__global__ __launch_bounds__(PF_THREADS) void k_sq_partial(const double* __restrict__ z, const double* __restrict__ wt, int ny,
                                                           int nx, const long long* __restrict__ cells,
                                                           const double* __restrict__ dir, long long K, int A, int h, int w,
                                                           double de, int min_samples, const double* __restrict__ tab_g,
                                                           double* __restrict__ prof_g, double* __restrict__ u_g,
                                                           int* __restrict__ cn, int* __restrict__ used,
                                                           double* __restrict__ planes) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, WT ? 2 * np : np, np, A);
    double* prof = L.prof;
    double* u = WT ? L.prof + np : nullptr;
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double* col = L.tab + ia;
    const size_t stride = (size_t)K * A;
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        if (act) {
            if (WT) rb_cut(z, wt, ny, nx, cells[kc], dir, kc, h, w, lane, prof, u, prof_g, u_g);
            else pf_cut(z, ny, nx, cells[kc], dir, kc, h, w, lane, prof, prof_g);
        }
        __syncthreads();
        if (act) {
            const rb_prev none = {0.0, 0.0, 0.0, 0.0};
            const rb_mom mo = rb_moments<0, WT>(prof, u, np, h, de, col, A, none);
            const bool ok = mo.n_neg >= min_samples && mo.n_pos >= min_samples;
            if (lane == 0) {
                cn[kc] = mo.n;
                used[kc] = ok ? 1 : 0;
            }
            if (ok) {
                const rb_par t = rb_terms<0, WT>(prof, u, np, h, de, col, A, none, mo);
                if (lane < A) sq_store_terms(planes, stride, (size_t)kc * A + lane, t);
            }
        }
        __syncthreads();
    }
}

// One iterate: the previous fit's (c0, b, a) of every age, then the weighted terms under q = u f(|r|).  tot: the blocked sums
// of See and Sep of the previous iterate; check: that iterate was not iterate 0, whose a is taken as it comes
template <bool TAB_LDS, bool WT, int LOSS>
__global__ __launch_bounds__(PF_THREADS) void k_sq_step(const double* __restrict__ prof_g, const double* __restrict__ u_g,
                                                        const int* __restrict__ cseg, const int* __restrict__ used,
                                                        sq_state S, const double* __restrict__ tot,
                                                        double* __restrict__ planes, long long K, int A, int h, double de,
                                                        int min_samples, double tuning, int check,
                                                        const double* __restrict__ tab_g) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, WT ? 2 * np : np, np, A);
    double* prof = L.prof;
    double* u = WT ? L.prof + np : nullptr;
    const int ia = min(lane, A - 1);
    const double* col = L.tab + ia;
    const size_t stride = (size_t)K * A;
    const double nan = __builtin_nan("");
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        bool act = kc < K;
        int s = 0;
        if (act) {
            s = cseg[kc];
            act = used[kc] != 0 && S.st[s] == 0;
        }
        if (act) pf_fetch<WT>(prof_g, u_g, kc, np, lane, prof, u);
        __syncthreads();
        if (act) {
            const size_t o = (size_t)kc * A + ia;
            const double See = tot[((size_t)s * 2) * A + ia], Sep = tot[((size_t)s * 2 + 1) * A + ia];
            if (check && !(See > 0.0)) {                 // a dead age stays dead: its sums are NaN from here on
                if (lane < A) {
                    planes[SQ_SEE * stride + o] = nan;
                    planes[SQ_SEP * stride + o] = nan;
                }
            } else {
                rb_prev v;
                v.a = Sep / See;
                v.c = tuning * S.sigma[s];
                sq_line(planes, stride, o, lane < A, v.a, v.b, v.c0);
                const rb_mom mq = rb_moments<LOSS, WT>(prof, u, np, h, de, col, A, v);
                if (mq.n_neg < min_samples || mq.n_pos < min_samples) {           // dormant: no say in a_i
                    if (lane < A) {
                        planes[SQ_SBAR * stride + o] = nan;
                        planes[SQ_SEE * stride + o] = 0.0;
                        planes[SQ_SEP * stride + o] = 0.0;
                    }
                } else {
                    const rb_par t = rb_terms<LOSS, WT>(prof, u, np, h, de, col, A, v, mq);
                    if (lane < A) sq_store_terms(planes, stride, o, t);
                }
            }
        }
        __syncthreads();
    }
}

// The last sweep of a fit: (c0, b) under the segment's a_i, then the profile's loss (in place of See), its sum u r^2 (in
// place of Sep) and, with a robust loss, its points with f < 1 (in place of ebar).  LOSS 0: iterate 0, on every fitted
// segment; else the last iterate, on the segments still iterating
template <bool TAB_LDS, bool WT, int LOSS>
__global__ __launch_bounds__(PF_THREADS) void k_sq_loss(const double* __restrict__ prof_g, const double* __restrict__ u_g,
                                                        const int* __restrict__ cseg, const int* __restrict__ used,
                                                        const int* __restrict__ cnt, sq_state S,
                                                        const double* __restrict__ tot, double* __restrict__ planes,
                                                        long long K, int A, int h, double de, int min_profiles, double tuning,
                                                        const double* __restrict__ tab_g) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, WT ? 2 * np : np, np, A);
    double* prof = L.prof;
    double* u = WT ? L.prof + np : nullptr;
    const int ia = min(lane, A - 1);
    const double* col = L.tab + ia;
    const size_t stride = (size_t)K * A;
    const double nan = __builtin_nan("");
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        bool act = kc < K;
        int s = 0;
        if (act) {
            s = cseg[kc];
            const int m = cnt[2 * s];
            act = used[kc] != 0 && (LOSS ? S.st[s] == 0 : sg_fitted(m, sg_dof(m, cnt[2 * s + 1], 0), min_profiles));
        }
        if (act) pf_fetch<WT>(prof_g, u_g, kc, np, lane, prof, u);
        __syncthreads();
        if (act) {
            const size_t o = (size_t)kc * A + ia;
            const double See = tot[((size_t)s * 2) * A + ia], Sep = tot[((size_t)s * 2 + 1) * A + ia];
            double sse = nan, loss = nan;
            int n_down = 0;
            if (!LOSS || See > 0.0) {
                rb_prev v;
                v.a = Sep / See;
                v.c = LOSS ? tuning * S.sigma[s] : 0.0;
                sq_line(planes, stride, o, lane < A, v.a, v.b, v.c0);
                rb_loss<LOSS, WT>(prof, u, np, h, de, col, A, v, sse, loss, n_down);
            }
            if (lane < A) {
                planes[SQ_SEE * stride + o] = loss;
                planes[SQ_SEP * stride + o] = sse;
                if (LOSS) planes[SQ_EBAR * stride + o] = (double)n_down;
            }
        }
        __syncthreads();
    }
}

// after iterate 0: the segment's state, ls_index, a_i of iterate 0 (the row of a segment without a scale needs it after
// the iterates have reused tot) and the select's start.  tl: the blocked sums of (loss, sum u r^2) of iterate 0
__global__ __launch_bounds__(64) void k_sq_begin(const int* __restrict__ cnt, long long Sn, const double* __restrict__ tot,
                                                 const double* __restrict__ tl, int A, double delta, int min_profiles,
                                                 double scale_in, sq_state S, int* __restrict__ hist,
                                                 double* __restrict__ a0) {
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);
    for (long long s = blockIdx.x; s < Sn; s += gridDim.x) {
        const int m = cnt[2 * s], n = cnt[2 * s + 1];
        const int dof = sg_dof(m, n, 0);
        int state = 1, ls = -1;
        if (sg_fitted(m, dof, min_profiles)) {
            const double sse = tl[((size_t)s * 2 + 1) * A + ia];
            if (lane < A) a0[s * A + lane] = tot[((size_t)s * 2 + 1) * A + lane] / tot[((size_t)s * 2) * A + lane];
            if (__ballot(lane < A && sse == sse) == 0ull) {
                state = 1 | 32;
            } else {
                state = 0;
                ls = pf_choose(sse, lane, A, delta, dof).best;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) hist[s * 256 + 4 * lane + q] = 0;
        if (lane == 0) {
            S.st[s] = state;
            S.ls[s] = ls;
            S.rank[s] = (n - 1) / 2;
            S.prefix[s] = 0ull;
            S.sigma[s] = (state == 0 && scale_in > 0.0) ? scale_in : __builtin_nan("");
        }
    }
}

// One round of the select: digit `round` (0: the top 8 bits) of the bit patterns of |r| at ls_index, over the points of the
// usable profiles of the segments still iterating, among the values that carry the prefix found so far
__global__ __launch_bounds__(PF_THREADS) void k_sq_hist(const double* __restrict__ prof_g, const int* __restrict__ cseg,
                                                        const int* __restrict__ used, sq_state S,
                                                        const double* __restrict__ a0, const double* __restrict__ planes,
                                                        long long K, int A, int h, double de, int round,
                                                        const double* __restrict__ tab_g, int* __restrict__ hist) {
    __shared__ int bins[PF_WAVES][256];
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int shift = 56 - 8 * round;
    const size_t stride = (size_t)K * A;
    int* mine = bins[wave];
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        bool act = kc < K;
        int s = 0;
        if (act) {
            s = cseg[kc];
            act = used[kc] != 0 && S.st[s] == 0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) mine[lane + 64 * q] = 0;
        __syncthreads();
        if (act) {
            const int ls = S.ls[s];
            const size_t o = (size_t)kc * A + ls;
            rb_prev v;
            v.a = a0[(size_t)s * A + ls];
            v.c0 = planes[SQ_C0 * stride + o];
            v.b = planes[SQ_B * stride + o];
            v.c = 0.0;
            const unsigned long long prefix = S.prefix[s];
            const double* col = tab_g + ls;
            for (int jj = lane; jj < np; jj += 64) {
                const double p = prof_g[(size_t)kc * np + jj];
                if (p != p) continue;
                const double x = fabs(rb_resid(p, (double)(jj - h) * de, col[(size_t)jj * A], v));
                const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
                if (round == 0 || (bits >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&mine[(int)((bits >> shift) & 255ull)], 1);
            }
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = mine[lane + 64 * q];
                if (c) atomicAdd(&hist[(size_t)s * 256 + lane + 64 * q], c);
            }
        }
        __syncthreads();
    }
}

// ... and the bin that holds the rank; the bins are cleared for the next round.  After round 7 the prefix is the element
__global__ __launch_bounds__(64) void k_sq_pick(long long Sn, sq_state S, int round, int* __restrict__ hist) {
    const int lane = threadIdx.x;
    const int shift = 56 - 8 * round;
    for (long long s = blockIdx.x; s < Sn; s += gridDim.x) {
        if (S.st[s] != 0) continue;                      // (uniform per wave)
        const int rank = S.rank[s];
        const unsigned long long prefix = S.prefix[s];
        int c[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            c[q] = hist[(size_t)s * 256 + 4 * lane + q];
            hist[(size_t)s * 256 + 4 * lane + q] = 0;
            sum += c[q];
        }
        int incl = sum;                                  // inclusive prefix sum over the lanes (integers)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        int before = incl - sum, digit = -1, left = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (digit < 0 && rank >= before && rank < before + c[q]) {
                digit = 4 * lane + q;
                left = rank - before;
            }
            before += c[q];
        }
        const unsigned long long found = __ballot(digit >= 0);
        if (found == 0ull) continue;                     // (cannot happen: the bins hold more than `rank` values)
        const int src = __ffsll((long long)found) - 1;
        digit = __shfl(digit, src, 64);
        left = __shfl(left, src, 64);
        if (lane == 0) {
            const unsigned long long next = prefix | ((unsigned long long)digit << shift);
            S.prefix[s] = next;
            S.rank[s] = left;
            if (round == 7) {
                const double sigma = SQ_MAD * __longlong_as_double((long long)next);
                S.sigma[s] = sigma;
                if (!(sigma > 0.0)) S.st[s] = 16;        // no scale: the row of iterate 0
            }
        }
    }
}

// The age of each segment, its interval and its row; the cell table at the best age.  tl: the blocked sums of (loss, sum u
// r^2) of the last sweep; S.st null: loss SC_ROBUST_NONE, where tot still holds iterate 0
template <bool ROBUST>
__global__ __launch_bounds__(64) void k_sq_choose(const int* __restrict__ seg_start, const int* __restrict__ label,
                                                  const int* __restrict__ cnt, long long Sn, long long K,
                                                  const double* __restrict__ tot, const double* __restrict__ tl,
                                                  const double* __restrict__ a0, sq_state S, const double* __restrict__ ages,
                                                  int A, double delta, int min_profiles, const long long* __restrict__ cells,
                                                  const int* __restrict__ cn, const int* __restrict__ used,
                                                  const double* __restrict__ planes, sc_segment_robust_fit* __restrict__ rows,
                                                  sc_segment_robust_cell* __restrict__ out_cells, double* __restrict__ curve) {
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);
    const double nan = __builtin_nan("");
    const size_t stride = (size_t)K * A;
    for (long long s = blockIdx.x; s < Sn; s += gridDim.x) {
        const int start = seg_start[s], end = seg_start[s + 1];
        const int m = cnt[2 * s], n = cnt[2 * s + 1];
        const int dof = sg_dof(m, n, 0);
        int state = ROBUST ? S.st[s] : (sg_fitted(m, dof, min_profiles) ? 0 : 1);
        const double sigma = ROBUST ? S.sigma[s] : nan;
        double loss = nan, sse = nan, a = nan;
        if (state == 0 || state == 16) {
            loss = tl[((size_t)s * 2) * A + ia];
            sse = tl[((size_t)s * 2 + 1) * A + ia];
            a = (ROBUST && state == 16) ? a0[s * A + ia] : tot[((size_t)s * 2 + 1) * A + ia] / tot[((size_t)s * 2) * A + ia];
            if (__ballot(lane < A && loss == loss) == 0ull) state = 1 | 32;       // no age survived
        }
        const bool fitted = state == 0 || state == 16;
        const bool iterated = ROBUST && state == 0;      // the robust weights of the last iterate are behind the row
        pf_pick k = {-1, -1, -1, nan};
        int best = 0;
        if (fitted) {
            k = pf_choose(loss, lane, A, delta, dof);
            best = k.best;
        }
        if (curve && lane < A) curve[s * A + lane] = fitted ? loss : nan;
        // the down-weighted points and the dormant profiles of the best age's fit: integer sums, any order
        int n_down = 0, n_dormant = 0;
        if (iterated) {
            for (int c = start + lane; c < end; c += 64) {
                if (!used[c]) continue;
                const size_t o = (size_t)c * A + best;
                n_down += (int)planes[SQ_EBAR * stride + o];
                const double sbar = planes[SQ_SBAR * stride + o];
                n_dormant += sbar != sbar ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                n_down += __shfl_xor(n_down, o, 64);
                n_dormant += __shfl_xor(n_dormant, o, 64);
            }
        }
        // (the rows were cleared: their padding is part of what the caller compares)
        sc_segment_robust_fit* out = rows + s;
        if (lane == best) {
            out->label = label[s];
            out->n_cells = end - start;
            out->n_profiles = m;
            out->n = n;
            out->dof = dof;
            out->kt_index = k.best;
            out->lo_index = k.lo;
            out->hi_index = k.hi;
            out->status = fitted ? pf_open(k, A) + (state == 16 ? 16 : 0) : state;
            out->kt = fitted ? ages[k.best] : nan;
            out->kt_lo = fitted ? ages[k.lo] : nan;
            out->kt_hi = fitted ? ages[k.hi] : nan;
            out->a = fitted ? a : nan;
            out->sse = fitted ? sse : nan;
            out->rmse = fitted ? sqrt(loss / (double)dof) : nan;
            out->loss = fitted ? loss : nan;
            out->scale = sigma;
            out->n_down = n_down;
            out->ls_index = !fitted ? -1 : (ROBUST ? S.ls[s] : k.best);
            out->n_dormant = n_dormant;
        }
        if (!out_cells) continue;
        for (int c = start + lane; c < end; c += 64) {
            sc_segment_robust_cell* oc = out_cells + c;
            const int u = used[c];
            double b = nan, c0 = nan, csse = nan, closs = nan;
            int down = 0, dormant = 0;
            if (fitted && u) {
                const size_t o = (size_t)c * A + best;
                // ((c0, b) as the last sweep parked them: pf_slope on the parked terms under the segment's a)
                b = planes[SQ_B * stride + o];
                c0 = planes[SQ_C0 * stride + o];
                closs = planes[SQ_SEE * stride + o];
                csse = planes[SQ_SEP * stride + o];
                if (iterated) {
                    down = (int)planes[SQ_EBAR * stride + o];
                    const double sbar = planes[SQ_SBAR * stride + o];
                    dormant = sbar != sbar ? 1 : 0;
                }
            }
            oc->cell = cells[c];
            oc->used = u;
            oc->n = cn[c];
            oc->b = b; oc->c0 = c0; oc->sse = csse; oc->loss = closs;
            oc->n_down = down;
            oc->dormant = dormant;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the park: the weights behind the profiles where there is a plane, nine planes for sc_fit_segments' four -
// 8 ((2h + 1)(1 + plane) + 9 A) bytes a cell
static sg_park sq_park(int A, int h, bool plane) { return {(2 * h + 1) * (plane ? 2 : 1), SQ_PLANES, A, false}; }

typedef void (*sq_partial_kernel)(const double*, const double*, int, int, const long long*, const double*, long long, int, int, int,
                                  double, int, const double*, double*, double*, int*, int*, double*);
typedef void (*sq_step_kernel)(const double*, const double*, const int*, const int*, sq_state, const double*, double*, long long,
                               int, int, double, int, double, int, const double*);
typedef void (*sq_loss_kernel)(const double*, const double*, const int*, const int*, const int*, sq_state, const double*, double*,
                               long long, int, int, double, int, double, const double*);

template <bool TAB_LDS, bool WT>
static sq_step_kernel sq_step_of(int loss) {
    return loss == SC_ROBUST_TUKEY ? k_sq_step<TAB_LDS, WT, 2> : k_sq_step<TAB_LDS, WT, 1>;
}
template <bool TAB_LDS, bool WT>
static sq_loss_kernel sq_loss_of(int loss) {
    return loss == SC_ROBUST_TUKEY ? k_sq_loss<TAB_LDS, WT, 2> : loss == SC_ROBUST_HUBER ? k_sq_loss<TAB_LDS, WT, 1> : k_sq_loss<TAB_LDS, WT, 0>;
}

static int sq_run(sc_ctx* ctx, const double* z, const double* wt, int ny, int nx, const long long* cells, const double* sa,
                  const double* ca, const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                  int h, int w, double de, double delta, int min_samples, int min_profiles, int loss, double tuning,
                  int iterations, double scale, sc_segment_robust_fit* out_rows, sc_segment_robust_cell* out_cells,
                  double* out_loss) {
    if (S == 0) return SC_OK;
    const bool robust = loss != SC_ROBUST_NONE, plane = wt != nullptr;
    const int np = 2 * h + 1, np2 = plane ? 2 * np : np;
    const size_t tab_bytes = sizeof(double) * (size_t)np * A;
    int rc;
    // (the profiles and their weights come first: the table goes to LDS only where the CU still holds it beside them)
    const bool tab_lds = tab_bytes <= PF_TAB_LDS && pf_lds_bytes(np2, np, A, false, true) <= SQ_LDS_BYTES;
    const size_t lds = pf_lds_bytes(np2, np, A, false, tab_lds);
    const sq_partial_kernel k_partial = tab_lds ? (plane ? k_sq_partial<true, true> : k_sq_partial<true, false>)
                                                : (plane ? k_sq_partial<false, true> : k_sq_partial<false, false>);
    const sq_loss_kernel k_loss0 = tab_lds ? (plane ? sq_loss_of<true, true>(0) : sq_loss_of<true, false>(0))
                                           : (plane ? sq_loss_of<false, true>(0) : sq_loss_of<false, false>(0));
    const sq_loss_kernel k_lossT = tab_lds ? (plane ? sq_loss_of<true, true>(loss) : sq_loss_of<true, false>(loss))
                                           : (plane ? sq_loss_of<false, true>(loss) : sq_loss_of<false, false>(loss));
    const sq_step_kernel k_step = tab_lds ? (plane ? sq_step_of<true, true>(loss) : sq_step_of<true, false>(loss))
                                          : (plane ? sq_step_of<false, true>(loss) : sq_step_of<false, false>(loss));
    if ((rc = sc_lds_attr(ctx, (const void*)k_partial, lds))) return rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_loss0, lds))) return rc;
    if (robust && (rc = sc_lds_attr(ctx, (const void*)k_lossT, lds))) return rc;
    if (robust && (rc = sc_lds_attr(ctx, (const void*)k_step, lds))) return rc;
    const auto k_choose = robust ? k_sq_choose<true> : k_sq_choose<false>;

    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, h, de, sq_park(A, h, plane), SQ_MAX_SEGS, nullptr, 0, 2};
    c.out = {{out_rows, &ctx->sg_rows, sizeof(sc_segment_robust_fit), SG_SEGS, true},
             {out_cells, &ctx->sg_out, sizeof(sc_segment_robust_cell), SG_CELLS},
             {out_loss, &ctx->sg_sse, sizeof(double) * A, SG_SEGS}};
    double* d_a0 = nullptr;
    int* d_hist = nullptr;
    sq_state Q = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (robust) c.prepare = [&](const sg_chunk& k) {
        const long long Sc = k.st.Sc;
        if ((rc = sc_ensure(ctx, ctx->sq_state, (size_t)Sc * (2 * sizeof(double) + 3 * sizeof(int))))) return rc;
        if ((rc = sc_ensure(ctx, ctx->sq_hist, sizeof(int) * 256 * (size_t)Sc))) return rc;
        if ((rc = sc_ensure(ctx, ctx->sq_a, sizeof(double) * (size_t)Sc * A))) return rc;
        Q.sigma = (double*)ctx->sq_state.p;
        Q.prefix = (unsigned long long*)(Q.sigma + Sc);
        Q.st = (int*)(Q.prefix + Sc);
        Q.ls = Q.st + Sc;
        Q.rank = Q.ls + Sc;
        d_hist = (int*)ctx->sq_hist.p;
        d_a0 = (double*)ctx->sq_a.p;
        return SC_OK;
    };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const long long Sc = st.Sc, m = st.m, G = k.G;
        const size_t mA = (size_t)m * A;
        double* d_u = plane ? st.prof + (size_t)m * np : nullptr;
        double *d_part = k.part, *d_tot = k.tot, *d_tl = k.tsum;        // (tl: the loss and sum u r^2 of the last sweep)
        const unsigned gcell = pf_grid(m);
        int launches = 0;
        if (m) {
            k_partial<<<gcell, PF_THREADS, lds, ctx->stream>>>(z, wt, ny, nx, st.cells, st.dirs, m, A, h, w, de, min_samples, k.tab, st.prof,
                                                              d_u, st.cn, st.used, st.planes);
            ++launches;
        }
        sc_sg_rank_launch(ctx, st);
        ++launches;
        if (G) {
            sc_sg_sum_launch(ctx, st.planes + SQ_SEE * mA, st, k.blk, G, A, 2, d_part, d_tot);
            k_loss0<<<gcell, PF_THREADS, lds, ctx->stream>>>(st.prof, d_u, k.cseg, st.used, st.cnt, Q, d_tot, st.planes, m, A, h, de,
                                                            min_profiles, 0.0, k.tab);
            sc_sg_sum_launch(ctx, st.planes + SQ_SEE * mA, st, k.blk, G, A, 2, d_part, d_tl);
            launches += 5;
        }
        if (robust) {
            k_sq_begin<<<sg_grid(Sc), 64, 0, ctx->stream>>>(st.cnt, Sc, d_tot, d_tl, A, delta, min_profiles, scale, Q, d_hist, d_a0);
            ++launches;
            if (G && !(scale > 0.0)) {
                for (int r = 0; r < 8; ++r) {
                    k_sq_hist<<<gcell, PF_THREADS, 0, ctx->stream>>>(st.prof, k.cseg, st.used, Q, d_a0, st.planes, m, A, h, de, r, k.tab,
                                                                    d_hist);
                    k_sq_pick<<<sg_grid(Sc), 64, 0, ctx->stream>>>(Sc, Q, r, d_hist);
                }
                launches += 16;
            }
            if (G) {
                for (int t = 0; t < iterations; ++t) {
                    k_step<<<gcell, PF_THREADS, lds, ctx->stream>>>(st.prof, d_u, k.cseg, st.used, Q, d_tot, st.planes, m, A, h, de,
                                                                   min_samples, tuning, t > 0 ? 1 : 0, k.tab);
                    sc_sg_sum_launch(ctx, st.planes + SQ_SEE * mA, st, k.blk, G, A, 2, d_part, d_tot);
                }
                k_lossT<<<gcell, PF_THREADS, lds, ctx->stream>>>(st.prof, d_u, k.cseg, st.used, st.cnt, Q, d_tot, st.planes, m, A, h, de,
                                                                min_profiles, tuning, k.tab);
                sc_sg_sum_launch(ctx, st.planes + SQ_SEE * mA, st, k.blk, G, A, 2, d_part, d_tl);
                launches += 3 * iterations + 3;
            }
        }
        k_choose<<<sg_grid(Sc), 64, 0, ctx->stream>>>(st.seg, st.label, st.cnt, Sc, m, d_tot, d_tl, d_a0, Q, k.ages, A, delta, min_profiles,
                                                     st.cells, st.cn, st.used, st.planes, (sc_segment_robust_fit*)k.out[0],
                                                     (sc_segment_robust_cell*)k.out[1], (double*)k.out[2]);
        return launches + 1;
    };
    return sc_sg_chunks(ctx, c);
}

// The two calls after their null checks: the argument checks, then the fit on z - ny x nx on the host, uploaded - or on
// the context's DEM (z null); the weight plane, where there is one, is uploaded either way.
static int sq_call(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                   long long K, const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                   int h, int w, double de, double delta, int min_samples, int min_profiles, const double* weights, int loss,
                   double tuning, int iterations, double scale, sc_segment_robust_fit* out_rows,
                   sc_segment_robust_cell* out_cells, double* out_loss) {
    const char* who = "sc_fit_segments_robust";
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, -1, de, delta, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_rb_check(ctx, who, loss, tuning, iterations, scale))) return rc;
    if ((rc = sc_sg_check_cap(ctx, who, seg_start, S, sc_sg_cap_cells(sq_park(A, h, weights != nullptr)), "at this h and A")))
        return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    const double* w_dev = nullptr;
    if (weights && S > 0) {
        if ((rc = sc_pf_upload(ctx, ctx->sq_wt, weights, ny, nx))) return rc;
        w_dev = (const double*)ctx->sq_wt.p;
    }
    return sq_run(ctx, z_dev, w_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, ages, A, h, w, de, delta, min_samples,
                  min_profiles, loss, tuning, iterations, scale, out_rows, out_cells, out_loss);
}

extern "C" int sc_fit_segments_robust(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                      const long long* seg_start, const int32_t* seg_label, long long S, const double* ages,
                                      int A, int h, int w, double de, double delta, int min_samples, int min_profiles,
                                      const double* weights, int loss, double tuning, int iterations, double scale,
                                      sc_segment_robust_fit* out_rows, sc_segment_robust_cell* out_cells, double* out_loss) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_segments_robust");
    if (rc) return rc;
    return sq_call(ctx, nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, de, delta,
                   min_samples, min_profiles, weights, loss, tuning, iterations, scale, out_rows, out_cells, out_loss);
}

// (reports as sc_fit_segments_robust)
extern "C" int sc_fit_segments_robust_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                          const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                          long long S, const double* ages, int A, int h, int w, double de, double delta,
                                          int min_samples, int min_profiles, const double* weights, int loss, double tuning,
                                          int iterations, double scale, sc_segment_robust_fit* out_rows,
                                          sc_segment_robust_cell* out_cells, double* out_loss) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return sq_call(ctx, z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, de, delta, min_samples, min_profiles,
                   weights, loss, tuning, iterations, scale, out_rows, out_cells, out_loss);
}
