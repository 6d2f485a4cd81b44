// sc_fit_segments*: one scarp age per trace segment, fitted jointly (docs/segments.md).
//
// The cells arrive grouped by segment (CSR seg_start).  Per segment and age one least-squares problem over all its
// usable profiles: a shared amplitude a, and an intercept and a slope per profile.  Orthogonalising each profile's erf
// column and data against its own (1, s) - passes 0 to 2 of the fit, sc_fit.h - leaves a one-column problem whose
// normal equation is a_i = sum_c Sep_ci / sum_c See_ci; the residuals are then explicit.
//   k_sg_partial  one wave per cell: pf_cut, lanes over the points (the profile goes to LDS and is PARKED in global
//                 memory); then lanes over the ages for pf_moments and pf_line with the lane's column in the same
//                 sweep, and pf_rest.  Parks sbar, pbar, beta and per age ebar, gamma, See, Sep
//   k_sg_shift    sc_fit_segments_shift's k_sg_partial: pf_moments and pf_line without a column, once, then the
//                 lanes run over the (shift, age) pairs (sh_search); parks the same terms AT d_ci, and d_ci itself
//   k_sg_rank     one wave per segment: the usable cells of the segment in input order (ballot and popcount), their
//                 number and the pooled number of valid points
//   k_sg_sum1     one wave per block of 64 consecutive usable profiles and 64 of the C columns, lanes over the columns
//                 (C = A ages here: one wave a block; sc_segment_ramp.hip sums its A (M + 1) pairs): the block's terms
//                 summed in sequence from the first
//   k_sg_sum2     one wave per segment and 64 columns: the block sums in sequence from the first.  The shape of the sum
//                 depends on n_profiles alone; one profile is no addition at all
//   k_sg_resid    one wave per cell: the parked profile back into LDS, lanes over the ages, pf_slope and pf_sse with
//                 the segment's a_i and the column at d_ci (the unshifted call: no d_ci, D = 0); the cell's sse_ci
//                 takes the place of See_ci
//   (k_sg_sum1 and k_sg_sum2 again, on sse_ci)
//   k_sg_choose   one wave per segment: pf_choose, the row; then lanes over the segment's cells for the cell table at
//                 the best age (sc_segment_cell, or sc_segment_shift_cell with d_ci at that age)
// No atomics at all.  The erf table is k_pf_table's: the same bits as sc_fit_profiles*.
// The host side holds the frame of every segment call (sc_fit.h): the argument checks, stage one, the segmented sum and
// sc_sg_chunks, the chunked driver.  A call - sg_run here; sr_run, sq_run, bs_run, st_run, sx_run, cs_run in their files - is the shape of
// its park, its bounds, its list of outputs and the launches of one chunk.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>
#include <type_traits>

#define SG_MAX_SEGS (1ll << 20)          // segments per chunk: bounds the rows and totals of a call with empty segments

// what k_sg_partial and k_sg_shift park of a cell apart from the per-age terms
__device__ __forceinline__ void sg_park_cell(long long kc, int lane, int n, bool ok, int* __restrict__ cn,
                                             int* __restrict__ used) {
    if (lane == 0) {
        cn[kc] = n;
        used[kc] = ok ? 1 : 0;
    }
}
__device__ __forceinline__ void sg_park_line(long long kc, int lane, const pf_lin& f, double* __restrict__ scal) {
    if (lane == 0) {
        scal[3 * kc] = f.sbar;
        scal[3 * kc + 1] = f.pbar;
        scal[3 * kc + 2] = f.beta;
    }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_sg_partial(const double* __restrict__ z, int ny, int nx,
                                                           const long long* __restrict__ cells,
                                                           const double* __restrict__ dir, long long K, int A, int h,
                                                           int w, double de, int min_samples,
                                                           const double* __restrict__ tab_g, double* __restrict__ prof_g,
                                                           int* __restrict__ cn, int* __restrict__ used,
                                                           double* __restrict__ scal, double* __restrict__ planes) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, np, np, A);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double* col = L.tab + ia;
    const size_t stride = (size_t)K * A;                 // one per-cell-and-age plane
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        if (act) pf_cut(z, ny, nx, cells[kc], dir, kc, h, w, lane, L.prof, prof_g);
        __syncthreads();
        if (act) {
            const pf_mom mo = pf_moments<true>(L.prof, np, h, de, col, A);
            const bool ok = mo.n_neg >= min_samples && mo.n_pos >= min_samples;
            sg_park_cell(kc, lane, mo.n, ok, cn, used);
            if (ok) {
                pf_col t;
                const pf_lin f = pf_line<true>(L.prof, np, h, de, mo, col, A, t);
                pf_rest(L.prof, np, h, de, f, pf_at(col, A), t);
                sg_park_line(kc, lane, f, scal);
                if (lane < A) {
                    const size_t o = (size_t)kc * A + lane;
                    planes[o] = t.ebar;
                    planes[stride + o] = t.gamma;
                    planes[2 * stride + o] = t.See;
                    planes[3 * stride + o] = t.Sep;
                }
            }
        }
        __syncthreads();
    }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_sg_shift(const double* __restrict__ z, int ny, int nx,
                                                         const long long* __restrict__ cells,
                                                         const double* __restrict__ dir, long long K, int A, int h, int w,
                                                         int D, double de, int min_samples,
                                                         const double* __restrict__ tab_g, double* __restrict__ prof_g,
                                                         int* __restrict__ cn, int* __restrict__ used,
                                                         double* __restrict__ scal, double* __restrict__ planes,
                                                         signed char* __restrict__ shifts) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, true>(tab_g, np, 2 * (h + D) + 1, A);
    const double* slot = L.slot;
    const int* srank = (const int*)(slot + (size_t)SH_TERMS * A);
    const size_t stride = (size_t)K * A;                 // one per-cell-and-age plane
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        if (act) pf_cut(z, ny, nx, cells[kc], dir, kc, h, w, lane, L.prof, prof_g);
        __syncthreads();
        if (act) {
            // what depends on neither the age nor the shift, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, A);
            const bool ok = mo.n_neg >= min_samples && mo.n_pos >= min_samples;
            sg_park_cell(kc, lane, mo.n, ok, cn, used);
            if (!ok) {
                if (lane < A) shifts[(size_t)kc * A + lane] = 0;
            } else {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, A, t);
                sh_search(L.prof, L.tab, np, h, A, D, de, lane, f, L.slot);
                sg_park_line(kc, lane, f, scal);
                if (lane < A) {
                    const size_t o = (size_t)kc * A + lane;
                    planes[o] = slot[3 * A + lane];
                    planes[stride + o] = slot[4 * A + lane];
                    planes[2 * stride + o] = slot[A + lane];
                    planes[3 * stride + o] = slot[2 * A + lane];
                    shifts[o] = (signed char)sh_shift_of(srank[lane]);
                }
            }
        }
        __syncthreads();
    }
}

// the usable cells of each segment in input order, their number and the pooled number of valid points
__global__ __launch_bounds__(64) void k_sg_rank(const int* __restrict__ seg_start, long long S, const int* __restrict__ cn,
                                                const int* __restrict__ used, int* __restrict__ list,
                                                int* __restrict__ cnt) {
    const int lane = threadIdx.x;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int start = seg_start[s], end = seg_start[s + 1];
        int m = 0, nsum = 0;
        for (int k0 = start; k0 < end; k0 += 64) {
            const int k = k0 + lane;
            const bool u = k < end && used[k] != 0;
            const unsigned long long mask = __ballot(u);
            if (u) {
                list[start + m + __popcll(mask & ((1ull << lane) - 1ull))] = k;
                nsum += cn[k];
            }
            m += __popcll(mask);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) nsum += __shfl_xor(nsum, o, 64);       // (integers: any order)
        if (lane == 0) {
            cnt[2 * s] = m;
            cnt[2 * s + 1] = nsum;
        }
    }
}

// block g of SG_BLOCK consecutive usable profiles of its segment, 64 of the C columns: P planes summed in sequence from
// the first term.  Work item t = g NC + (the chunk of columns); C <= 64 columns are one chunk, NC = 1 and t = g
template <int P>
__global__ __launch_bounds__(64) void k_sg_sum1(const double* __restrict__ src, size_t stride, const int* __restrict__ list,
                                                const int* __restrict__ seg_start, const int* __restrict__ blk_start,
                                                const int* __restrict__ cnt, long long S, long long G, int C,
                                                double* __restrict__ part) {
    const int lane = threadIdx.x;
    const long long NC = (C + 63) / 64;
    for (long long t = blockIdx.x; t < G * NC; t += gridDim.x) {
        const long long g = t / NC;
        const int q = (int)(t - g * NC) * 64 + lane;
        long long lo = 0, hi = S;                        // the segment with blk_start[s] <= g < blk_start[s + 1]
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((long long)blk_start[mid + 1] <= g) lo = mid + 1; else hi = mid;
        }
        const long long s = lo;
        const int m = cnt[2 * s];
        const int r0 = (int)(g - blk_start[s]) * SG_BLOCK;
        if (r0 >= m || q >= C) continue;
        const int r1 = min(m, r0 + SG_BLOCK);
        const int* ls = list + seg_start[s];
        double acc[P];
        {
            const size_t o = (size_t)ls[r0] * C + q;
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = src[p * stride + o];
        }
        for (int r = r0 + 1; r < r1; ++r) {
            const size_t o = (size_t)ls[r] * C + q;
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] += src[p * stride + o];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) part[((size_t)g * P + p) * C + q] = acc[p];
    }
}

// the block sums of each segment in sequence from the first.  Work item t = s NC + (the chunk of columns)
template <int P>
__global__ __launch_bounds__(64) void k_sg_sum2(const double* __restrict__ part, const int* __restrict__ blk_start,
                                                const int* __restrict__ cnt, long long S, int C, double* __restrict__ tot) {
    const int lane = threadIdx.x;
    const long long NC = (C + 63) / 64;
    for (long long t = blockIdx.x; t < S * NC; t += gridDim.x) {
        const long long s = t / NC;
        const int q = (int)(t - s * NC) * 64 + lane;
        const int nb = (cnt[2 * s] + SG_BLOCK - 1) / SG_BLOCK;
        if (nb == 0 || q >= C) continue;
        const size_t g0 = (size_t)blk_start[s];
        double acc[P];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = part[(g0 * P + p) * C + q];
        for (int b = 1; b < nb; ++b) {
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] += part[((g0 + b) * P + p) * C + q];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) tot[((size_t)s * P + p) * C + q] = acc[p];
    }
}

// the explicit residuals of every usable cell of a fitted segment, with the segment's a_i: sse_ci replaces See_ci.  The
// table covers j = -(h + D)..(h + D) and the cell's column at age i is its row j - d_ci; shifts null: d_ci = 0
template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_sg_resid(const double* __restrict__ prof_g, const int* __restrict__ cseg,
                                                         const int* __restrict__ used, const int* __restrict__ cnt,
                                                         const double* __restrict__ scal, double* __restrict__ planes,
                                                         const signed char* __restrict__ shifts,
                                                         const double* __restrict__ tot, long long K, int A, int h, int D,
                                                         double de, int min_profiles, const double* __restrict__ tab_g) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, np, 2 * (h + D) + 1, A);
    const int ia = min(lane, A - 1);
    const size_t stride = (size_t)K * A;
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        bool act = kc < K;
        int s = 0;
        if (act) {
            s = cseg[kc];
            const int m = cnt[2 * s];
            act = used[kc] != 0 && sg_fitted(m, sg_dof(m, cnt[2 * s + 1], D), min_profiles);
        }
        if (act) pf_fetch<false>(prof_g, nullptr, kc, np, lane, L.prof, nullptr);
        __syncthreads();
        if (act) {
            const size_t o = (size_t)kc * A + ia;
            const double See = tot[((size_t)s * 2) * A + ia], Sep = tot[((size_t)s * 2 + 1) * A + ia];
            const double* col = L.tab + (size_t)(D - (shifts ? (int)shifts[o] : 0)) * A + ia;
            const double a = Sep / See;
            double b, c0;
            pf_slope(scal[3 * kc], scal[3 * kc + 1], scal[3 * kc + 2], planes[o], planes[stride + o], a, b, c0);
            const double sse = pf_sse(L.prof, np, h, de, pf_at(col, A), a, b, c0);
            if (lane < A) planes[2 * stride + o] = sse;
        }
        __syncthreads();
    }
}

// the age of each segment, its interval and its row; the cell table at the best age.  CELL: sc_segment_cell, or
// sc_segment_shift_cell with the shift's degrees of freedom, status bit 8 and the cells' d_ci at the best age (the
// call without a shift: D = 0, shifts null).  The rows are sc_segment_fit, or - with CELL sc_segment_fine_cell - the
// sc_segment_fine_fit of sc_segment_refine.hip, whose shared fields are written here and whose fine fields are left alone
template <class CELL> struct sg_row_of { typedef sc_segment_fit type; };
template <> struct sg_row_of<sc_segment_fine_cell> { typedef sc_segment_fine_fit type; };

template <class CELL>
__global__ __launch_bounds__(64) void k_sg_choose(const int* __restrict__ seg_start, const int* __restrict__ label,
                                                  const int* __restrict__ cnt, long long S, long long K,
                                                  const double* __restrict__ tot, const double* __restrict__ tsse,
                                                  const double* __restrict__ ages, int A, int D, double delta,
                                                  int min_profiles, const long long* __restrict__ cells,
                                                  const int* __restrict__ cn, const int* __restrict__ used,
                                                  const double* __restrict__ scal, const double* __restrict__ planes,
                                                  const signed char* __restrict__ shifts,
                                                  typename sg_row_of<CELL>::type* __restrict__ rows,
                                                  CELL* __restrict__ out_cells, double* __restrict__ curve) {
    typedef typename sg_row_of<CELL>::type ROW;
    constexpr bool SHIFT = std::is_same<CELL, sc_segment_shift_cell>::value;
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);
    const double nan = __builtin_nan("");
    const size_t stride = (size_t)K * A;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int start = seg_start[s], end = seg_start[s + 1];
        const int m = cnt[2 * s], n = cnt[2 * s + 1];
        const int dof = sg_dof(m, n, D);
        const bool fitted = sg_fitted(m, dof, min_profiles);
        // (the rows were cleared: their padding is part of what the caller compares)
        ROW* out = rows + s;
        int best = -1;
        double a_best = nan;
        pf_pick k = {-1, -1, -1, nan};
        int status = 1;
        double a = nan, sse = nan;
        if (fitted) {
            sse = tsse[(size_t)s * A + ia];
            a = tot[((size_t)s * 2 + 1) * A + ia] / tot[((size_t)s * 2) * A + ia];
            k = pf_choose(sse, lane, A, delta, dof);
            best = k.best;
            a_best = __shfl(a, best, 64);
            // a usable profile whose shift at the best age sits at the end of the range
            bool at_end = false;
            if (SHIFT && D > 0)
                for (int c = start + lane; c < end; c += 64) {
                    const int d = shifts[(size_t)c * A + best];
                    at_end = at_end || (used[c] != 0 && (d == D || d == -D));
                }
            status = pf_open(k, A) + (__ballot(at_end) != 0ull ? 8 : 0);
        }
        if (curve && lane < A) curve[s * A + lane] = sse;
        if (lane == (fitted ? best : 0)) {
            out->label = label[s];
            out->n_cells = end - start;
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
            out->a = a;
            out->sse = sse;
            out->rmse = fitted ? sqrt(sse / (double)dof) : nan;
        }
        if (!out_cells) continue;
        for (int c = start + lane; c < end; c += 64) {
            // (field by field: sc_segment_shift_cell ends in padding, which the host cleared)
            CELL* oc = out_cells + c;
            const int u = used[c];
            double b = nan, c0 = nan, csse = nan;
            int d = 0;
            if (fitted && u) {
                const size_t o = (size_t)c * A + best;
                pf_slope(scal[3 * c], scal[3 * c + 1], scal[3 * c + 2], planes[o], planes[stride + o], a_best, b, c0);
                csse = planes[2 * stride + o];
                if (SHIFT) d = shifts[o];
            }
            oc->cell = cells[c];
            oc->used = u;
            oc->n = cn[c];
            oc->b = b; oc->c0 = c0; oc->sse = csse;
            if constexpr (SHIFT) oc->shift_index = d;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// (D < 0 throughout the host side: the call without a shift, its kernels and its bytes)
long long sc_sg_cap_cells(const sg_park& park) {
    return sc_fit_park_cap(SC_SEGMENT_MAX_PARK, park.prof, park.planes, park.C, park.shift);
}

int sc_sg_check_cap(sc_ctx* ctx, const char* who, const long long* seg_start, long long S, long long cap, const char* tail) {
    for (long long s = 0; s < S; ++s)
        if (seg_start[s + 1] - seg_start[s] > cap)
            return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a segment of %lld cells, more than %lld %s", who,
                           seg_start[s + 1] - seg_start[s], cap, tail);
    return SC_OK;
}

int sc_sg_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa, const double* ca,
                    long long K, const long long* seg_start, const int32_t* seg_label, long long S, const double* ages,
                    int A, int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                    const void* out_rows) {
    int rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if (D >= 0 && (rc = sc_pf_check_shift(ctx, who, h, D, min_samples))) return rc;
    if (S < 0 || !seg_start || (S > 0 && (!seg_label || !out_rows)))
        return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (min_profiles < 1) return sc_fail(ctx, SC_ERR_INVALID, "%s: min_profiles must be >= 1", who);
    if (seg_start[0] != 0 || seg_start[S] != K)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_start must run from 0 to K", who);
    for (long long s = 0; s < S; ++s) {
        if (seg_start[s + 1] < seg_start[s])
            return sc_fail(ctx, SC_ERR_INVALID, "%s: seg_start decreases at segment %lld", who, s);
        if (seg_label[s] <= 0 || (s > 0 && seg_label[s] <= seg_label[s - 1]))
            return sc_fail(ctx, SC_ERR_INVALID, "%s: labels must be positive and strictly increasing", who);
    }
    return sc_sg_check_cap(ctx, who, seg_start, S, sc_sg_cap_cells(sg_park_plain(A, h, D >= 0)), "at this h and A");
}


// Stage one of the chunk of whole segments s0..s1: the chunk's cells, (sa, ca), CSR array and labels go up, and the buffers
// of what the parking kernel parks - in the shape of `park` - and k_sg_rank lists are sized.  No launch
static int sg_stage_prepare(sc_ctx* ctx, const sg_call& c, long long s0, long long s1, sg_stage& st) {
    const long long Sc = s1 - s0, k0 = c.seg_start[s0], m = c.seg_start[s1] - k0;
    const size_t mC = (size_t)m * c.park.C;
    int rc;
    st.Sc = Sc;
    st.m = m;
    sc_fit_chunk_start(c.seg_start, s0, s1, st.start);
    sc_fit_chunk_dir(c.sa, c.ca, k0, m, st.dir);
    if ((rc = sc_ensure(ctx, ctx->sg_cells, sizeof(long long) * (size_t)m))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_dir, sizeof(double) * 2 * (size_t)m))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_start, sizeof(int) * ((size_t)Sc + 1)))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_label, sizeof(int) * (size_t)Sc))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_prof, sizeof(double) * (size_t)m * c.park.prof))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_int, sizeof(int) * 2 * (size_t)m))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_scal, sizeof(double) * 3 * (size_t)m))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_age, sizeof(double) * c.park.planes * mC))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_list, sizeof(int) * (size_t)m))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_cnt, sizeof(int) * 2 * (size_t)Sc))) return rc;
    if (c.park.shift && (rc = sc_ensure(ctx, ctx->sg_shift, mC))) return rc;
    st.cells = (long long*)ctx->sg_cells.p;
    st.dirs = (double*)ctx->sg_dir.p;
    st.seg = (int*)ctx->sg_start.p;
    st.label = (int*)ctx->sg_label.p;
    st.prof = (double*)ctx->sg_prof.p;
    st.cn = (int*)ctx->sg_int.p;
    st.used = st.cn + m;
    st.scal = (double*)ctx->sg_scal.p;
    st.planes = (double*)ctx->sg_age.p;
    st.list = (int*)ctx->sg_list.p;
    st.cnt = (int*)ctx->sg_cnt.p;
    st.shift = c.park.shift ? (signed char*)ctx->sg_shift.p : nullptr;
    if (m) {
        SC_HIP(ctx, hipMemcpyAsync(st.cells, c.cells + k0, sizeof(long long) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(st.dirs, st.dir.data(), sizeof(double) * 2 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    }
    SC_HIP(ctx, hipMemcpyAsync(st.seg, st.start.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(st.label, c.seg_label + s0, sizeof(int) * (size_t)Sc, hipMemcpyHostToDevice, ctx->stream));
    return SC_OK;
}

// ... and its two launches, inside the chunk's timing bracket: the parking kernel (none for a chunk without cells) and
// k_sg_rank.  d_tab: the erf table over h + D (h without a shift).  Returns the number of launches
int sc_sg_stage_launch(sc_ctx* ctx, const double* z, int ny, int nx, int A, int h, int w, int D, double de, int min_samples,
                       const double* d_tab, const sg_stage& st) {
    const bool shift = D >= 0;
    const int np = 2 * h + 1, nt = 2 * (h + (shift ? D : 0)) + 1;
    const bool tab_lds = sizeof(double) * (size_t)nt * A <= PF_TAB_LDS;
    const size_t lds1 = pf_lds_bytes(np, nt, A, shift, tab_lds);
    const auto k_partial = tab_lds ? k_sg_partial<true> : k_sg_partial<false>;
    const auto k_shift = tab_lds ? k_sg_shift<true> : k_sg_shift<false>;
    const long long m = st.m;
    const unsigned gcell = pf_grid(m);
    if (m && shift)
        k_shift<<<gcell, PF_THREADS, lds1, ctx->stream>>>(z, ny, nx, st.cells, st.dirs, m, A, h, w, D, de, min_samples, d_tab, st.prof,
                                                         st.cn, st.used, st.scal, st.planes, st.shift);
    else if (m)
        k_partial<<<gcell, PF_THREADS, lds1, ctx->stream>>>(z, ny, nx, st.cells, st.dirs, m, A, h, w, de, min_samples, d_tab, st.prof,
                                                           st.cn, st.used, st.scal, st.planes);
    sc_sg_rank_launch(ctx, st);
    return m ? 2 : 1;
}

void sc_sg_rank_launch(sc_ctx* ctx, const sg_stage& st) {
    k_sg_rank<<<sg_grid(st.Sc), 64, 0, ctx->stream>>>(st.seg, st.Sc, st.cn, st.used, st.list, st.cnt);
}

void sc_sg_sum_launch(sc_ctx* ctx, const double* src, const sg_stage& st, const int* blk, long long G, int C, int P,
                      double* part, double* tot) {
    const size_t mC = (size_t)st.m * C;
    const long long NC = (C + 63) / 64;
    const auto sum1 = P == 2 ? k_sg_sum1<2> : k_sg_sum1<1>;
    const auto sum2 = P == 2 ? k_sg_sum2<2> : k_sg_sum2<1>;
    sum1<<<sg_grid(G * NC), 64, 0, ctx->stream>>>(src, mC, st.list, st.seg, blk, st.cnt, st.Sc, G, C, part);
    sum2<<<sg_grid(st.Sc * NC), 64, 0, ctx->stream>>>(part, blk, st.cnt, st.Sc, C, tot);
}

// the dynamic-LDS limit of the parking kernel, raised before the first chunk
int sc_sg_stage_attr(sc_ctx* ctx, int A, int h, int D) {
    const bool shift = D >= 0;
    const int np = 2 * h + 1, nt = 2 * (h + (shift ? D : 0)) + 1;
    const bool tab_lds = sizeof(double) * (size_t)nt * A <= PF_TAB_LDS;
    const auto k_partial = tab_lds ? k_sg_partial<true> : k_sg_partial<false>;
    const auto k_shift = tab_lds ? k_sg_shift<true> : k_sg_shift<false>;
    return sc_lds_attr(ctx, shift ? (const void*)k_shift : (const void*)k_partial, pf_lds_bytes(np, nt, A, shift, tab_lds));
}

int sc_sg_chunks(sc_ctx* ctx, const sg_call& c) {
    const long long S = c.S;
    const long long* seg_start = c.seg_start;
    const size_t nout = c.out.size();
    int rc;
    if ((rc = sc_ensure(ctx, ctx->sg_ages, sizeof(double) * c.A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sg_tab, sizeof(double) * (size_t)(2 * c.ht + 1) * c.A))) return rc;
    double* d_ages = (double*)ctx->sg_ages.p;
    double* d_tab = (double*)ctx->sg_tab.p;
    SC_HIP(ctx, hipMemcpyAsync(d_ages, c.ages, sizeof(double) * c.A, hipMemcpyHostToDevice, ctx->stream));
    // (rows -h..h of the table over h + D are the bits of the table over h: s = (double)j * de either way)
    if ((rc = sc_pf_table(ctx, d_ages, c.A, c.ht, c.de, d_tab))) return rc;
    if (c.tables && (rc = c.tables(d_ages))) return rc;

    const long long max_cells = sc_fit_chunk_bound(sc_sg_cap_cells(c.park), ctx->fit_chunk);
    sg_stage st;
    std::vector<int> cseg, blk;
    std::vector<void*> d_out(nout);
    for (long long s0 = 0; s0 < S;) {
        // a chunk of whole segments: as many as fit the parked bytes (and the bound on the second CSR array)
        const long long s1 = sc_fit_chunk_end(seg_start, s0, S, c.max_segs, max_cells, c.aux, c.max_aux);
        const long long Sc = s1 - s0, k0 = seg_start[s0], m = seg_start[s1] - k0;
        // where an output of the chunk begins along its axis, and its items
        const auto first = [&](const sg_out& o) { return o.axis == SG_SEGS ? s0 : o.axis == SG_CELLS ? k0 : c.aux[s0]; };
        const auto count = [&](const sg_out& o) { return o.axis == SG_SEGS ? Sc : o.axis == SG_CELLS ? m : c.aux[s1] - c.aux[s0]; };
        if ((rc = sg_stage_prepare(ctx, c, s0, s1, st))) return rc;
        long long G = 0;
        int *d_cseg = nullptr, *d_blk = nullptr;
        double *d_part = nullptr, *d_tot = nullptr, *d_tsum = nullptr;
        if (c.sums) {
            const size_t C = (size_t)c.park.C;
            G = sc_fit_chunk_blocks(seg_start, s0, s1, cseg, blk);
            if ((rc = sc_ensure(ctx, ctx->sg_cseg, sizeof(int) * (size_t)m))) return rc;
            if ((rc = sc_ensure(ctx, ctx->sg_blk, sizeof(int) * ((size_t)Sc + 1)))) return rc;
            if ((rc = sc_ensure(ctx, ctx->sg_part, sizeof(double) * 2 * (size_t)G * C))) return rc;
            if ((rc = sc_ensure(ctx, ctx->sg_tot, sizeof(double) * 2 * (size_t)Sc * C))) return rc;
            if ((rc = sc_ensure(ctx, ctx->sg_tsse, sizeof(double) * c.sums * (size_t)Sc * C))) return rc;
            d_cseg = (int*)ctx->sg_cseg.p;
            d_blk = (int*)ctx->sg_blk.p;
            d_part = (double*)ctx->sg_part.p;
            d_tot = (double*)ctx->sg_tot.p;
            d_tsum = (double*)ctx->sg_tsse.p;
            if (m) SC_HIP(ctx, hipMemcpyAsync(d_cseg, cseg.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
            SC_HIP(ctx, hipMemcpyAsync(d_blk, blk.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
        }
        for (size_t i = 0; i < nout; ++i) {
            const sg_out& o = c.out[i];
            d_out[i] = nullptr;
            if (!o.host && !o.always) continue;
            if ((rc = sc_ensure(ctx, *o.buf, o.item * (size_t)count(o)))) return rc;
            d_out[i] = o.buf->p;
            // (the padding of a row or of a cell of the shifted table is part of what the caller compares: cleared, the
            // kernel writes the fields)
            if (o.clear && count(o)) SC_HIP(ctx, hipMemsetAsync(d_out[i], 0, o.item * (size_t)count(o), ctx->stream));
        }
        const sg_chunk chunk = {st, s0, s1, k0, G, d_cseg, d_blk, d_part, d_tot, d_tsum, d_out, d_ages, d_tab};
        if (c.prepare && (rc = c.prepare(chunk))) return rc;

        sc_prof_begin(ctx, SC_K_PROFILE);
        const int launches = c.launch(chunk);
        if (launches < 0) return launches;
        SC_HIP(ctx, hipGetLastError());
        sc_prof_end(ctx, launches);
        for (size_t i = 0; i < nout; ++i) {
            const sg_out& o = c.out[i];
            if (o.host && count(o))
                SC_HIP(ctx, hipMemcpyAsync((char*)o.host + o.item * (size_t)first(o), d_out[i], o.item * (size_t)count(o),
                                           hipMemcpyDeviceToHost, ctx->stream));
        }
        // (the host arrays are reused by the next chunk, and the caller owns the outputs on return)
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        s0 = s1;
    }
    return SC_OK;
}

// k_sg_resid of a call with the shift range D (D < 0: none), and the dynamic LDS it takes
template <class F>
static auto sg_resid_of(int A, int h, int D, F&& f) {
    const int np = 2 * h + 1, nt = 2 * (h + (D >= 0 ? D : 0)) + 1;
    const bool tab_lds = sizeof(double) * (size_t)nt * A <= PF_TAB_LDS;
    return f(tab_lds ? k_sg_resid<true> : k_sg_resid<false>, pf_lds_bytes(np, nt, A, false, tab_lds));
}

int sc_sg_grid_attr(sc_ctx* ctx, int A, int h, int D) {
    return sg_resid_of(A, h, D, [&](auto k_resid, size_t lds) { return sc_lds_attr(ctx, (const void*)k_resid, lds); });
}

void sc_sg_resid_launch(sc_ctx* ctx, const sg_chunk& k, int A, int h, int D, double de, int min_profiles) {
    const sg_stage& st = k.st;
    sg_resid_of(A, h, D, [&](auto k_resid, size_t lds) {
        k_resid<<<pf_grid(st.m), PF_THREADS, lds, ctx->stream>>>(st.prof, k.cseg, st.used, st.cnt, st.scal, st.planes, st.shift,
                                                                k.tot, st.m, A, h, D >= 0 ? D : 0, de, min_profiles, k.tab);
        return 0;
    });
}

int sc_sg_grid_launch(sc_ctx* ctx, const sg_chunk& k, int A, int h, int D, double de, double delta, int min_profiles, bool fine,
                      void* rows, void* cells, double* curve) {
    const sg_stage& st = k.st;
    const size_t mA = (size_t)st.m * A;
    const int Dk = D >= 0 ? D : 0;                       // what k_sg_resid and k_sg_choose take: no shift is a range of 0
    int launches = 1;
    if (k.G) {
        sc_sg_sum_launch(ctx, st.planes + 2 * mA, st, k.blk, k.G, A, 2, k.part, k.tot);
        sc_sg_resid_launch(ctx, k, A, h, D, de, min_profiles);
        sc_sg_sum_launch(ctx, st.planes + 2 * mA, st, k.blk, k.G, A, 1, k.part, k.tsum);
        launches += 5;
    }
    const auto choose = [&](auto* r, auto* c) {
        k_sg_choose<<<sg_grid(st.Sc), 64, 0, ctx->stream>>>(st.seg, st.label, st.cnt, st.Sc, st.m, k.tot, k.tsum, k.ages, A, Dk, delta,
                                                           min_profiles, st.cells, st.cn, st.used, st.scal, st.planes, st.shift, r,
                                                           c, curve);
    };
    if (fine) choose((sc_segment_fine_fit*)rows, (sc_segment_fine_cell*)cells);
    else if (D >= 0) choose((sc_segment_fit*)rows, (sc_segment_shift_cell*)cells);
    else choose((sc_segment_fit*)rows, (sc_segment_cell*)cells);
    return launches;
}

static int sg_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A, int h,
                  int w, int D, double de, double delta, int min_samples, int min_profiles, sc_segment_fit* out_rows,
                  void* out_cells, double* out_sse, int8_t* out_shift) {
    if (S == 0) return SC_OK;
    const bool shift = D >= 0;
    const int ht = h + (shift ? D : 0);
    const size_t cell_bytes = shift ? sizeof(sc_segment_shift_cell) : sizeof(sc_segment_cell);
    int rc;
    if ((rc = sc_sg_stage_attr(ctx, A, h, D))) return rc;
    if ((rc = sc_sg_grid_attr(ctx, A, h, D))) return rc;

    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, ht, de, sg_park_plain(A, h, shift), SG_MAX_SEGS, nullptr, 0, 1};
    // (the shifted call's cells end in padding; d_ci comes back from where it is parked)
    c.out = {{out_rows, &ctx->sg_rows, sizeof(sc_segment_fit), SG_SEGS, true},
             {out_cells, &ctx->sg_out, cell_bytes, SG_CELLS, shift},
             {out_sse, &ctx->sg_sse, sizeof(double) * A, SG_SEGS},
             {out_shift, &ctx->sg_shift, (size_t)A, SG_CELLS}};
    c.launch = [&](const sg_chunk& k) {
        return sc_sg_stage_launch(ctx, z, ny, nx, A, h, w, D, de, min_samples, k.tab, k.st) +
               sc_sg_grid_launch(ctx, k, A, h, D, de, delta, min_profiles, false, k.out[0], k.out[1], (double*)k.out[2]);
    };
    return sc_sg_chunks(ctx, c);
}

// The four calls after their null checks and the early check of D: the argument checks under the name `who`, then the
// fit on z - ny x nx on the host, uploaded - or on the context's DEM (z null).  D < 0: the call without a shift
static int sg_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                   sc_segment_fit* out_rows, void* out_cells, double* out_sse, int8_t* out_shift) {
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, D, de, delta, min_samples,
                      min_profiles, out_rows);
    if (rc) return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return sg_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, ages, A, h, w, D, de, delta, min_samples,
                  min_profiles, out_rows, out_cells, out_sse, out_shift);
}

extern "C" int sc_fit_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                               const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A,
                               int h, int w, double de, double delta, int min_samples, int min_profiles,
                               sc_segment_fit* out_rows, sc_segment_cell* out_cells, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_segments");
    if (rc) return rc;
    return sg_call(ctx, "sc_fit_segments", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w,
                   -1, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, nullptr);
}

// (reports as sc_fit_segments)
extern "C" int sc_fit_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                   long long S, const double* ages, int A, int h, int w, double de, double delta,
                                   int min_samples, int min_profiles, sc_segment_fit* out_rows, sc_segment_cell* out_cells,
                                   double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return sg_call(ctx, "sc_fit_segments", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, -1, de, delta,
                   min_samples, min_profiles, out_rows, out_cells, out_sse, nullptr);
}

extern "C" int sc_fit_segments_shift(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                     const long long* seg_start, const int32_t* seg_label, long long S, const double* ages,
                                     int A, int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                                     sc_segment_fit* out_rows, sc_segment_shift_cell* out_cells, double* out_sse,
                                     int8_t* out_shift) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_segments_shift");
    if (rc) return rc;
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "sc_fit_segments_shift: the shift range must be >= 0 cells");
    return sg_call(ctx, "sc_fit_segments_shift", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A,
                   h, w, D, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_shift);
}

extern "C" int sc_fit_segments_shift_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                         const double* sa, const double* ca, long long K, const long long* seg_start,
                                         const int32_t* seg_label, long long S, const double* ages, int A, int h, int w,
                                         int D, double de, double delta, int min_samples, int min_profiles,
                                         sc_segment_fit* out_rows, sc_segment_shift_cell* out_cells, double* out_sse,
                                         int8_t* out_shift) {
    if (!ctx || !z) return SC_ERR_INVALID;
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "sc_fit_segments_shift_dem: the shift range must be >= 0 cells");
    return sg_call(ctx, "sc_fit_segments_shift_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, D, de,
                   delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_shift);
}
