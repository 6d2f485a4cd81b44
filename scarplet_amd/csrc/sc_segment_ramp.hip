// sc_fit_segments_ramp*: the initial slope of sl.fit_segments (docs/segments.md, "The initial slope").
//
// The joint fit of sc_fit_segments with the scarp of sc_fit_profiles_ramp: z_c(s) = c0_c + b_c s + a g(s; kt, L), L = m de.
// The amplitude, the age AND the half-width are the segment's, so nothing is searched per profile: every (m, age) pair
// is one column of the joint problem, C = A (M + 1) columns where sc_fit_segments has A.  The pieces are those of sc_fit.h.
//   k_sr_partial  one wave per cell: pf_cut (the profile goes to LDS and is PARKED), pf_moments and pf_line without a
//                 column, once; then the lanes run over the (m, age) pairs, age-minor, 64 a round: pf_column on the erf
//                 table at m = 0 - the plain call's arithmetic -, on the ramp's column (rp_col) of the table of F at m >= 1.  Parks ebar,
//                 gamma, See, Sep of every pair, pair-minor: a round's 64 lanes write 64 neighbouring doubles
//   (k_sg_rank, sc_segment.hip)
//   (k_sg_sum1 and k_sg_sum2, sc_segment.hip, over C columns: one wave per block of 64 consecutive usable profiles - per
//   segment - and 64 columns, the terms summed in sequence from the first)
//   k_sr_resid    one wave per cell: the parked profile back into LDS, lanes over the pairs, pf_slope with the segment's
//                 a_im, then pf_sse on the same columns; sse_cim takes the place of See_cim and b_cim that of Sep_cim
//   (k_sg_sum1 and k_sg_sum2 again, on sse_cim and b_cim)
//   k_sr_choose   one wave per segment, lane i age i: the argmin over m on (key, m) in ascending m - the key is sse_im, or
//                 the distance of the segment's mean initial slope from the given one -, then pf_choose along sse*, the
//                 row, and lanes over the segment's cells for the cell table at the best pair
// The table of F sits in LDS when it fits PF_TAB_LDS bytes, as in k_pf_ramp; the erf table of the m = 0 pairs stays in
// global memory.  No atomics at all, no float sum across lanes.
// The host side is the park's shape (C columns for A), the second table, and the launches of one chunk handed to
// sc_sg_chunks (sc_segment.hip); the chunks are bounded by the totals as well, a second CSR array.  k_sr_resid keeps its
// own lines for the parked profile: with pf_fetch the call measured 0.9 ms of 389 slower in two sessions, at unchanged
// registers (profiles/segment_frame_refactor.txt).
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

#define SR_MAX_SEGS (1ll << 20)          // segments per chunk
#define SR_MAX_TOTALS (1ll << 25)        // (blocks + segments) x columns per chunk: bounds the partials and totals

// the degrees of freedom of a segment of m usable profiles and n pooled points: the free width is the segment's, one
__device__ __forceinline__ int sr_dof(int m, int n, int M, bool given) { return n - 2 * m - 1 - (!given && M > 0 ? 1 : 0); }

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_sr_partial(const double* __restrict__ z, int ny, int nx,
                                                           const long long* __restrict__ cells,
                                                           const double* __restrict__ dir, long long K, int A, int h,
                                                           int w, int M, double de, int min_samples,
                                                           const double* __restrict__ etab,
                                                           const double* __restrict__ ftab_g, double* __restrict__ prof_g,
                                                           int* __restrict__ cn, int* __restrict__ used,
                                                           double* __restrict__ scal, double* __restrict__ planes) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(ftab_g, np, 2 * (h + M) + 1, A);
    const int C = A * (M + 1);
    const size_t stride = (size_t)K * C;                 // one per-cell-and-pair plane
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        if (act) pf_cut(z, ny, nx, cells[kc], dir, kc, h, w, lane, L.prof, prof_g);
        __syncthreads();
        if (act) {
            // what depends on neither the age nor the half-width, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, A);
            const bool ok = mo.n_neg >= min_samples && mo.n_pos >= min_samples;
            if (lane == 0) {
                cn[kc] = mo.n;
                used[kc] = ok ? 1 : 0;
            }
            if (ok) {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, A, t);
                if (lane == 0) {
                    scal[3 * kc] = f.sbar;
                    scal[3 * kc + 1] = f.pbar;
                    scal[3 * kc + 2] = f.beta;
                }
                for (int q0 = 0; q0 < C; q0 += 64) {
                    const bool on = q0 + lane < C;
                    const int q = on ? q0 + lane : C - 1;    // lanes beyond the pairs repeat the last one and are ignored
                    const int m = q / A, i = q - m * A;
                    if (m == 0)
                        t = pf_column(L.prof, np, h, de, f, pf_at(etab + i, A));
                    else
                        t = pf_column(L.prof, np, h, de, f, rp_col_of(L.tab, A, M, m, i, de));
                    if (on) {
                        const size_t o = (size_t)kc * C + q;
                        planes[o] = t.ebar;
                        planes[stride + o] = t.gamma;
                        planes[2 * stride + o] = t.See;
                        planes[3 * stride + o] = t.Sep;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// the explicit residuals of every usable cell of a fitted segment at every pair, with the segment's a_im: sse_cim replaces
// See_cim and b_cim replaces Sep_cim
template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_sr_resid(const double* __restrict__ prof_g, const int* __restrict__ cseg,
                                                         const int* __restrict__ used, const int* __restrict__ cnt,
                                                         const double* __restrict__ scal, double* __restrict__ planes,
                                                         const double* __restrict__ tot, long long K, int A, int h, int M,
                                                         int given, double de, int min_profiles,
                                                         const double* __restrict__ etab,
                                                         const double* __restrict__ ftab_g) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, false>(ftab_g, np, 2 * (h + M) + 1, A);
    const int C = A * (M + 1);
    const size_t stride = (size_t)K * C;
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        bool act = kc < K;
        int s = 0;
        if (act) {
            s = cseg[kc];
            const int m = cnt[2 * s];
            act = used[kc] != 0 && sg_fitted(m, sr_dof(m, cnt[2 * s + 1], M, given != 0), min_profiles);
        }
        if (act)
            for (int jj = lane; jj < np; jj += 64) L.prof[jj] = prof_g[(size_t)kc * np + jj];
        __syncthreads();
        if (act) {
            const double sbar = scal[3 * kc], pbar = scal[3 * kc + 1], beta = scal[3 * kc + 2];
            for (int q0 = 0; q0 < C; q0 += 64) {
                const bool on = q0 + lane < C;
                const int q = on ? q0 + lane : C - 1;        // lanes beyond the pairs repeat the last one and are ignored
                const int m = q / A, i = q - m * A;
                const size_t o = (size_t)kc * C + q;
                const double See = tot[((size_t)s * 2) * C + q], Sep = tot[((size_t)s * 2 + 1) * C + q];
                const double a = Sep / See;
                double b, c0, sse;
                pf_slope(sbar, pbar, beta, planes[o], planes[stride + o], a, b, c0);
                if (m == 0)
                    sse = pf_sse(L.prof, np, h, de, pf_at(etab + i, A), a, b, c0);
                else
                    sse = pf_sse(L.prof, np, h, de, rp_col_of(L.tab, A, M, m, i, de), a, b, c0);
                if (on) {
                    planes[2 * stride + o] = sse;
                    planes[3 * stride + o] = b;
                }
            }
        }
        __syncthreads();
    }
}

// the half-width of every age, the age of each segment, its interval and its row; the cell table at the best pair.
// tot: See and Sep of every (segment, pair); tsum: sse and the sum of b_c
__global__ __launch_bounds__(64) void k_sr_choose(const int* __restrict__ seg_start, const int* __restrict__ label,
                                                  const int* __restrict__ cnt, long long S, long long K,
                                                  const double* __restrict__ tot, const double* __restrict__ tsum,
                                                  const double* __restrict__ ages, int A, int M, int given, double slope,
                                                  double de, double delta, int min_profiles,
                                                  const long long* __restrict__ cells, const int* __restrict__ cn,
                                                  const int* __restrict__ used, const double* __restrict__ scal,
                                                  const double* __restrict__ planes, sc_segment_ramp_fit* __restrict__ rows,
                                                  sc_segment_cell* __restrict__ out_cells, double* __restrict__ curve,
                                                  signed char* __restrict__ widths) {
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const int C = A * (M + 1);
    const size_t stride = (size_t)K * C;
    const int m0 = given ? 1 : 0;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int start = seg_start[s], end = seg_start[s + 1];
        const int m = cnt[2 * s], n = cnt[2 * s + 1];
        const int dof = sr_dof(m, n, M, given != 0);
        const bool fitted = sg_fitted(m, dof, min_profiles);
        // (the rows were cleared: their padding is part of what the caller compares)
        sc_segment_ramp_fit* out = rows + s;
        int best = -1, mi = 0, m_best = 0;
        double a_best = nan;
        pf_pick k = {-1, -1, -1, nan};
        int status = 1;
        double a = nan, sse = nan, bbar = nan;
        if (fitted) {
            // the first smallest key over m in ascending order; a pair that cannot win counts as +inf
            const double dm = (double)m;
            double kbest = INFINITY;
            for (int mm = m0; mm <= M; ++mm) {
                const size_t q = (size_t)mm * A + ia;
                const double See = tot[((size_t)s * 2) * C + q], Sep = tot[((size_t)s * 2 + 1) * C + q];
                const double ssem = tsum[((size_t)s * 2) * C + q], bb = tsum[((size_t)s * 2 + 1) * C + q] / dm;
                const double am = Sep / See;
                const bool alive = See > 0.0 && ssem == ssem;
                double key = given ? fabs(fabs(rp_slope_of(am, bb, mm, de)) - slope) : ssem;
                if (!(alive && key == key)) key = INFINITY;
                if (mm == m0 || key < kbest) {
                    kbest = key;
                    sse = alive ? ssem : nan;
                    a = am;
                    bbar = bb;
                    mi = mm;
                }
            }
            k = pf_choose(sse, lane, A, delta, dof);
            best = k.best;
            a_best = __shfl(a, best, 64);
            m_best = __shfl(mi, best, 64);
            status = pf_open(k, A) + (M > 0 && m_best == M ? 8 : 0);
        }
        if (curve && lane < A) curve[s * A + lane] = sse;
        if (widths && lane < A) widths[s * A + lane] = (signed char)(fitted ? mi : 0);
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
            out->width_index = fitted ? mi : 0;
            out->width = fitted ? (double)mi * de : nan;
            out->initial_slope = fitted ? (mi ? rp_slope_of(a, bbar, mi, de) : copysign(INFINITY, a)) : nan;
        }
        if (!out_cells) continue;
        for (int c = start + lane; c < end; c += 64) {
            sc_segment_cell* oc = out_cells + c;
            const int u = used[c];
            double b = nan, c0 = nan, csse = nan;
            if (fitted && u) {
                const size_t o = (size_t)c * C + (size_t)m_best * A + best;
                pf_slope(scal[3 * c], scal[3 * c + 1], scal[3 * c + 2], planes[o], planes[stride + o], a_best, b, c0);
                csse = planes[2 * stride + o];
            }
            oc->cell = cells[c];
            oc->used = u;
            oc->n = cn[c];
            oc->b = b; oc->c0 = c0; oc->sse = csse;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

static sg_park sr_park(int A, int h, int M) { return sg_park_plain(A * (M + 1), h, false); }

static int sr_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A, int h,
                  int w, int M, int mode, double slope, double de, double delta, int min_samples, int min_profiles,
                  sc_segment_ramp_fit* out_rows, sc_segment_cell* out_cells, double* out_sse, int8_t* out_width) {
    if (S == 0) return SC_OK;
    const int given = mode == SC_RAMP_SLOPE ? 1 : 0;
    const int np = 2 * h + 1, ht = h + M, nt = 2 * ht + 1, C = A * (M + 1);
    const size_t ftab_bytes = sizeof(double) * (size_t)nt * A;
    const bool tab_lds = ftab_bytes <= PF_TAB_LDS;
    const size_t lds = pf_lds_bytes(np, nt, A, false, tab_lds);
    const auto k_partial = tab_lds ? k_sr_partial<true> : k_sr_partial<false>;
    const auto k_resid = tab_lds ? k_sr_resid<true> : k_sr_resid<false>;
    int rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_partial, lds))) return rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_resid, lds))) return rc;

    // (the totals of a chunk as a CSR array over the segments: a segment's blocks and one more, C columns each)
    std::vector<long long> tot_start;
    sc_fit_block_totals(seg_start, S, tot_start);
    // (the erf table of the m = 0 pairs is the plain call's, by its launch: the same bits; the park is the plain call's
    // with C columns for A: four planes of m C doubles)
    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, h, de, sr_park(A, h, M), SR_MAX_SEGS, tot_start.data(),
                 SR_MAX_TOTALS / C, 2};
    c.out = {{out_rows, &ctx->sg_rows, sizeof(sc_segment_ramp_fit), SG_SEGS, true},
             {out_cells, &ctx->sg_out, sizeof(sc_segment_cell), SG_CELLS},
             {out_sse, &ctx->sg_sse, sizeof(double) * A, SG_SEGS},
             {out_width, &ctx->sg_width, (size_t)A, SG_SEGS}};
    double* d_ftab;
    c.tables = [&](const double* d_ages) {
        if ((rc = sc_ensure(ctx, ctx->sg_ftab, ftab_bytes))) return rc;
        d_ftab = (double*)ctx->sg_ftab.p;
        return sc_rp_table(ctx, d_ages, A, ht, de, d_ftab);
    };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const long long m = st.m;
        const size_t mC = (size_t)m * C;
        const unsigned gcell = pf_grid(m);
        int launches = 0;
        if (m) {
            k_partial<<<gcell, PF_THREADS, lds, ctx->stream>>>(z, ny, nx, st.cells, st.dirs, m, A, h, w, M, de, min_samples, k.tab,
                                                              d_ftab, st.prof, st.cn, st.used, st.scal, st.planes);
            ++launches;
        }
        sc_sg_rank_launch(ctx, st);
        ++launches;
        if (k.G) {
            sc_sg_sum_launch(ctx, st.planes + 2 * mC, st, k.blk, k.G, C, 2, k.part, k.tot);
            k_resid<<<gcell, PF_THREADS, lds, ctx->stream>>>(st.prof, k.cseg, st.used, st.cnt, st.scal, st.planes, k.tot, m, A, h, M,
                                                            given, de, min_profiles, k.tab, d_ftab);
            sc_sg_sum_launch(ctx, st.planes + 2 * mC, st, k.blk, k.G, C, 2, k.part, k.tsum);
            launches += 5;
        }
        k_sr_choose<<<sg_grid(st.Sc), 64, 0, ctx->stream>>>(st.seg, st.label, st.cnt, st.Sc, m, k.tot, k.tsum, k.ages, A, M, given,
                                                           slope, de, delta, min_profiles, st.cells, st.cn, st.used, st.scal,
                                                           st.planes, (sc_segment_ramp_fit*)k.out[0], (sc_segment_cell*)k.out[1],
                                                           (double*)k.out[2], (signed char*)k.out[3]);
        return launches + 1;
    };
    return sc_sg_chunks(ctx, c);
}

// The two calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null)
static int sr_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const double* ages, int A, int h, int w, int M, int mode, double slope, double de, double delta,
                   int min_samples, int min_profiles, sc_segment_ramp_fit* out_rows, sc_segment_cell* out_cells,
                   double* out_sse, int8_t* out_width) {
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, -1, de, delta, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if ((rc = sc_rp_check(ctx, who, h, M, mode, slope, min_samples))) return rc;
    if ((rc = sc_sg_check_cap(ctx, who, seg_start, S, sc_sg_cap_cells(sr_park(A, h, M)), "at this h, A and M"))) return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return sr_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, ages, A, h, w, M, mode, slope, de, delta, min_samples,
                  min_profiles, out_rows, out_cells, out_sse, out_width);
}

extern "C" int sc_fit_segments_ramp(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                    const long long* seg_start, const int32_t* seg_label, long long S, const double* ages,
                                    int A, int h, int w, int M, int mode, double slope, double de, double delta,
                                    int min_samples, int min_profiles, sc_segment_ramp_fit* out_rows,
                                    sc_segment_cell* out_cells, double* out_sse, int8_t* out_width) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_segments_ramp");
    if (rc) return rc;
    return sr_call(ctx, "sc_fit_segments_ramp", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A,
                   h, w, M, mode, slope, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_width);
}

extern "C" int sc_fit_segments_ramp_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                        const double* sa, const double* ca, long long K, const long long* seg_start,
                                        const int32_t* seg_label, long long S, const double* ages, int A, int h, int w,
                                        int M, int mode, double slope, double de, double delta, int min_samples,
                                        int min_profiles, sc_segment_ramp_fit* out_rows, sc_segment_cell* out_cells,
                                        double* out_sse, int8_t* out_width) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return sr_call(ctx, "sc_fit_segments_ramp_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, M, mode,
                   slope, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_width);
}
