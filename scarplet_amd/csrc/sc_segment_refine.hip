// sc_fit_segments_refine*: continuous ages of the joint fit (docs/segments.md, "Continuous ages").
//
// The fit of sc_fit_segments by its own launches (stage one, sc_sg_grid_launch: the shared fields are its bytes), and after
// it the refinement of sc_refine.hip on the segment's POOLED criterion.  A candidate age's sse is a sum over the segment's
// profiles, so where k_pf_refine runs a search inside one wave, here a level of a search is a ROUND of launches, and what a
// search knows between two rounds lives in a record per segment on the device (sx_state): no copy to the host in between.
//   k_sx_begin    one wave per segment: the record from the grid fit's row - the first bracket of the minimum, the grid's
//                 best as the fine best so far -, and the grid's b, c0, sse as the fine fields of the cell table
//   a round       of the minimum (64 candidate columns a cell), or of BOTH ends of the interval side by side (128: the
//                 lower end's candidates in columns 0..63, the upper end's in 64..127) - 2 R rounds, not 3 R:
//     k_sx_column one wave per cell: pf_fetch, pf_moments and pf_line without a column (the bits of stage one's), then the
//                 lanes run over the 64 candidates of the bracket of the cell's segment: pf_column on rf_col.  ebar, gamma,
//                 See, Sep go to candidate planes shaped like the per-age planes, parked behind them
//     (sc_sg_sum_launch on See, Sep: the blocked sum of the grid fit, on C = 64 or 128 columns)
//     k_sx_resid  one wave per cell, lanes over the candidates: a = Sep / See of the segment's totals, pf_slope, pf_sse on
//                 rf_col; the cell's sse takes the place of See
//     (sc_sg_sum_launch on sse)
//     k_sx_pick   one wave per segment, lane l holding sse(x_l): the shuffle argmin and the ballots of k_pf_refine, the next
//                 bracket into the record.  After the minimum's last level: the fine best, thr, the walk along the grid
//                 curve, the first brackets of the ends, and the cell table's fine fields (lanes over the segment's cells)
//                 before the ends' rounds overwrite the planes
//   k_sx_finish   one thread per segment: the row's fine fields from the record
// A cell whose segment is not fitted, or whose search left the grid, skips the round's work: the test reads the record of
// the cell's segment, is uniform over the wave, and no barrier sits inside it.  The launches of a chunk are 10 + 14 R (4
// for a chunk without cells): they depend on R alone, never on the data.
// A candidate's arithmetic is pf_column, Sep / See, pf_slope, pf_sse - pf_candidate's helpers in its order - and the sum
// over one profile is no addition: a segment of one usable profile returns k_pf_refine's bytes.
// No atomics, no float sum across lanes other than the blocked sums, no scratch.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

#define SX_MAX_SEGS (1ll << 20)          // segments per chunk, as sc_fit_segments
#define SX_COLUMNS SC_SEGMENT_REFINE_COLUMNS

// What the searches of one segment know between two rounds.  Search 0: the minimum; 1: the lower end; 2: the upper end
struct sx_state {
    double p[3], q[3];         // the bracket of each search
    double thr;                // sse_fine (1 + delta / dof), once the minimum is known
    double fx, fa, fs;         // the fine best so far: age, amplitude, sse
    double lo, hi;             // the ends of the interval so far
    int act[3];                // the search still runs rounds
    int st;                    // status_fine so far
    int dof;
    int fitted;
};

// the searches ph0 .. ph0 + nh - 1 of a round, and whether the cell kc takes part in any: wave-uniform
__device__ __forceinline__ bool sx_cell_on(const sx_state* state, const int* __restrict__ cseg, const int* __restrict__ used,
                                           long long kc, long long K, int ph0, int nh, int& s) {
    s = 0;
    if (kc >= K || used[kc] == 0) return false;
    s = cseg[kc];
    bool on = false;
    for (int hf = 0; hf < nh; ++hf) on = on || state[s].act[ph0 + hf] != 0;
    return on;
}

__global__ __launch_bounds__(64) void k_sx_begin(const int* __restrict__ seg_start, long long S,
                                                 const sc_segment_fine_fit* __restrict__ rows, const double* __restrict__ ages,
                                                 int A, int R, sx_state* state, sc_segment_fine_cell* out_cells) {
    const int lane = threadIdx.x;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const sc_segment_fine_fit* row = rows + s;
        const int i = row->kt_index;
        const bool fitted = i >= 0;
        if (lane == 0) {
            sx_state* t = state + s;
            for (int ph = 0; ph < 3; ++ph) {
                t->p[ph] = 0.0;
                t->q[ph] = 0.0;
                t->act[ph] = 0;
            }
            if (fitted) {
                t->p[0] = ages[max(i - 1, 0)];
                t->q[0] = ages[min(i + 1, A - 1)];
                t->act[0] = R > 0 ? 1 : 0;
            }
            t->thr = 0.0;
            t->fx = row->kt; t->fa = row->a; t->fs = row->sse;
            t->lo = row->kt_lo; t->hi = row->kt_hi;
            t->st = row->status;
            t->dof = row->dof;
            t->fitted = fitted ? 1 : 0;
        }
        if (!out_cells) continue;
        // (the grid's values: what stays where the grid age is kept, and NaN where b is NaN)
        for (int c = seg_start[s] + lane; c < seg_start[s + 1]; c += 64) {
            sc_segment_fine_cell* oc = out_cells + c;
            oc->b_fine = oc->b; oc->c0_fine = oc->c0; oc->sse_fine = oc->sse;
        }
    }
}

// the terms of the candidates of the searches ph0 .. ph0 + nh - 1 against every usable profile: C = 64 nh columns a cell
__global__ __launch_bounds__(PF_THREADS) void k_sx_column(const double* __restrict__ prof_g, const int* __restrict__ cseg,
                                                          const int* __restrict__ used, const sx_state* state, long long K, int h,
                                                          double de, int ph0, int nh, double* __restrict__ cand) {
    const int np = 2 * h + 1, C = 64 * nh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<false, false>(nullptr, np, np, 0);
    const size_t stride = (size_t)K * C;                 // one per-cell-and-candidate plane
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        int s;
        const bool act = sx_cell_on(state, cseg, used, kc, K, ph0, nh, s);
        if (act) pf_fetch<false>(prof_g, nullptr, kc, np, lane, L.prof, nullptr);
        __syncthreads();
        if (act) {
            // the profile's own terms, as stage one formed them
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, 0);
            pf_col none;
            const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, 0, none);
            for (int hf = 0; hf < nh; ++hf) {
                const sx_state* t = state + s;
                if (!t->act[ph0 + hf]) continue;
                const double x = rf_x(t->p[ph0 + hf], t->q[ph0 + hf], lane);
                const pf_col tc = pf_column(L.prof, np, h, de, f, rf_col{2.0 * sqrt(x), de, h});
                const size_t o = (size_t)kc * C + hf * 64 + lane;
                cand[o] = tc.ebar;
                cand[stride + o] = tc.gamma;
                cand[2 * stride + o] = tc.See;
                cand[3 * stride + o] = tc.Sep;
            }
        }
        __syncthreads();
    }
}

// the explicit residuals of every usable cell at every candidate, with the segment's a: sse_c replaces See_c
__global__ __launch_bounds__(PF_THREADS) void k_sx_resid(const double* __restrict__ prof_g, const int* __restrict__ cseg,
                                                         const int* __restrict__ used, const sx_state* state,
                                                         const double* __restrict__ scal, double* __restrict__ cand,
                                                         const double* __restrict__ tot, long long K, int h, double de, int ph0,
                                                         int nh) {
    const int np = 2 * h + 1, C = 64 * nh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<false, false>(nullptr, np, np, 0);
    const size_t stride = (size_t)K * C;
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        int s;
        const bool act = sx_cell_on(state, cseg, used, kc, K, ph0, nh, s);
        if (act) pf_fetch<false>(prof_g, nullptr, kc, np, lane, L.prof, nullptr);
        __syncthreads();
        if (act) {
            for (int hf = 0; hf < nh; ++hf) {
                const sx_state* t = state + s;
                if (!t->act[ph0 + hf]) continue;
                const int q = hf * 64 + lane;
                const size_t o = (size_t)kc * C + q;
                const double See = tot[((size_t)s * 2) * C + q], Sep = tot[((size_t)s * 2 + 1) * C + q];
                const double a = Sep / See;
                double b, c0;
                pf_slope(scal[3 * kc], scal[3 * kc + 1], scal[3 * kc + 2], cand[o], cand[stride + o], a, b, c0);
                const double x = rf_x(t->p[ph0 + hf], t->q[ph0 + hf], lane);
                cand[2 * stride + o] = pf_sse(L.prof, np, h, de, rf_col{2.0 * sqrt(x), de, h}, a, b, c0);
            }
        }
        __syncthreads();
    }
}

// One level of the searches ph0 .. (ph0 = 0: the minimum, 64 columns; ph0 = 1: both ends, 128 columns) of every segment:
// k_pf_refine's picks on the pooled sse, lane l holding candidate l.  `last`: the level is the search's last
__global__ __launch_bounds__(64) void k_sx_pick(const int* __restrict__ seg_start, long long S, long long K, sx_state* state,
                                                const double* __restrict__ tot, const double* __restrict__ tsse,
                                                const double* __restrict__ curve, const double* __restrict__ ages, int A,
                                                double delta, int ph0, int last, const int* __restrict__ used,
                                                const double* __restrict__ scal, const double* __restrict__ cand,
                                                sc_segment_fine_cell* out_cells) {
    const int lane = threadIdx.x;
    const int ia = min(lane, A - 1);
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        sx_state* t = state + s;
        if (ph0 == 0) {
            if (!t->act[0]) continue;
            const double x = rf_x(t->p[0], t->q[0], lane);
            const double cs = tsse[(size_t)s * 64 + lane];
            const double ca = tot[((size_t)s * 2 + 1) * 64 + lane] / tot[((size_t)s * 2) * 64 + lane];
            double m = cs == cs ? cs : INFINITY;
            int mi = lane;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double om = __shfl_xor(m, o, 64);
                const int oi = __shfl_xor(mi, o, 64);
                if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
            }
            const double p = __shfl(x, max(mi - 1, 0), 64), q = __shfl(x, min(mi + 1, 63), 64);
            if (!last) {
                if (lane == 0) {
                    t->p[0] = p;
                    t->q[0] = q;
                }
                continue;
            }
            const double bx = __shfl(x, mi, 64), ba = __shfl(ca, mi, 64), bs = __shfl(cs, mi, 64);
            double fx = t->fx, fa = t->fa, fs = t->fs;
            const bool moved = bs <= fs;
            if (moved) { fx = bx; fa = ba; fs = bs; }
            const double thr = fs * (1.0 + delta / (double)t->dof);
            const unsigned long long okm = __ballot(lane < A && curve[(size_t)s * A + ia] <= thr);
            int st = 0;
            // the lower end: the walk along the grid curve, then the first bracket
            double lo = t->lo, hi = t->hi, p1 = 0.0, q1 = 0.0, p2 = 0.0, q2 = 0.0;
            int on1 = 0, on2 = 0;
            {
                const unsigned long long le = __ballot(lane < A && ages[ia] <= fx);
                const int g = le ? 63 - __clzll((long long)le) : 0;
                int j = g;
                while (j >= 0 && ((okm >> j) & 1ull)) --j;
                if (j < 0) {
                    lo = ages[0];
                    st |= 2;
                } else {
                    p1 = ages[j];
                    q1 = j + 1 <= g ? ages[j + 1] : fx;
                    on1 = 1;
                }
            }
            {
                const unsigned long long ge = __ballot(lane < A && ages[ia] >= fx);
                const int g = ge ? __ffsll((unsigned long long)ge) - 1 : A - 1;
                int j = g;
                while (j <= A - 1 && ((okm >> j) & 1ull)) ++j;
                if (j > A - 1) {
                    hi = ages[A - 1];
                    st |= 4;
                } else {
                    q2 = ages[j];
                    p2 = j - 1 >= g ? ages[j - 1] : fx;
                    on2 = 1;
                }
            }
            // the cell table at kt_fine, before the ends' rounds overwrite the planes (the grid's values are in place)
            if (out_cells && moved) {
                const size_t stride = (size_t)K * 64;
                for (int c = seg_start[s] + lane; c < seg_start[s + 1]; c += 64) {
                    if (!used[c]) continue;
                    const size_t o = (size_t)c * 64 + mi;
                    double b, c0;
                    pf_slope(scal[3 * c], scal[3 * c + 1], scal[3 * c + 2], cand[o], cand[stride + o], ba, b, c0);
                    sc_segment_fine_cell* oc = out_cells + c;
                    oc->b_fine = b; oc->c0_fine = c0; oc->sse_fine = cand[2 * stride + o];
                }
            }
            if (lane == 0) {
                t->act[0] = 0;
                t->fx = fx; t->fa = fa; t->fs = fs;
                t->thr = thr;
                t->st = st;
                t->lo = lo; t->hi = hi;
                t->p[1] = p1; t->q[1] = q1; t->act[1] = on1;
                t->p[2] = p2; t->q[2] = q2; t->act[2] = on2;
            }
        } else {
            const double thr = t->thr;
            if (t->act[1]) {
                const double x = rf_x(t->p[1], t->q[1], lane);
                const double cs = tsse[(size_t)s * 128 + lane];
                const unsigned long long in = __ballot(lane >= 1 && (cs <= thr || lane == 63));
                const int l = __ffsll(in) - 1;
                const double p = __shfl(x, l - 1, 64), q = __shfl(x, l, 64);
                if (lane == 0) {
                    t->p[1] = p;
                    t->q[1] = q;
                    if (last) {
                        t->lo = q;
                        t->act[1] = 0;
                    }
                }
            }
            if (t->act[2]) {
                const double x = rf_x(t->p[2], t->q[2], lane);
                const double cs = tsse[(size_t)s * 128 + 64 + lane];
                const unsigned long long in = __ballot(lane <= 62 && (cs <= thr || lane == 0));
                const int l = 63 - __clzll((long long)in);
                const double p = __shfl(x, l, 64), q = __shfl(x, l + 1, 64);
                if (lane == 0) {
                    t->p[2] = p;
                    t->q[2] = q;
                    if (last) {
                        t->hi = p;
                        t->act[2] = 0;
                    }
                }
            }
        }
    }
}

// the fine fields of every row (the rows were cleared: their padding is part of what the caller compares)
__global__ __launch_bounds__(64) void k_sx_finish(long long S, const sx_state* __restrict__ state,
                                                  sc_segment_fine_fit* __restrict__ rows) {
    const double nan = __builtin_nan("");
    for (long long s = (long long)blockIdx.x * 64 + threadIdx.x; s < S; s += (long long)gridDim.x * 64) {
        const sx_state* t = state + s;
        sc_segment_fine_fit* out = rows + s;
        const bool fitted = t->fitted != 0;
        out->kt_fine = fitted ? t->fx : nan;
        out->kt_lo_fine = fitted ? t->lo : nan;
        out->kt_hi_fine = fitted ? t->hi : nan;
        out->a_fine = fitted ? t->fa : nan;
        out->sse_fine = fitted ? t->fs : nan;
        out->rmse_fine = fitted ? sqrt(t->fs / (double)t->dof) : nan;
        out->status_fine = fitted ? t->st : 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// the park of the plain call with the candidate columns of a round behind the A ages: four planes of m (A + Cc) doubles
static sg_park sx_park(int A, int h, int R) { return sg_park_plain(A + (R > 0 ? SX_COLUMNS : 0), h, false); }

static int sx_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const double* ages, int A, int h,
                  int w, int R, double de, double delta, int min_samples, int min_profiles, sc_segment_fine_fit* out_rows,
                  sc_segment_fine_cell* out_cells, double* out_sse) {
    if (S == 0) return SC_OK;
    const int np = 2 * h + 1;
    const size_t lds = pf_lds_bytes(np, np, 0, false, false);
    int rc;
    if ((rc = sc_sg_stage_attr(ctx, A, h, -1))) return rc;
    if ((rc = sc_sg_grid_attr(ctx, A, h, -1))) return rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_sx_column, lds))) return rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_sx_resid, lds))) return rc;

    sg_call c = {cells, sa, ca, seg_start, seg_label, S, ages, A, h, de, sx_park(A, h, R), SX_MAX_SEGS, nullptr, 0, 1};
    // (the curve is read by the walk of every segment: on the device whether or not it is asked for)
    c.out = {{out_rows, &ctx->sg_rows, sizeof(sc_segment_fine_fit), SG_SEGS, true},
             {out_cells, &ctx->sg_out, sizeof(sc_segment_fine_cell), SG_CELLS},
             {out_sse, &ctx->sg_sse, sizeof(double) * A, SG_SEGS, false, true}};
    sx_state* d_state;
    c.prepare = [&](const sg_chunk& k) {
        if ((rc = sc_ensure(ctx, ctx->sg_fine, sizeof(sx_state) * (size_t)k.st.Sc))) return rc;
        d_state = (sx_state*)ctx->sg_fine.p;
        return SC_OK;
    };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const long long m = st.m, Sc = st.Sc;
        sc_segment_fine_fit* rows = (sc_segment_fine_fit*)k.out[0];
        sc_segment_fine_cell* tab = (sc_segment_fine_cell*)k.out[1];
        double* curve = (double*)k.out[2];
        // (the candidates' planes, totals and sums sit behind the A columns of the grid fit's)
        double* cand = st.planes + 4 * (size_t)m * A;
        double* ctot = k.tot + 2 * (size_t)Sc * A;
        double* csse = k.tsum + (size_t)Sc * A;
        int launches = sc_sg_stage_launch(ctx, z, ny, nx, A, h, w, -1, de, min_samples, k.tab, st) +
                       sc_sg_grid_launch(ctx, k, A, h, -1, de, delta, min_profiles, true, rows, tab, curve);
        k_sx_begin<<<sg_grid(Sc), 64, 0, ctx->stream>>>(st.seg, Sc, rows, k.ages, A, R, d_state, tab);
        ++launches;
        for (int r = 0; k.G && r < 2 * R; ++r) {         // R levels of the minimum, then R of both ends
            const int ph0 = r < R ? 0 : 1, nh = r < R ? 1 : 2, C = 64 * nh;
            const int last = (r == R - 1 || r == 2 * R - 1) ? 1 : 0;
            const size_t mC = (size_t)m * C;
            k_sx_column<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(st.prof, k.cseg, st.used, d_state, m, h, de, ph0, nh, cand);
            sc_sg_sum_launch(ctx, cand + 2 * mC, st, k.blk, k.G, C, 2, k.part, ctot);
            k_sx_resid<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(st.prof, k.cseg, st.used, d_state, st.scal, cand, ctot, m, h, de,
                                                                    ph0, nh);
            sc_sg_sum_launch(ctx, cand + 2 * mC, st, k.blk, k.G, C, 1, k.part, csse);
            k_sx_pick<<<sg_grid(Sc), 64, 0, ctx->stream>>>(st.seg, Sc, m, d_state, ctot, csse, curve, k.ages, A, delta, ph0, last,
                                                          st.used, st.scal, cand, tab);
            launches += 7;
        }
        k_sx_finish<<<sg_grid((Sc + 63) / 64), 64, 0, ctx->stream>>>(Sc, d_state, rows);
        return launches + 1;
    };
    return sc_sg_chunks(ctx, c);
}

// The two calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null)
static int sx_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const double* ages, int A, int h, int w, int R, double de, double delta, int min_samples, int min_profiles,
                   sc_segment_fine_fit* out_rows, sc_segment_fine_cell* out_cells, double* out_sse) {
    int rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, -1, de, delta, min_samples,
                         min_profiles, out_rows);
    if (rc) return rc;
    if (R < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the refinement must be >= 0 levels", who);
    if (R > SC_PROFILE_MAX_REFINE)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d levels of refinement, more than %d", who, R, SC_PROFILE_MAX_REFINE);
    if ((rc = sc_sg_check_cap(ctx, who, seg_start, S, sc_sg_cap_cells(sx_park(A, h, R)), "at this h and A with refinement")))
        return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return sx_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, ages, A, h, w, R, de, delta, min_samples,
                  min_profiles, out_rows, out_cells, out_sse);
}

extern "C" int sc_fit_segments_refine(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                      const long long* seg_start, const int32_t* seg_label, long long S, const double* ages,
                                      int A, int h, int w, int R, double de, double delta, int min_samples, int min_profiles,
                                      sc_segment_fine_fit* out_rows, sc_segment_fine_cell* out_cells, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_segments_refine");
    if (rc) return rc;
    return sx_call(ctx, "sc_fit_segments_refine", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, ages,
                   A, h, w, R, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse);
}

extern "C" int sc_fit_segments_refine_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                          const double* sa, const double* ca, long long K, const long long* seg_start,
                                          const int32_t* seg_label, long long S, const double* ages, int A, int h, int w,
                                          int R, double de, double delta, int min_samples, int min_profiles,
                                          sc_segment_fine_fit* out_rows, sc_segment_fine_cell* out_cells, double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return sx_call(ctx, "sc_fit_segments_refine_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, ages, A, h, w, R, de,
                   delta, min_samples, min_profiles, out_rows, out_cells, out_sse);
}
