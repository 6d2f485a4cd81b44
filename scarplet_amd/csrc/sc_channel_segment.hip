// sc_channel_segments*: one channel width per reach, fitted jointly (docs/channels.md, "One width per reach").
//
// sc_channel_profiles fits every trace cell on its own; a mapped reach gets ONE width.  The cells arrive grouped by reach
// (CSR seg_start), the frame is that of sc_fit_segments_shift (sc_segment.hip) and the search that of sc_channel_profiles
// (sc_channel.h): every usable profile c takes, at every frequency i, its own centre shift d_ci by the single-profile
// rule, dead pairs never winning, and then
//   SC_CHANNEL_DEPTH_PROFILE  the frequency is the reach's; depth, intercept, slope and centre are each profile's own.
//                             sse_i = sum_c sse*_ci, abar_i = (sum_c a_ci) / n_profiles
//   SC_CHANNEL_DEPTH_SEGMENT  the fixed-effects fit of sc_fit_segments_shift on the Gaussian column: a_i = sum_c Sep_ci /
//                             sum_c See_ci, then explicit residuals with that a_i and the column at d_ci
//   k_cs_stage   k_sg_shift's shape with ch_search's dead-pair rule and k_ch_terms' fast route (ch_search_terms): one wave
//                per cell, PF_WAVES per workgroup.  Parks n, used, (sbar, pbar, beta), d_ci and four planes per cell and
//                frequency - segment mode: ebar, gamma, See, Sep at d_ci (k_sg_shift's layout, so that k_sg_resid reads
//                them) and the profile; profile mode: sse*, a, b, c0 - all NaN where the frequency has no live pair
//   (k_sg_rank, k_sg_sum1, k_sg_sum2, sc_segment.hip: the usable profiles in input order, blocks of 64 in sequence, then
//   the block sums in sequence - on (sse*, a) or on (See, Sep); NaN propagates, so a frequency that is dead in one usable
//   profile is dead for the reach)
//   (segment mode: k_sg_resid on the Gaussian table, then the sums again on sse_ci)
//   k_cs_choose  one wave per reach, lanes over the frequencies: pf_choose on the pooled curve, the row; then lanes over
//                the reach's cells for status bit 8 and the cell table at the best frequency
// The park per cell is sc_fit_segments_shift's, 8 ((2h + 1) + 4 F) + F bytes (SC_CHANNEL_SEGMENT_PARK; profile mode leaves
// the profile's share unused).  G sits in LDS when it fits PF_TAB_LDS bytes and in global memory otherwise (pf_stage).  No
// atomics at all, no float sum across lanes.
#include "sc_channel.h"
#include <math.h>
#include <algorithm>

#define CS_MAX_SEGS (1ll << 20)          // reaches per chunk: bounds the rows and totals of a call with empty reaches

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_cs_stage(const double* __restrict__ z, int ny, int nx,
                                                         const long long* __restrict__ cells,
                                                         const double* __restrict__ dir, long long K, int F, int h, int w,
                                                         int D, double de, int min_samples, int mode,
                                                         const double* __restrict__ tab_g, const double* __restrict__ terms,
                                                         double* __restrict__ prof_g, int* __restrict__ cn,
                                                         int* __restrict__ used, double* __restrict__ scal,
                                                         double* __restrict__ planes, signed char* __restrict__ shifts) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pf_lds L = pf_stage<TAB_LDS, true>(tab_g, np, 2 * (h + D) + 1, F);
    const double* slot = L.slot;
    const int* srank = (const int*)(slot + (size_t)SH_TERMS * F);
    const double nan = __builtin_nan("");
    const size_t stride = (size_t)K * F;                 // one per-cell-and-frequency plane
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        if (act) pf_cut(z, ny, nx, cells[kc], dir, kc, h, w, lane, L.prof, prof_g);
        __syncthreads();
        if (act) {
            // what depends on neither the frequency nor the shift, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, F);
            const bool ok = mo.n_neg >= min_samples && mo.n_pos >= min_samples;
            if (lane == 0) {
                cn[kc] = mo.n;
                used[kc] = ok ? 1 : 0;
            }
            if (!ok) {
                if (lane < F) shifts[(size_t)kc * F + lane] = 0;
            } else {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, F, t);
                ch_search_terms(L.prof, L.tab, mo.n == np ? terms : nullptr, np, h, F, D, de, lane, f, L.slot);
                if (lane == 0) {
                    scal[3 * kc] = f.sbar;
                    scal[3 * kc + 1] = f.pbar;
                    scal[3 * kc + 2] = f.beta;
                }
                if (lane < F) {
                    const size_t o = (size_t)kc * F + lane;
                    const double sse = slot[lane], See = slot[F + lane], Sep = slot[2 * F + lane];
                    const double ebar = slot[3 * F + lane], gamma = slot[4 * F + lane];
                    const bool dead = sse != sse;        // (no live pair at this frequency: NaN terms, d_ci = 0)
                    if (mode == SC_CHANNEL_DEPTH_PROFILE) {
                        const double a = Sep / See;
                        double b, c0;
                        pf_slope(f.sbar, f.pbar, f.beta, ebar, gamma, a, b, c0);
                        planes[o] = sse;
                        planes[stride + o] = dead ? nan : a;
                        planes[2 * stride + o] = dead ? nan : b;
                        planes[3 * stride + o] = dead ? nan : c0;
                    } else {
                        planes[o] = dead ? nan : ebar;
                        planes[stride + o] = dead ? nan : gamma;
                        planes[2 * stride + o] = dead ? nan : See;
                        planes[3 * stride + o] = dead ? nan : Sep;
                    }
                    shifts[o] = (signed char)(dead ? 0 : sh_shift_of(srank[lane]));
                }
            }
        }
        __syncthreads();
    }
}

// The frequency of each reach, its interval and its row; the cell table at the best frequency.  tot: profile mode the sums
// of sse*_ci and of a_ci, segment mode those of See_ci and Sep_ci; tsse (segment mode): the sum of the explicit sse_ci.
// planes: what k_cs_stage parked, with - segment mode - sse_ci in the place of See_ci (k_sg_resid)
__global__ __launch_bounds__(64) void k_cs_choose(const int* __restrict__ seg_start, const int* __restrict__ label,
                                                  const int* __restrict__ cnt, long long S, long long K,
                                                  const double* __restrict__ tot, const double* __restrict__ tsse,
                                                  const double* __restrict__ freqs, int F, int D, double delta,
                                                  int min_profiles, int mode, const long long* __restrict__ cells,
                                                  const int* __restrict__ cn, const int* __restrict__ used,
                                                  const double* __restrict__ scal, const double* __restrict__ planes,
                                                  const signed char* __restrict__ shifts, sc_segment_fit* __restrict__ rows,
                                                  sc_channel_segment_cell* __restrict__ out_cells,
                                                  double* __restrict__ curve) {
    const int lane = threadIdx.x;
    const int ia = min(lane, F - 1);                     // lanes beyond the frequencies repeat the last one and are ignored
    const double nan = __builtin_nan("");
    const size_t stride = (size_t)K * F;
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;
    for (long long s = blockIdx.x; s < S; s += gridDim.x) {
        const int start = seg_start[s], end = seg_start[s + 1];
        const int m = cnt[2 * s], n = cnt[2 * s + 1];
        const int dof = cs_dof(mode, m, n, D);
        const bool fitted = sg_fitted(m, dof, min_profiles);
        // (the rows were cleared: their padding is part of what the caller compares)
        sc_segment_fit* out = rows + s;
        int best = -1;
        double a_best = nan;
        pf_pick k = {-1, -1, -1, nan};
        int status = 1;
        double a = nan, sse = nan;
        if (fitted) {
            const double t0 = tot[((size_t)s * 2) * F + ia], t1 = tot[((size_t)s * 2 + 1) * F + ia];
            if (own) {
                sse = t0;
                a = t1 / (double)m;
            } else {
                a = t1 / t0;
                sse = t0 > 0.0 ? tsse[(size_t)s * F + ia] : nan;       // (a frequency whose sum of See is not > 0 is dead)
            }
            if (!__ballot(lane < F && sse == sse)) {
                status = 1 | 32;                         // every frequency is dead
                a = nan;
            } else {
                k = pf_choose(sse, lane, F, delta, dof);
                best = k.best;
                a_best = __shfl(a, best, 64);
                // a usable profile whose shift at the best frequency sits at the end of the range
                bool at_end = false;
                if (D > 0)
                    for (int c = start + lane; c < end; c += 64) {
                        const int d = shifts[(size_t)c * F + best];
                        at_end = at_end || (used[c] != 0 && (d == D || d == -D));
                    }
                status = pf_open(k, F) + (__ballot(at_end) != 0ull ? 8 : 0);
            }
        }
        const bool alive = best >= 0;
        if (curve && lane < F) curve[s * F + lane] = sse;
        if (lane == (alive ? best : 0)) {
            out->label = label[s];
            out->n_cells = end - start;
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
            out->a = a;
            out->sse = alive ? sse : nan;
            out->rmse = alive ? sqrt(sse / (double)dof) : nan;
        }
        if (!out_cells) continue;
        for (int c = start + lane; c < end; c += 64) {
            // (field by field: the cell ends in padding, which the host cleared)
            sc_channel_segment_cell* oc = out_cells + c;
            const int u = used[c];
            double ca = nan, b = nan, c0 = nan, csse = nan;
            int d = 0;
            if (alive && u) {
                const size_t o = (size_t)c * F + best;
                if (own) {
                    csse = planes[o];
                    ca = planes[stride + o];
                    b = planes[2 * stride + o];
                    c0 = planes[3 * stride + o];
                } else {
                    ca = a_best;
                    pf_slope(scal[3 * c], scal[3 * c + 1], scal[3 * c + 2], planes[o], planes[stride + o], a_best, b, c0);
                    csse = planes[2 * stride + o];
                }
                d = shifts[o];
            }
            oc->cell = cells[c];
            oc->used = u;
            oc->n = cn[c];
            oc->a = ca; oc->b = b; oc->c0 = c0; oc->sse = csse;
            oc->shift_index = d;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// (the park of sc_fit_segments_shift: SC_CHANNEL_SEGMENT_PARK bytes per cell)
static sg_park cs_park(int F, int h) { return sg_park_plain(F, h, true); }
static_assert(SC_CHANNEL_SEGMENT_PARK(100, 35) == 8 * (201 + 4 * 35) + 35, "the park's formula");

int sc_cs_stage_attr(sc_ctx* ctx, int F, int h, int D, cs_stage_plan* plan) {
    const int np = 2 * h + 1, nt = 2 * (h + D) + 1;
    plan->tab_lds = sizeof(double) * (size_t)nt * F <= PF_TAB_LDS;
    plan->lds = pf_lds_bytes(np, nt, F, true, plan->tab_lds);
    return sc_lds_attr(ctx, (const void*)(plan->tab_lds ? k_cs_stage<true> : k_cs_stage<false>), plan->lds);
}

int sc_cs_stage_launch(sc_ctx* ctx, const cs_stage_plan& plan, const double* z, int ny, int nx, int F, int h, int w, int D,
                       double de, int min_samples, int mode, const double* d_tab, const double* d_terms, bool park_prof,
                       const sg_stage& st) {
    const auto k_stage = plan.tab_lds ? k_cs_stage<true> : k_cs_stage<false>;
    int launches = 0;
    if (st.m) {
        k_stage<<<pf_grid(st.m), PF_THREADS, plan.lds, ctx->stream>>>(z, ny, nx, st.cells, st.dirs, st.m, F, h, w, D, de, min_samples,
                                                                      mode, d_tab, d_terms, park_prof ? st.prof : nullptr, st.cn,
                                                                      st.used, st.scal, st.planes, st.shift);
        ++launches;
    }
    sc_sg_rank_launch(ctx, st);
    return launches + 1;
}

static int cs_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  const long long* seg_start, const int32_t* seg_label, long long S, const double* freqs, int F, int h,
                  int w, int D, int mode, double de, double delta, int min_samples, int min_profiles,
                  sc_segment_fit* out_rows, sc_channel_segment_cell* out_cells, double* out_sse, int8_t* out_shift) {
    if (S == 0) return SC_OK;
    const bool own = mode == SC_CHANNEL_DEPTH_PROFILE;
    cs_stage_plan plan;
    int rc;
    if ((rc = sc_cs_stage_attr(ctx, F, h, D, &plan))) return rc;
    if (!own && (rc = sc_sg_grid_attr(ctx, F, h, D))) return rc;

    sg_call c = {cells, sa, ca, seg_start, seg_label, S, freqs, F, h + D, de, cs_park(F, h), CS_MAX_SEGS, nullptr, 0, 1};
    // (rows and cells end in padding; d_ci comes back from where it is parked)
    c.out = {{out_rows, &ctx->sg_rows, sizeof(sc_segment_fit), SG_SEGS, true},
             {out_cells, &ctx->sg_out, sizeof(sc_channel_segment_cell), SG_CELLS, true},
             {out_sse, &ctx->sg_sse, sizeof(double) * F, SG_SEGS},
             {out_shift, &ctx->sg_shift, (size_t)F, SG_CELLS}};
    const double* d_terms = nullptr;
    // (the frame's table over h + D has the size of G, which takes its place: k.tab is G from here on)
    c.tables = [&](const double* d_freqs) { return sc_ch_tables(ctx, d_freqs, F, h, D, de, (double*)ctx->sg_tab.p, &d_terms); };
    c.launch = [&](const sg_chunk& k) {
        const sg_stage& st = k.st;
        const long long m = st.m;
        const size_t mF = (size_t)m * F;
        int launches = sc_cs_stage_launch(ctx, plan, z, ny, nx, F, h, w, D, de, min_samples, mode, k.tab, d_terms, !own, st);
        if (k.G && own) {
            sc_sg_sum_launch(ctx, st.planes, st, k.blk, k.G, F, 2, k.part, k.tot);
            launches += 2;
        } else if (k.G) {
            sc_sg_sum_launch(ctx, st.planes + 2 * mF, st, k.blk, k.G, F, 2, k.part, k.tot);
            sc_sg_resid_launch(ctx, k, F, h, D, de, min_profiles);
            sc_sg_sum_launch(ctx, st.planes + 2 * mF, st, k.blk, k.G, F, 1, k.part, k.tsum);
            launches += 5;
        }
        k_cs_choose<<<sg_grid(st.Sc), 64, 0, ctx->stream>>>(st.seg, st.label, st.cnt, st.Sc, m, k.tot, k.tsum, k.ages, F, D, delta,
                                                           min_profiles, mode, st.cells, st.cn, st.used, st.scal, st.planes, st.shift,
                                                           (sc_segment_fit*)k.out[0], (sc_channel_segment_cell*)k.out[1],
                                                           (double*)k.out[2]);
        return launches + 1;
    };
    return sc_sg_chunks(ctx, c);
}

// the argument checks under the name `who`: ch_call's of the frequencies, then sc_sg_check's with the park's cap
int sc_cs_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                const double* freqs, int F, int h, int w, int D, int mode, double de, double delta, int min_samples,
                int min_profiles, const void* out_rows) {
    int rc = sc_ch_check_freqs(ctx, who, freqs, F);
    if (rc) return rc;
    if (mode != SC_CHANNEL_DEPTH_PROFILE && mode != SC_CHANNEL_DEPTH_SEGMENT)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: the depth mode must be SC_CHANNEL_DEPTH_PROFILE or SC_CHANNEL_DEPTH_SEGMENT", who);
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    if ((rc = sc_sg_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, freqs, F, h, w, D, de, delta, min_samples,
                          min_profiles, out_rows)))
        return rc;
    return sc_ch_check_arg(ctx, who, freqs, F, de);
}

// The two calls after their null checks: sc_cs_check, then the fit on z - ny x nx on the host, uploaded - or on the
// context's DEM (z null)
static int cs_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                   const double* freqs, int F, int h, int w, int D, int mode, double de, double delta, int min_samples,
                   int min_profiles, sc_segment_fit* out_rows, sc_channel_segment_cell* out_cells, double* out_sse,
                   int8_t* out_shift) {
    int rc = sc_cs_check(ctx, who, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, freqs, F, h, w, D, mode, de, delta,
                         min_samples, min_profiles, out_rows);
    if (rc) return rc;
    if (z && S == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->sg_z, z, ny, nx, &z_dev))) return rc;
    return cs_run(ctx, z_dev, ny, nx, cells, sa, ca, seg_start, seg_label, S, freqs, F, h, w, D, mode, de, delta, min_samples,
                  min_profiles, out_rows, out_cells, out_sse, out_shift);
}

extern "C" int sc_channel_segments(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                   const long long* seg_start, const int32_t* seg_label, long long S, const double* frequencies,
                                   int F, int h, int w, int D, int mode, double de, double delta, int min_samples,
                                   int min_profiles, sc_segment_fit* out_rows, sc_channel_segment_cell* out_cells,
                                   double* out_sse, int8_t* out_shift) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_channel_segments");
    if (rc) return rc;
    return cs_call(ctx, "sc_channel_segments", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, seg_start, seg_label, S, frequencies,
                   F, h, w, D, mode, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_shift);
}

extern "C" int sc_channel_segments_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                       const double* ca, long long K, const long long* seg_start, const int32_t* seg_label,
                                       long long S, const double* frequencies, int F, int h, int w, int D, int mode, double de,
                                       double delta, int min_samples, int min_profiles, sc_segment_fit* out_rows,
                                       sc_channel_segment_cell* out_cells, double* out_sse, int8_t* out_shift) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return cs_call(ctx, "sc_channel_segments_dem", z, ny, nx, cells, sa, ca, K, seg_start, seg_label, S, frequencies, F, h, w, D,
                   mode, de, delta, min_samples, min_profiles, out_rows, out_cells, out_sse, out_shift);
}
