// sc_snr_surface: the search's float64 SNR surface at chosen cells (docs/surface.md).
//
// sc_match keeps per cell the template that scored best and nothing of the rest.  This call returns, for K cells, the float64
// score of EVERY template of an (age, orientation) grid - match_template() (core.py:297-377) as the real-space closed form,
// k_score_f64's arithmetic - and what the surface says about the maximum: the run of ages and the run of orientations that
// score within `keep` of it, and how many templates do.
//
// The float64 scorers that exist score pair by pair: k_score_f64 a workgroup per (cell, template) over whole boxes, k_st_score
// a wave per listed pair over the runs.  For many cells x the whole grid that fetches every curvature value once per age: all
// ages of an orientation read the same curvature at the same taps.  Here:
//   score_prepare_f64, sc_window_runs   the settle's preparation: float64 windows, stencil planes, n and sum(W**2) in a fixed
//                                       order, the runs of the window rows
//   k_sf_union                          per orientation and row of its union box the span all its ages' runs lie in
//   k_sf_score                          a workgroup per (SF_CB consecutive cells of the list, orientation): the curvature of a
//                                       group of union rows is mixed once per cell and staged in LDS; a thread per (age, cell)
//                                       then walks the age's runs over the stage and keeps its two sums in registers
//   k_sf_reduce                         a wave per cell: first maximum, the two walks, n_within, the row
// No atomics on floating-point values and no order that depends on scheduling: the same bytes on every run.
#include "sc_fit_chunk.h"
#include "sc_internal.h"
#include <algorithm>
#include <math.h>

constexpr int SF_CB = 8;                       // cells per workgroup of k_sf_score (the reduction below is written for 8)
constexpr int SF_TILE = 512;                   // taps per cell the stage holds: SF_CB * SF_TILE doubles = 32 KB of LDS
constexpr int SF_STRIDE = SF_TILE + 4;         // ... a cell's taps 8 banks apart from the next cell's: the 8 cells of a tap read without conflict
constexpr int SF_THREADS = 512;                // threads of k_sf_score: one per (age of the pass, cell)
constexpr int SF_AP = SF_THREADS / SF_CB;      // ages per pass over the union box
constexpr size_t SF_CUBE_BYTES = (size_t)256 << 20;   // bound of the two score cubes on the device: the cells go through in chunks

// what the host knows of an orientation's union box: its rows pmin .. pmax and where their spans start in the table
struct OrientDev {
    int32_t pmin, pmax;
    uint32_t uoff;
    int32_t pad;
};

// The span of every row of an orientation's union box: from the first to the last column (as q, relative to the cell) any of
// its ages' runs covers; per orientation the widest span.  grid = (ceil(rows / 256), orientations), a thread per row.
// (atomicMax on integers: the same value in whatever order)
__global__ void __launch_bounds__(256)
k_sf_union(const TemplDev* __restrict__ templ, int n_par, const unsigned* __restrict__ soff, const int2* __restrict__ spans,
           const OrientDev* __restrict__ orient, int2* __restrict__ uspan, int* __restrict__ usw) {
    const int ib = blockIdx.y;
    const OrientDev od = orient[ib];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > od.pmax - od.pmin) return;
    const int p = od.pmin + r;
    int lo = INT_MAX, hi = INT_MIN;
    for (int ia = 0; ia < n_par; ++ia) {
        const int it = ib * n_par + ia;
        const int a = p - templ[it].pmin;
        if (a < 0 || a >= templ[it].wh) continue;
        const int2 sp = spans[soff[it] + a];
        if (sp.y < sp.x) continue;
        lo = min(lo, templ[it].qmin + sp.x);
        hi = max(hi, templ[it].qmin + sp.y);
    }
    uspan[od.uoff + r] = hi >= lo ? make_int2(lo, hi) : make_int2(0, -1);
    if (hi >= lo) atomicMax(usw + ib, hi - lo + 1);
}

// match_template() in float64 of SF_CB cells x the ages of one orientation.  grid = (batches of SF_CB cells, orientations):
// the workgroups of an orientation follow each other, so those that run together share its windows in L2.
//
// The orientation's union box is walked in tiles of RG rows x CW columns of the rows' union spans (CW = min(widest span,
// SF_TILE), RG = SF_TILE / CW: a thin young scarp's rows are a few taps wide and a tile holds many of them, an old scarp's or a
// Ricker's are hundreds wide and a tile holds one or a part of one).  Per tile:
//   1. all threads: the curvature of every tap and cell - three plane values at ((i - p + oy) mod ny, (j - q + ox) mod nx),
//      mixed as k_score_f64 mixes them - into stage[cell][row][column], float64
//   2. barrier; thread (age, cell) walks the age's runs inside the tile tap by tap: xc += w * cv, t3 += cv * cv where w != 0.
//      The 8 threads of an age read the same weight (one fetch) and 8 stage words 8 banks apart; the sums stay in the
//      thread's registers from the first tile to the last - one fixed order of additions per (cell, template), no reduction
//      across lanes at all, so the bytes do not depend on the batch a cell lands in
// When the box is done the thread forms amp and snr (k_score_f64's last block, masks included) and stores them.
// More than SF_AP = 64 ages go through in passes of 64 (the stage is then filled once per pass).
// (Measured and replaced: a wave per age with lanes over the taps and a shuffle tree per (age, tile) - an old scarp's union
//  rows are hundreds of taps wide, a tile then holds one row, and the tree and the wave's load chain per (age, tile) cost
//  more than the taps: 2466 ms for 10 000 cells of the 4096^2 workload, no faster than a workgroup per pair.)
__global__ void __launch_bounds__(SF_THREADS)
k_sf_score(const double* __restrict__ pa, const double* __restrict__ pb, const double* __restrict__ pc, Geom g,
           const TemplDev* __restrict__ templ, int n_par, int n_t, const double* __restrict__ sums,
           const double* __restrict__ xaxis, const double* __restrict__ yaxis,
           const unsigned long long* __restrict__ woff, const double* __restrict__ wbuf,
           const unsigned* __restrict__ soff, const int2* __restrict__ spans, const int* __restrict__ maxlen,
           const double* __restrict__ mix, const OrientDev* __restrict__ orient, const int2* __restrict__ uspan,
           const int* __restrict__ usw, const int* __restrict__ cells, int K,
           double* __restrict__ amp_out, double* __restrict__ snr_out) {
    __shared__ double stage[SF_CB * SF_STRIDE];
    __shared__ int cell_i[SF_CB], cell_j[SF_CB];
    const int ib = blockIdx.y, k0 = blockIdx.x * SF_CB;
    const int tid = threadIdx.x;
    if (tid < SF_CB) {
        const int k = min(k0 + tid, K - 1);                                // (beyond the list: the last cell again, not stored)
        cell_i[tid] = cells[2 * k];
        cell_j[tid] = cells[2 * k + 1];
    }
    const OrientDev od = orient[ib];
    const int UH = od.pmax - od.pmin + 1;
    const int sw = max(usw[ib], 1);
    const int CW = min(sw, SF_TILE), RG = SF_TILE / CW;
    const int t0 = ib * n_par;
    // the orientation's curvature mix (k_score_f64): the host has checked that all its ages carry the same
    const TemplDev tf = templ[t0];
    double ca = tf.cos_a, sa = -tf.sin_a;
    double k_cc = __dmul_rn(ca, ca), k_ss = __dmul_rn(sa, sa);
    if (tf.kind == SC_KIND_WINDOW) sc_window_mix(mix, t0, ca, sa, k_cc, k_ss);
    const int2* __restrict__ us_o = uspan + od.uoff;
    const int ai = tid / SF_CB, c = tid - ai * SF_CB;                      // this thread's age of the pass and its cell

    for (int ia0 = 0; ia0 < n_par; ia0 += SF_AP) {
        const bool act = ia0 + ai < n_par;
        const int it = t0 + (act ? ia0 + ai : 0);
        const int t_pmin = templ[it].pmin, t_qmin = templ[it].qmin, t_wh = templ[it].wh, t_ww = templ[it].ww;
        const double* __restrict__ wt = wbuf + woff[it];
        const int2* __restrict__ sp_t = spans + soff[it];
        double xc = 0.0, t3 = 0.0;
        for (int r0 = 0; r0 < UH; r0 += RG) {
            for (int c0 = 0; c0 < sw; c0 += CW) {
                __syncthreads();                                           // (the tile before is done with; cell_i is written)
                // ---- 1. the stage ----
                for (int e = tid; e < RG * CW; e += SF_THREADS) {
                    const int r = e / CW, kc = e - r * CW;
                    const int row = r0 + r;
                    int2 us = make_int2(0, -1);
                    if (row < UH) us = us_o[row];
                    const int q = us.x + c0 + kc;
                    const bool v = q <= us.y;
                    const int p = od.pmin + row;
#pragma unroll
                    for (int cc = 0; cc < SF_CB; ++cc) {
                        double cv = 0.0;
                        if (v) {
                            const int li = wrap_index(cell_i[cc] - p + g.oy, g.ny), lj = wrap_index(cell_j[cc] - q + g.ox, g.nx);
                            const size_t o = (size_t)li * g.lx + lj;
                            const double A = pa[o], Bc = pb[o], C = pc[o];
                            cv = __dadd_rn(__dsub_rn(__dmul_rn(A, k_cc), __dmul_rn(__dmul_rn(__dmul_rn(2.0, Bc), sa), ca)),
                                           __dmul_rn(C, k_ss));
                        }
                        stage[cc * SF_STRIDE + e] = cv;
                    }
                }
                __syncthreads();
                // ---- 2. every (age, cell) of the pass walks the age's runs inside the tile ----
                if (!act) continue;
                // rows of the tile this age has: a = p - pmin in [0, wh)
                const int r_lo = max(0, t_pmin - od.pmin - r0), r_hi = min(min(RG, UH - r0), t_pmin + t_wh - od.pmin - r0);
                for (int r = r_lo; r < r_hi; ++r) {
                    const int row = r0 + r, a = od.pmin + row - t_pmin;
                    const int2 sp = sp_t[a];
                    const int shift = t_qmin - us_o[row].x - c0;          // column of the stage = b + shift
                    const int b_lo = max(sp.x, -shift), b_hi = min(sp.y, CW - 1 - shift);
                    const double* __restrict__ wr = wt + (size_t)a * t_ww;
                    const double* st = stage + c * SF_STRIDE + r * CW + shift;
#pragma unroll 4
                    for (int b = b_lo; b <= b_hi; ++b) {
                        const double w = wr[b];
                        const double cv = st[b];
                        const double m = w != 0.0 ? cv : 0.0;              // (W != 0 is the mask M, core.py:348)
                        xc = fma(w, cv, xc);
                        t3 = fma(m, m, t3);
                    }
                }
            }
        }
        // ---- the closed form: k_score_f64's last block ----
        if (act && k0 + c < K) {
            const TemplDev t = templ[it];
            const int i = cell_i[c], j = cell_j[c];
            const double n = sums[2 * it] + SC_EPS, ts = sums[2 * it + 1];
            double amp = xc / ts;
            const double T1 = ts * (amp * amp);
            const double err = (1.0 / n) * (T1 - 2.0 * amp * xc + t3) + SC_EPS;
            double snr = fabs(T1 / err);
            if (t.flags & (SC_FLAG_ERR_XR_LE0 | SC_FLAG_ERR_XR_GE0)) {
                const double xr = __dadd_rn(__dmul_rn(xaxis[j], t.cos_a), __dmul_rn(yaxis[i], t.sin_a));
                if ((t.flags & SC_FLAG_ERR_XR_LE0) ? (xr <= 0.0) : (xr >= 0.0)) snr = 0.0;
            }
            if (!(i >= t.ilo && i <= t.ihi && j >= t.jlo && j <= t.jhi)) { amp = 0.0; snr = 0.0; }
            sc_window_masks(t, g, i, j, amp, snr);
            const size_t oo = (size_t)(k0 + c) * n_t + it;
            amp_out[oo] = amp;
            snr_out[oo] = snr;
        }
    }
}

static __device__ __forceinline__ double sf_clean(double v) { return v == v ? v : -HUGE_VAL; }      // a NaN score counts as -inf

// One wave per cell (four cells a workgroup): the definition of docs/surface.md on the cell's n_ang x n_par scores.
//   best     lanes strided over the templates, each keeping its first maximum; a butterfly on the key (score, earlier template)
//   P, Q     P[ia] = max over orientations, Q[ib] = max over ages, into pq (LDS; global memory where the grid is too long)
//   walks    lane 0, down and up from the maximum while the neighbour stays >= thr = best * keep; they do not wrap
//   n_within ballots over S >= thr
// Comparisons of float64 values alone decide, and maxima are exact: bit for bit tests/surface_reference.py.
__global__ void __launch_bounds__(256)
k_sf_reduce(const double* __restrict__ snr, const double* __restrict__ amp, int n_par, int n_ang, int K, double keep,
            double* __restrict__ pq_global, sc_surface_row* __restrict__ rows) {
    extern __shared__ double pq_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wv, kk = min(k, K - 1);
    const int n_t = n_par * n_ang;
    const double* __restrict__ S = snr + (size_t)kk * n_t;
    double* P = pq_global ? pq_global + (size_t)(blockIdx.x * 4 + wv) * (n_par + n_ang) : pq_lds + (size_t)wv * (n_par + n_ang);
    double* Q = P + n_par;
    double best = -HUGE_VAL;
    int bt = INT_MAX;
    for (int t = lane; t < n_t; t += 64) {
        const double v = sf_clean(S[t]);
        if (v > best) { best = v; bt = t; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(best, m, 64);
        const int ot = __shfl_xor(bt, m, 64);
        if (ov > best || (ov == best && ot < bt)) { best = ov; bt = ot; }
    }
    for (int ia = lane; ia < n_par; ia += 64) {
        double m = -HUGE_VAL;
        for (int ib = 0; ib < n_ang; ++ib) {
            const double v = sf_clean(S[(size_t)ib * n_par + ia]);
            m = v > m ? v : m;
        }
        P[ia] = m;
    }
    for (int ib = 0; ib < n_ang; ++ib) {                                    // (lanes over the ages of an orientation: whole lines of S)
        double m = -HUGE_VAL;
        for (int ia = lane; ia < n_par; ia += 64) {
            const double v = sf_clean(S[(size_t)ib * n_par + ia]);
            m = v > m ? v : m;
        }
        for (int sft = 32; sft >= 1; sft >>= 1) {                         // (a maximum: exact in any order)
            const double o = __shfl_xor(m, sft, 64);
            m = o > m ? o : m;
        }
        if (lane == 0) Q[ib] = m;
    }
    __threadfence_block();
    __syncthreads();
    const bool live = best > 0.0;
    const double thr = __dmul_rn(best, keep);
    int within = 0;
    for (int t0 = 0; t0 < n_t; t0 += 64) {
        const int t = t0 + lane;
        const bool in = live && t < n_t && sf_clean(S[t < n_t ? t : 0]) >= thr;
        within += __popcll(__ballot(in));
    }
    if (lane != 0 || k >= K) return;
    sc_surface_row r;
    if (!live) {
        // no score > 0: the cell lies outside every template's window limits
        r.par_index = r.ang_index = r.par_lo = r.par_hi = r.ang_lo = r.ang_hi = -1;
        r.n_within = 0;
        r.status = 1;
        r.snr = r.amp = __builtin_nan("");
    } else {
        const int ib = bt / n_par, ia = bt - ib * n_par;
        int plo = ia, phi = ia, alo = ib, ahi = ib;
        while (plo > 0 && P[plo - 1] >= thr) --plo;
        while (phi < n_par - 1 && P[phi + 1] >= thr) ++phi;
        while (alo > 0 && Q[alo - 1] >= thr) --alo;
        while (ahi < n_ang - 1 && Q[ahi + 1] >= thr) ++ahi;
        r.par_index = ia; r.ang_index = ib;
        r.par_lo = plo; r.par_hi = phi; r.ang_lo = alo; r.ang_hi = ahi;
        r.n_within = within;
        r.status = (plo == 0 ? 2 : 0) | (phi == n_par - 1 ? 4 : 0) | (alo == 0 ? 8 : 0) | (ahi == n_ang - 1 ? 16 : 0);
        r.snr = best;
        r.amp = amp[(size_t)kk * n_t + bt];
    }
    rows[k] = r;
}

static inline size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

extern "C" int sc_snr_surface(sc_ctx* ctx, const sc_template* t, int n_par, int n_ang, const int32_t* cells, long long K,
                              double keep, sc_surface_row* rows, double* snr, double* amp) {
    if (!ctx) return SC_ERR_INVALID;
    if (!t || n_par < 1 || n_ang < 1) return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: an empty grid (%d parameters x %d orientations)", n_par, n_ang);
    if (K < 0 || (K > 0 && (!cells || !rows))) return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: %lld cells without a list or without rows", K);
    if (K > 2147483647LL) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_snr_surface: %lld cells: more than 2^31 - 1", K);
    if (!(keep > 0.0 && keep <= 1.0)) return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: keep = 1 - drop must lie in (0, 1], got %g", keep);
    if ((long long)n_par * n_ang > 65535) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_snr_surface: %d x %d templates: more than 65535", n_par, n_ang);
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const Geom& g = ctx->g;
    if (!g.wrap) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_snr_surface: the context holds a block of a larger DEM; the surface needs the whole DEM");
    if (ctx->dem_nan > 0)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: the DEM has %lld NaN cells: every score would be NaN; fill them first", ctx->dem_nan);
    for (long long k = 0; k < K; ++k)
        if (cells[2 * k] < 0 || cells[2 * k] >= g.ny || cells[2 * k + 1] < 0 || cells[2 * k + 1] >= g.nx)
            return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: cell %lld (%d, %d) outside the %d x %d DEM", k, cells[2 * k], cells[2 * k + 1], g.ny, g.nx);
    const int n = n_par * n_ang;
    // orientation-major, and one curvature per orientation: k_sf_score mixes it once for all its ages
    for (int ib = 0; ib < n_ang; ++ib)
        for (int ia = 1; ia < n_par; ++ia) {
            const sc_template &a = t[(size_t)ib * n_par], &b = t[(size_t)ib * n_par + ia];
            const bool wa = a.kind == SC_KIND_WINDOW, wb = b.kind == SC_KIND_WINDOW;
            if (wa != wb || a.cc != b.cc || a.sc2 != b.sc2 || a.ss != b.ss || (!wa && (a.cos_a != b.cos_a || a.sin_a != b.sin_a)))
                return sc_fail(ctx, SC_ERR_INVALID, "sc_snr_surface: templates %d and %d of orientation %d differ in their curvature "
                               "(the table must be orientation-major, as Matcher.describe makes it)", ib * n_par, ib * n_par + ia, ib);
        }
    if (K == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = sc_load_templates(ctx, t, n))) return rc;                    // the scorers' table: nothing is matched, the record stays
    ctx->last_batch = 0;                          // (the scorers refuse the table until its sums are in place, below)
    sc_prof_begin(ctx, SC_K_SETTLE);              // (one bracket over the whole call: every return below closes it)
    struct ProfEnd { sc_ctx* c; ~ProfEnd() { sc_prof_end(c); } } prof_end{ctx};
    const unsigned long long* woff = nullptr;
    const double *wbuf = nullptr, *pa = nullptr, *mix = nullptr;
    if ((rc = score_prepare_f64(ctx, n, &woff, &wbuf, &pa, &mix))) return rc;
    // the union boxes of the orientations: rows from the descriptors, spans from the device
    std::vector<OrientDev> h_or(n_ang);
    size_t urows = 0;
    int uh_max = 1;
    for (int ib = 0; ib < n_ang; ++ib) {
        int pmin = INT_MAX, pmax = INT_MIN;
        for (int ia = 0; ia < n_par; ++ia) {
            const TemplDev& d = ctx->h_templ[(size_t)ib * n_par + ia];
            pmin = std::min(pmin, d.pmin);
            pmax = std::max(pmax, d.pmax);
        }
        h_or[ib] = OrientDev{pmin, pmax, (uint32_t)urows, 0};
        urows += (size_t)(pmax - pmin + 1);
        uh_max = std::max(uh_max, pmax - pmin + 1);
    }
    if (urows > 0x7FFFFFFFull) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_snr_surface: %zu rows of union boxes", urows);
    const size_t o_sums = 0, o_soff = o_sums + up64(16 * (size_t)n), o_mlen = o_soff + up64(4 * ((size_t)n + 1)),
                 o_or = o_mlen + up64(4 * (size_t)n), o_usw = o_or + up64(sizeof(OrientDev) * (size_t)n_ang),
                 o_usp = o_usw + up64(4 * (size_t)n_ang), o_end = o_usp + up64(sizeof(int2) * urows);
    if ((rc = sc_ensure(ctx, ctx->sf_work, o_end))) return rc;
    char* wk = (char*)ctx->sf_work.p;
    double* sums64 = (double*)(wk + o_sums);
    unsigned* soff = (unsigned*)(wk + o_soff);
    int* maxlen = (int*)(wk + o_mlen);
    OrientDev* d_or = (OrientDev*)(wk + o_or);
    int* usw = (int*)(wk + o_usw);
    int2* uspan = (int2*)(wk + o_usp);
    if ((rc = sc_window_runs(ctx, n, woff, wbuf, sums64, soff, maxlen))) return rc;
    // the table is now the float64 scorers' "last search": k_score_f64 reads n and sum(W**2) of its templates from ctx->sums,
    // which only a search fills - these are the table's own, from the float64 windows
    if ((rc = sc_ensure(ctx, ctx->sums, sizeof(double) * 2 * (size_t)n))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->sums.p, sums64, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->last_batch = n;
    SC_HIP(ctx, hipMemcpyAsync(d_or, h_or.data(), sizeof(OrientDev) * (size_t)n_ang, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemsetAsync(usw, 0, 4 * (size_t)n_ang, ctx->stream));
    hipLaunchKernelGGL(k_sf_union, dim3((uh_max + 255) / 256, n_ang), dim3(256), 0, ctx->stream, (const TemplDev*)ctx->templ.p, n_par,
                       (const unsigned*)soff, (const int2*)ctx->st_spans.p, (const OrientDev*)d_or, uspan, usw);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));                        // (h_or is a local; the descriptors have arrived)
    ctx->async_in_flight = false;

    // chunks of cells: the two cubes of a chunk stay within SF_CUBE_BYTES (at least one batch of cells)
    const size_t per_cell = 16 * (size_t)n;
    long long KC = (long long)(SF_CUBE_BYTES / per_cell) / SF_CB * SF_CB;
    KC = std::max<long long>(KC, SF_CB);
    KC = std::min<long long>(KC, (K + SF_CB - 1) / SF_CB * SF_CB);
    // (option "fit_chunk" lowers it, to whole batches of cells)
    KC = sc_fit_chunk_bound(KC, (ctx->fit_chunk + SF_CB - 1) / SF_CB * SF_CB);
    const bool pq_lds = (size_t)(n_par + n_ang) <= 2048;                   // four cells' P and Q in 64 KB of LDS
    const size_t pq_bytes = pq_lds ? 0 : up64(8 * (size_t)(n_par + n_ang) * (size_t)((KC + 3) / 4 * 4));
    if ((rc = sc_ensure(ctx, ctx->sf_cube, 2 * up64(8 * (size_t)n * (size_t)KC) + pq_bytes))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sf_cells, 8 * (size_t)KC))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sf_rows, sizeof(sc_surface_row) * (size_t)KC))) return rc;
    double* d_snr = (double*)ctx->sf_cube.p;
    double* d_amp = (double*)((char*)ctx->sf_cube.p + up64(8 * (size_t)n * (size_t)KC));
    double* d_pq = pq_lds ? nullptr : (double*)((char*)ctx->sf_cube.p + 2 * up64(8 * (size_t)n * (size_t)KC));
    int* d_cells = (int*)ctx->sf_cells.p;
    sc_surface_row* d_rows = (sc_surface_row*)ctx->sf_rows.p;
    const size_t lds_reduce = pq_lds ? 4 * 8 * (size_t)(n_par + n_ang) : 0;
    if (lds_reduce > 48 * 1024 && (rc = sc_lds_attr(ctx, (const void*)k_sf_reduce, lds_reduce))) return rc;
    const size_t npl = (size_t)g.ly * g.lx;
    for (long long k0 = 0; k0 < K; k0 += KC) {
        const int kc = (int)std::min<long long>(KC, K - k0);
        SC_HIP(ctx, hipMemcpyAsync(d_cells, cells + 2 * k0, 8 * (size_t)kc, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_sf_score, dim3((unsigned)((kc + SF_CB - 1) / SF_CB), (unsigned)n_ang), dim3(SF_THREADS), 0, ctx->stream,
                           pa, pa + npl, pa + 2 * npl, g, (const TemplDev*)ctx->templ.p, n_par, n, (const double*)sums64,
                           (const double*)ctx->xaxis.p, (const double*)ctx->yaxis.p, woff, wbuf, (const unsigned*)soff,
                           (const int2*)ctx->st_spans.p, (const int*)maxlen, mix, (const OrientDev*)d_or, (const int2*)uspan,
                           (const int*)usw, (const int*)d_cells, kc, d_amp, d_snr);
        hipLaunchKernelGGL(k_sf_reduce, dim3((unsigned)((kc + 3) / 4)), dim3(256), lds_reduce, ctx->stream, (const double*)d_snr,
                           (const double*)d_amp, n_par, n_ang, kc, keep, d_pq, d_rows);
        SC_HIP(ctx, hipGetLastError());
        SC_HIP(ctx, hipMemcpyAsync(rows + k0, d_rows, sizeof(sc_surface_row) * (size_t)kc, hipMemcpyDeviceToHost, ctx->stream));
        if (snr) SC_HIP(ctx, hipMemcpyAsync(snr + (size_t)k0 * n, d_snr, 8 * (size_t)n * kc, hipMemcpyDeviceToHost, ctx->stream));
        if (amp) SC_HIP(ctx, hipMemcpyAsync(amp + (size_t)k0 * n, d_amp, 8 * (size_t)n * kc, hipMemcpyDeviceToHost, ctx->stream));
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));                    // (the next chunk reuses the buffers)
    }
    return SC_OK;
}
