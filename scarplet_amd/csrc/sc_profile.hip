// sc_fit_profiles* : scarp-profile dating across a trace (docs/profiles.md).
//
// For each cell a profile of 2h + 1 points is cut across the strike (each point the mean of up to 2w + 1 bilinear
// samples along the strike), and z(s) = c0 + b s + a erf(s / (2 sqrt(kt))) is fitted to it for each of A ages.  The
// pieces are those of sc_fit.h; a kernel here is the order in which it calls them.
//   k_pf_table   the erf column of every (point, age): it depends on the cell in no way, so it is a table of
//                (2h + 1) x A float64, age-minor, built once per call
//   k_pf_fit     one wave per cell, PF_WAVES cells per workgroup, workgroups striding over the cells so that the
//                cells in flight are neighbours of the input order (cells of one trace share their samples' lines)
//     pf_cut       lanes over the points j; the profile goes to the wave's slice of LDS, NaN marking a point without
//                  a valid sample
//     the fit      lanes over the AGES: lane i walks the whole profile for age i - the profile is an LDS broadcast,
//                  the table row j is A consecutive doubles - in four sweeps: pf_moments and pf_line with the lane's
//                  column in the same sweep, pf_rest, pf_sse.  Every sum is a plain loop over ascending j in one
//                  lane: no cross-lane reduction, the same bits every run, and a profile with missing points is the
//                  same code as a complete one.
//     pf_choose    argmin over the lanes (ties to the smaller age index), a ballot of sse <= thr for the interval
//   k_pf_shift   sc_fit_profiles_shift: the same wave per cell, pf_cut and LDS profile; the table covers
//                j = -(h + D)..(h + D).  pf_moments and pf_line without a column, once; then the lanes run over the
//                (shift, age) pairs (sh_search), whose winners per age come back in the wave's slot of LDS, and
//                pf_choose runs on sse*.
// The table sits in LDS when it fits PF_TAB_LDS bytes (35 ages at h = 100: 56 KB) and in global memory otherwise
// (pf_stage).  No atomics at all.  Both kernels run in sc_fit.h's loop (pf_each_cell).
// The host side owns the frame of EVERY per-cell call - these, sc_ramp.hip, sc_robust.hip and sc_lateral.hip: sc_pf_dem
// (the DEM on the host, or the context's), sc_pf_table and sc_pf_chunks, the chunked driver, which a call hands its
// launch line as a lambda.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

__global__ __launch_bounds__(256) void k_pf_table(const double* __restrict__ ages, int A, int h, double de,
                                                  double* __restrict__ tab) {
    const int total = (2 * h + 1) * A;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        const int jj = idx / A, i = idx - jj * A;
        const double s = (double)(jj - h) * de;
        tab[idx] = erf(s / (2.0 * sqrt(ages[i])));
    }
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_fit(const double* __restrict__ z, int ny, int nx,
                                                       const long long* __restrict__ cells,
                                                       const double* __restrict__ dir, long long K,
                                                       const double* __restrict__ ages, int A, int h, int w, double de,
                                                       double delta, int min_samples, const double* __restrict__ tab_g,
                                                       sc_profile_fit* __restrict__ rows, double* __restrict__ curve) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63;
    const pf_lds L = pf_stage<TAB_LDS, false>(tab_g, np, np, A);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    const double* col = L.tab + ia;
    pf_each_cell(
        cells, K, [&](long long kc, long long cell) { pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, L.prof, nullptr); },
        [&](long long kc, long long cell) {
            const pf_mom mo = pf_moments<true>(L.prof, np, h, de, col, A);
            sc_profile_fit* out = rows + kc;
            if (mo.n_neg < min_samples || mo.n_pos < min_samples) {
                if (lane == 0) pf_row_unfit(out, cell, mo.n);
                pf_unfit_planes(kc, lane, A, curve, nullptr);
            } else {
                pf_col t;
                const pf_lin f = pf_line<true>(L.prof, np, h, de, mo, col, A, t);
                pf_rest(L.prof, np, h, de, f, pf_at(col, A), t);
                const double a = t.Sep / t.See;
                double b, c0;
                pf_slope(f.sbar, f.pbar, f.beta, t.ebar, t.gamma, a, b, c0);
                const double sse = pf_sse(L.prof, np, h, de, pf_at(col, A), a, b, c0);
                if (curve && lane < A) curve[kc * A + lane] = sse;
                const int dof = mo.n - 3;
                const pf_pick k = pf_choose(sse, lane, A, delta, dof);
                if (lane == k.best) pf_row_fit(out, cell, mo.n, k, pf_open(k, A), ages, a, b, c0, sse, dof);
            }
        });
}

template <bool TAB_LDS>
__global__ __launch_bounds__(PF_THREADS) void k_pf_shift(const double* __restrict__ z, int ny, int nx,
                                                         const long long* __restrict__ cells,
                                                         const double* __restrict__ dir, long long K,
                                                         const double* __restrict__ ages, int A, int h, int w, int D,
                                                         double de, double delta, int min_samples,
                                                         const double* __restrict__ tab_g,
                                                         sc_profile_shift_fit* __restrict__ rows,
                                                         double* __restrict__ curve, signed char* __restrict__ shifts) {
    const int np = 2 * h + 1;
    const int lane = threadIdx.x & 63;
    const pf_lds L = pf_stage<TAB_LDS, true>(tab_g, np, 2 * (h + D) + 1, A);
    const double* slot = L.slot;
    const int* srank = (const int*)(slot + (size_t)SH_TERMS * A);
    const int ia = min(lane, A - 1);                     // lanes beyond the ages repeat the last one and are ignored
    pf_each_cell(
        cells, K, [&](long long kc, long long cell) { pf_cut(z, ny, nx, cell, dir, kc, h, w, lane, L.prof, nullptr); },
        [&](long long kc, long long cell) {
            // what depends on neither the age nor the shift, once
            const pf_mom mo = pf_moments<false>(L.prof, np, h, de, nullptr, A);
            const int dof = mo.n - 3 - (D > 0 ? 1 : 0);
            sc_profile_shift_fit* out = rows + kc;
            if (mo.n_neg < min_samples || mo.n_pos < min_samples || dof < 1) {
                if (lane == 0) {
                    pf_row_unfit(out, cell, mo.n);
                    out->shift_index = 0;
                    out->shift = __builtin_nan("");
                }
                pf_unfit_planes(kc, lane, A, curve, shifts);
            } else {
                pf_col t;
                const pf_lin f = pf_line<false>(L.prof, np, h, de, mo, nullptr, A, t);
                sh_search(L.prof, L.tab, np, h, A, D, de, lane, f, L.slot);
                // lane i takes age i's winner
                const double sse = slot[ia];
                const int d = sh_shift_of(srank[ia]);
                if (curve && lane < A) curve[kc * A + lane] = sse;
                if (shifts && lane < A) shifts[kc * A + lane] = (signed char)d;
                const pf_pick k = pf_choose(sse, lane, A, delta, dof);
                if (lane == k.best) {
                    const double a = slot[2 * A + ia] / slot[A + ia];
                    double b, c0;
                    pf_slope(f.sbar, f.pbar, f.beta, slot[3 * A + ia], slot[4 * A + ia], a, b, c0);
                    pf_row_fit(out, cell, mo.n, k, pf_open(k, A) + (D > 0 && (d == D || d == -D) ? 8 : 0), ages, a, b, c0, sse,
                               dof);
                    out->shift_index = d;
                    out->shift = (double)d * de;
                }
            }
        });
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// (shared with sc_fit_segments: `who` names the call in the messages)
int sc_pf_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const double* ages, int A, int h, int w, double de, double delta,
                int min_samples, const void* out_rows) {
    if (K < 0 || (K > 0 && (!cells || !sa || !ca || !out_rows)) || !ages)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (ny < 2 || nx < 2) return sc_fail(ctx, SC_ERR_INVALID, "%s: the grid must be at least 2 x 2", who);
    if (A < 1 || h < 1 || w < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: needs A >= 1, h >= 1, w >= 0", who);
    if (A > SC_PROFILE_MAX_AGES) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %d ages, more than %d", who, A, SC_PROFILE_MAX_AGES);
    if (h > SC_PROFILE_MAX_HALF) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: half-length %d cells, more than %d", who, h, SC_PROFILE_MAX_HALF);
    if (w > SC_PROFILE_MAX_SWATH) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: swath %d cells, more than %d", who, w, SC_PROFILE_MAX_SWATH);
    if (K > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %lld cells, more than 2^31 - 1", who, K);
    if (min_samples < 2 || min_samples > h)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: min_samples must lie in 2..h", who);
    if (!(isfinite(delta) && delta >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: delta must be finite and >= 0", who);
    if (!(isfinite(de) && de > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the cell size must be finite and > 0", who);
    for (int i = 0; i < A; ++i)
        if (!(isfinite(ages[i]) && ages[i] > 0.0 && (i == 0 || ages[i] > ages[i - 1])))
            return sc_fail(ctx, SC_ERR_INVALID, "%s: ages must be finite, positive and strictly increasing", who);
    const long long nc = ny * nx;
    for (long long k = 0; k < K; ++k) {
        if (cells[k] < 0 || cells[k] >= nc) return sc_fail(ctx, SC_ERR_INVALID, "%s: cell %lld outside the grid", who, cells[k]);
        if (!(isfinite(sa[k]) && isfinite(ca[k]))) return sc_fail(ctx, SC_ERR_INVALID, "%s: sa / ca not finite at cell %lld", who, k);
    }
    return SC_OK;
}


// (shared with sc_fit_segments_shift)
int sc_pf_check_shift(sc_ctx* ctx, const char* who, int h, int D, int min_samples) {
    if (D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: the shift range must be >= 0 cells", who);
    if (D > SC_PROFILE_MAX_SHIFT) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a shift of %d cells, more than %d", who, D, SC_PROFILE_MAX_SHIFT);
    if (D > h - min_samples)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: a shift of %d cells, more than h - min_samples = %d", who, D, h - min_samples);
    return SC_OK;
}

int sc_pf_whole_grid(sc_ctx* ctx, const char* who) {
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const Geom& g = ctx->g;
    if (g.ly != g.ny || g.lx != g.nx || g.gy0 != 0 || g.gx0 != 0 || g.cy0 != 0 || g.cx0 != 0 || g.cy1 != g.ny || g.cx1 != g.nx)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: the context holds a block of a larger grid", who);
    return SC_OK;
}

int sc_pf_upload(sc_ctx* ctx, DevBuf& buf, const double* z, int ny, int nx) {
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * (size_t)ny * (size_t)nx;
    int rc = sc_ensure(ctx, buf, bytes);
    if (rc) return rc;
    SC_HIP(ctx, hipMemcpyAsync(buf.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SC_OK;
}

int sc_pf_table(sc_ctx* ctx, const double* d_ages, int A, int h, double de, double* d_tab) {
    const int np = 2 * h + 1;
    sc_prof_begin(ctx, SC_K_PROFILE);
    k_pf_table<<<std::max(1, std::min(256, (np * A + 255) / 256)), 256, 0, ctx->stream>>>(d_ages, A, h, de, d_tab);
    SC_HIP(ctx, hipGetLastError());
    sc_prof_end(ctx, 1);
    return SC_OK;
}

int sc_pf_dem(sc_ctx* ctx, DevBuf& buf, const double* z, int ny, int nx, const double** z_dev) {
    if (!z) {
        SC_HIP(ctx, hipSetDevice(ctx->device));
        *z_dev = ctx->z_dev;
        return SC_OK;
    }
    int rc = sc_pf_upload(ctx, buf, z, ny, nx);
    *z_dev = (const double*)buf.p;
    return rc;
}

int sc_pf_chunks(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K, long long chunk,
                 size_t row_bytes, void* out_rows, const pf_plane& p0, const pf_plane& p1, const pf_launch& launch) {
    const pf_plane planes[2] = {p0, p1};
    chunk = std::min(K, sc_fit_chunk_bound(chunk, ctx->fit_chunk));
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_cells, sizeof(long long) * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_dir, sizeof(double) * 2 * (size_t)chunk))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_rows, row_bytes * (size_t)chunk))) return rc;
    pf_chunk d = {(long long*)ctx->pf_cells.p, (double*)ctx->pf_dir.p, ctx->pf_rows.p, {nullptr, nullptr}};
    for (int p = 0; p < 2; ++p) {
        if (!planes[p].host) continue;
        if ((rc = sc_ensure(ctx, *planes[p].buf, planes[p].cell_bytes * (size_t)chunk))) return rc;
        d.plane[p] = planes[p].buf->p;
    }
    std::vector<double> dir;
    for (long long k0 = 0; k0 < K; k0 += chunk) {
        const long long m = std::min(chunk, K - k0);
        dir.resize(2 * (size_t)m);
        for (long long k = 0; k < m; ++k) {
            dir[2 * k] = sa[k0 + k];
            dir[2 * k + 1] = ca[k0 + k];
        }
        SC_HIP(ctx, hipMemcpyAsync(d.cells, cells + k0, sizeof(long long) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        SC_HIP(ctx, hipMemcpyAsync(d.dir, dir.data(), sizeof(double) * 2 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        // (the rows' padding is part of what the caller compares: cleared, the kernel writes the fields)
        SC_HIP(ctx, hipMemsetAsync(d.rows, 0, row_bytes * (size_t)m, ctx->stream));
        sc_prof_begin(ctx, SC_K_PROFILE);
        launch(d, m);
        SC_HIP(ctx, hipGetLastError());
        sc_prof_end(ctx, 1);
        SC_HIP(ctx, hipMemcpyAsync((char*)out_rows + row_bytes * (size_t)k0, d.rows, row_bytes * (size_t)m, hipMemcpyDeviceToHost,
                                   ctx->stream));
        for (int p = 0; p < 2; ++p)
            if (planes[p].host)
                SC_HIP(ctx, hipMemcpyAsync((char*)planes[p].host + planes[p].cell_bytes * (size_t)k0, d.plane[p],
                                           planes[p].cell_bytes * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        // (dir is reused by the next chunk, and the caller owns the outputs on return)
        SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SC_OK;
}

// D < 0: the call without a shift, its kernel and its rows (sc_profile_fit; sc_profile_shift_fit otherwise)
static int pf_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples,
                  void* out_rows, double* out_sse, int8_t* out_shift) {
    if (K == 0) return SC_OK;
    const bool shift = D >= 0;
    const int np = 2 * h + 1, ht = h + (shift ? D : 0), nt = 2 * ht + 1;
    const size_t tab_bytes = sizeof(double) * (size_t)nt * A;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->pf_ages, sizeof(double) * A))) return rc;
    if ((rc = sc_ensure(ctx, ctx->pf_tab, tab_bytes))) return rc;
    double* d_ages = (double*)ctx->pf_ages.p;
    double* d_tab = (double*)ctx->pf_tab.p;

    const bool tab_lds = tab_bytes <= PF_TAB_LDS;
    const size_t lds = pf_lds_bytes(np, nt, A, shift, tab_lds);
    const auto k_fit = tab_lds ? k_pf_fit<true> : k_pf_fit<false>;
    const auto k_shift = tab_lds ? k_pf_shift<true> : k_pf_shift<false>;
    if ((rc = sc_lds_attr(ctx, shift ? (const void*)k_shift : (const void*)k_fit, lds))) return rc;

    SC_HIP(ctx, hipMemcpyAsync(d_ages, ages, sizeof(double) * A, hipMemcpyHostToDevice, ctx->stream));
    // (rows -h..h of the table over h + D are the bits of the table over h: s = (double)j * de either way)
    if ((rc = sc_pf_table(ctx, d_ages, A, ht, de, d_tab))) return rc;

    const pf_plane curve = {out_sse, &ctx->pf_sse, sizeof(double) * (size_t)A}, shifts = {out_shift, &ctx->pf_shift, (size_t)A};
    return sc_pf_chunks(ctx, cells, sa, ca, K, PF_CHUNK, shift ? sizeof(sc_profile_shift_fit) : sizeof(sc_profile_fit), out_rows,
                        curve, shifts, [&](const pf_chunk& d, long long m) {
        if (shift)
            k_shift<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, d_ages, A, h, w, D, de, delta,
                                                                 min_samples, d_tab, (sc_profile_shift_fit*)d.rows,
                                                                 (double*)d.plane[0], (signed char*)d.plane[1]);
        else
            k_fit<<<pf_grid(m), PF_THREADS, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, d_ages, A, h, w, de, delta, min_samples,
                                                               d_tab, (sc_profile_fit*)d.rows, (double*)d.plane[0]);
    });
}

// The four calls after their null checks: the argument checks under the name `who`, then the fit on z - ny x nx on the
// host, uploaded - or on the context's DEM (z null).  shift: D is the caller's range, checked here.
static int pf_call(sc_ctx* ctx, const char* who, bool shift, const double* z, int ny, int nx, const long long* cells,
                   const double* sa, const double* ca, long long K, const double* ages, int A, int h, int w, int D, double de,
                   double delta, int min_samples, void* out_rows, double* out_sse, int8_t* out_shift) {
    int rc = sc_pf_check(ctx, who, ny, nx, cells, sa, ca, K, ages, A, h, w, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if (shift && (rc = sc_pf_check_shift(ctx, who, h, D, min_samples))) return rc;
    if (z && K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    return pf_run(ctx, z_dev, ny, nx, cells, sa, ca, K, ages, A, h, w, shift ? D : -1, de, delta, min_samples, out_rows, out_sse,
                  out_shift);
}

extern "C" int sc_fit_profiles(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                               const double* ages, int A, int h, int w, double de, double delta, int min_samples,
                               sc_profile_fit* out_rows, double* out_sse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_profiles");
    if (rc) return rc;
    return pf_call(ctx, "sc_fit_profiles", false, nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, ages, A, h, w, 0, de, delta,
                   min_samples, out_rows, out_sse, nullptr);
}

// (reports as sc_fit_profiles)
extern "C" int sc_fit_profiles_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                   const double* ca, long long K, const double* ages, int A, int h, int w, double de,
                                   double delta, int min_samples, sc_profile_fit* out_rows, double* out_sse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return pf_call(ctx, "sc_fit_profiles", false, z, ny, nx, cells, sa, ca, K, ages, A, h, w, 0, de, delta, min_samples, out_rows,
                   out_sse, nullptr);
}

extern "C" int sc_fit_profiles_shift(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K,
                                     const double* ages, int A, int h, int w, int D, double de, double delta,
                                     int min_samples, sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_fit_profiles_shift");
    if (rc) return rc;
    return pf_call(ctx, "sc_fit_profiles_shift", true, nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, ages, A, h, w, D, de, delta,
                   min_samples, out_rows, out_sse, out_shift);
}

extern "C" int sc_fit_profiles_shift_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells,
                                         const double* sa, const double* ca, long long K, const double* ages, int A, int h,
                                         int w, int D, double de, double delta, int min_samples,
                                         sc_profile_shift_fit* out_rows, double* out_sse, int8_t* out_shift) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return pf_call(ctx, "sc_fit_profiles_shift_dem", true, z, ny, nx, cells, sa, ca, K, ages, A, h, w, D, de, delta, min_samples,
                   out_rows, out_sse, out_shift);
}
