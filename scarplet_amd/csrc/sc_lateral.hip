// sc_lateral_offsets*: strike-slip offsets across a trace (docs/lateral.md).
//
// At each station (a cell and the strike's angle there) two fault-parallel profiles are cut, u on the -q side over
// t = -h..h and v on the +q side over t = -(h + D)..(h + D), each point the mean of a band of lines q0..q1 cells from the
// trace; for every lag d = -D..D the two are compared over the points where both are valid, each side keeping its own
// mean and line, and the lag with the smallest mean squared difference of the residuals wins.  The sampler is
// sc_fit.h's with the two axes exchanged (k = t, j = q); the candidates' order is sh_shift_of's.
//   k_lt_fit     one wave per station, the waves of a workgroup independent of one another (no workgroup barrier)
//     stage 1      lanes over t: u, then v, into the wave's LDS, every point's band summed in the fixed order of q
//     stage 2      lanes over the lag RANKS, 64 a round: a lane runs passes 0 to 2 of its lag over ascending t with its
//                  sums in registers - u_t is an LDS broadcast, v_{t + d} 64 neighbouring doubles - writes mse_d into
//                  the wave's LDS curve (and out_mse) and keeps its best (mse, rank) with n, rho, dz and tilt: a later
//                  round's lag wins only when strictly smaller, the ranks ascending from round to round
//     the choice   a butterfly argmin on the key (mse, rank) - a lane without a fitted lag holds (+inf, INT_MAX), the
//                  smaller rank wins a tie - then the winner's lane hands over what it kept; the walk of the interval
//                  and the parabola read the LDS curve, the same in every lane
// No atomics, no float sum across lanes: the same bytes on every run and for every order of the stations.
// The host side is the LDS sizing and one call of sc_pf_chunks (sc_profile.hip), to which it hands its own grid and
// workgroup shape and its own cap on the chunk.
#include "sc_fit.h"
#include <math.h>
#include <algorithm>

#define LT_MAX_WAVES 4                   // stations in flight per workgroup, where their LDS fits
#define LT_LDS_BYTES (160 * 1024)        // the LDS of a CU
#define LT_MAX_GRID 4096
#define LT_CURVE_DOUBLES (1ll << 25)     // stations per launch: PF_CHUNK, and 256 MiB of curves where they are asked for

// doubles of a wave's LDS: u, v and the mse curve
__host__ __device__ __forceinline__ size_t lt_wave_doubles(int h, int D) {
    return (size_t)(2 * h + 1) + (size_t)(2 * (h + D) + 1) + (size_t)(2 * D + 1);
}

// one point of a fault-parallel profile: the mean of the valid samples at q = sgn q0, sgn (q0 + 1), .., sgn q1 in that
// order, NaN where none is valid (pf_point's sample with k = t and j = q)
__device__ __forceinline__ double lt_point(const double* __restrict__ z, int ny, int nx, double r, double c, double sa,
                                           double ca, int tt, int q0, int q1, int sgn) {
    const double t = (double)tt;
    const double tca = t * ca, tsa = t * sa;
    double acc = 0.0;
    int cnt = 0;
    for (int qq = q0; qq <= q1; ++qq) {
        const double q = (double)(sgn * qq);
        const double rr = r + (tca - q * sa), cc = c + (q * ca + tsa);
        double v;
        if (pf_sample(z, ny, nx, rr, cc, v)) {
            acc += v;
            ++cnt;
        }
    }
    return cnt ? acc / (double)cnt : __builtin_nan("");
}

// one lag: u over t = -h..h against vd, v moved by the lag (vd[jj] = v_{t + d}, jj = t + h); every sum a plain loop over
// ascending t in one lane
struct lt_lag { bool fitted; int n; double mse, rho, dz, tilt; };

__device__ __forceinline__ lt_lag lt_fit_lag(const double* u, const double* vd, int np, int h, double de, int min_samples) {
    const double nan = __builtin_nan("");
    lt_lag f = {false, 0, nan, nan, nan, nan};
    // pass 0
    int n = 0;
    double Ss = 0.0, Su = 0.0, Sv = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double a = u[jj], b = vd[jj];
        if (a != a || b != b) continue;
        ++n;
        Ss += (double)(jj - h) * de;
        Su += a;
        Sv += b;
    }
    f.n = n;
    if (n < min_samples) return f;
    const double dn = (double)n;
    const double sbar = Ss / dn, ubar = Su / dn, vbar = Sv / dn;
    // pass 1
    double Stt = 0.0, Stu = 0.0, Stv = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double a = u[jj], b = vd[jj];
        if (a != a || b != b) continue;
        const double sc = (double)(jj - h) * de - sbar;
        Stt += sc * sc;
        Stu += sc * (a - ubar);
        Stv += sc * (b - vbar);
    }
    if (!(Stt > 0.0)) return f;
    const double bu = Stu / Stt, bv = Stv / Stt;
    // pass 2: the explicit residuals
    double Suu = 0.0, Svv = 0.0, Suv = 0.0, sse = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double a = u[jj], b = vd[jj];
        if (a != a || b != b) continue;
        const double sc = (double)(jj - h) * de - sbar;
        const double ru = (a - ubar) - bu * sc;
        const double rv = (b - vbar) - bv * sc;
        const double dr = rv - ru;
        Suu += ru * ru;
        Svv += rv * rv;
        Suv += ru * rv;
        sse += dr * dr;
    }
    f.fitted = true;
    f.mse = sse / (double)(n - 2);
    const double den = Suu * Svv;
    f.rho = den > 0.0 ? Suv / sqrt(den) : nan;
    f.dz = vbar - ubar;
    f.tilt = bv - bu;
    return f;
}

__global__ __launch_bounds__(64 * LT_MAX_WAVES) void k_lt_fit(const double* __restrict__ z, int ny, int nx,
                                                              const long long* __restrict__ cells,
                                                              const double* __restrict__ dir, long long K, int h, int q0,
                                                              int q1, int D, double de, double delta, int min_samples,
                                                              sc_lateral_fit* __restrict__ rows,
                                                              double* __restrict__ curve) {
    extern __shared__ double lt_lds_mem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    const int np = 2 * h + 1, nv = 2 * (h + D) + 1, nl = 2 * D + 1;
    double* u = lt_lds_mem + (size_t)wave * lt_wave_doubles(h, D);
    double* v = u + np;
    double* mc = v + nv;                                 // mse_d at d + D
    const double nan = __builtin_nan("");
    const long long rounds = (K + waves - 1) / waves;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {
        const long long kc = g * waves + wave;
        if (kc >= K) continue;                           // (per wave: no workgroup barrier in this kernel)
        const long long cell = cells[kc];
        const double sa = dir[2 * kc], ca = dir[2 * kc + 1];
        const double r = (double)(cell / nx), c = (double)(cell % nx);
        // stage 1
        for (int jj = lane; jj < np; jj += 64) u[jj] = lt_point(z, ny, nx, r, c, sa, ca, jj - h, q0, q1, -1);
        for (int jj = lane; jj < nv; jj += 64) v[jj] = lt_point(z, ny, nx, r, c, sa, ca, jj - (h + D), q0, q1, +1);
        wave_sync();
        // stage 2
        double bm = INFINITY, brho = nan, bdz = nan, btilt = nan;
        int br = INT_MAX, bn = 0;
        bool skipped = false;
        for (int r0 = 0; r0 < nl; r0 += 64) {
            const bool on = r0 + lane < nl;
            const int rk = on ? r0 + lane : nl - 1;      // lanes beyond the lags repeat the last one and are ignored
            const int d = sh_shift_of(rk);
            const lt_lag f = lt_fit_lag(u, v + (d + D), np, h, de, min_samples);
            if (on) {
                mc[d + D] = f.mse;
                if (curve) curve[(size_t)kc * nl + (d + D)] = f.mse;
                skipped = skipped || !f.fitted;
                if (f.fitted && f.mse == f.mse && (br == INT_MAX || f.mse < bm)) {
                    bm = f.mse;
                    br = rk;
                    bn = f.n;
                    brho = f.rho;
                    bdz = f.dz;
                    btilt = f.tilt;
                }
            }
        }
        double m = bm;
        int mr = br;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double om = __shfl_xor(m, o, 64);
            const int orr = __shfl_xor(mr, o, 64);
            if (om < m || (om == m && orr < mr)) { m = om; mr = orr; }
        }
        const bool any_skipped = __ballot(skipped) != 0ull;
        wave_sync();                                     // (the curve is whole)
        sc_lateral_fit* out = rows + kc;                 // (the rows were cleared: their padding is compared too)
        if (mr == INT_MAX) {
            if (lane == 0) {
                out->cell = cell;
                out->n = 0; out->lag = 0; out->lo = 0; out->hi = 0;
                out->status = 1;
                out->offset = nan; out->offset_lo = nan; out->offset_hi = nan;
                out->mse = nan; out->rho = nan; out->dz = nan; out->tilt = nan;
            }
        } else {
            const int wl = mr & 63;                      // the winner's lane
            const int n = __shfl(bn, wl, 64);
            const double rho = __shfl(brho, wl, 64), dz = __shfl(bdz, wl, 64), tilt = __shfl(btilt, wl, 64);
            const int lag = sh_shift_of(mr);
            const double thr = m * (1.0 + delta / (double)(n - 2));
            int lo = lag, hi = lag;
            while (lo > -D && mc[lo - 1 + D] <= thr) --lo;               // (a NaN stops the walk)
            while (hi < D && mc[hi + 1 + D] <= thr) ++hi;
            double frac = 0.0;
            if (lag > -D && lag < D) {
                const double mm = mc[lag - 1 + D], mp = mc[lag + 1 + D];
                const double den = (mm - m) + (mp - m);
                if (isfinite(mm) && isfinite(mp) && den > 0.0) frac = 0.5 * (mm - mp) / den;
            }
            if (lane == 0) {
                out->cell = cell;
                out->n = n; out->lag = lag; out->lo = lo; out->hi = hi;
                out->status = (lo == -D ? 2 : 0) + (hi == D ? 4 : 0) + (D > 0 && (lag == D || lag == -D) ? 8 : 0) +
                              (any_skipped ? 16 : 0);
                out->offset = ((double)lag + frac) * de;
                out->offset_lo = (double)lo * de;
                out->offset_hi = (double)hi * de;
                out->mse = m; out->rho = rho; out->dz = dz; out->tilt = tilt;
            }
        }
        wave_sync();                                     // (the next station overwrites what these lanes read)
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int lt_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                    const double* ca, long long K, int h, int q0, int q1, int D, double de, double delta, int min_samples,
                    const void* out_rows) {
    if (K < 0 || (K > 0 && (!cells || !sa || !ca || !out_rows))) return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (ny < 2 || nx < 2) return sc_fail(ctx, SC_ERR_INVALID, "%s: the grid must be at least 2 x 2", who);
    if (h < 1 || q0 < 1 || q1 < q0 || D < 0) return sc_fail(ctx, SC_ERR_INVALID, "%s: needs h >= 1, 1 <= q0 <= q1, D >= 0", who);
    if (h > SC_PROFILE_MAX_HALF) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: half-length %d cells, more than %d", who, h, SC_PROFILE_MAX_HALF);
    if (q1 > SC_LATERAL_MAX_FAR) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a band out to %d cells, more than %d", who, q1, SC_LATERAL_MAX_FAR);
    if (q1 - q0 + 1 > SC_LATERAL_MAX_BAND) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a band of %d lines, more than %d", who, q1 - q0 + 1, SC_LATERAL_MAX_BAND);
    if (D > SC_LATERAL_MAX_LAG) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: a lag of %d cells, more than %d", who, D, SC_LATERAL_MAX_LAG);
    if (K > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: %lld cells, more than 2^31 - 1", who, K);
    if (min_samples < 3 || min_samples > 2 * h + 1)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: min_samples must lie in 3..2 h + 1", who);
    if (!(isfinite(delta) && delta >= 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: delta must be finite and >= 0", who);
    if (!(isfinite(de) && de > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: the cell size must be finite and > 0", who);
    const long long nc = ny * nx;
    for (long long k = 0; k < K; ++k) {
        if (cells[k] < 0 || cells[k] >= nc) return sc_fail(ctx, SC_ERR_INVALID, "%s: cell %lld outside the grid", who, cells[k]);
        if (!(isfinite(sa[k]) && isfinite(ca[k]))) return sc_fail(ctx, SC_ERR_INVALID, "%s: sa / ca not finite at cell %lld", who, k);
    }
    return SC_OK;
}

// (the call's buffers are sc_fit_profiles': the two are never in flight together on one context)
static int lt_run(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa, const double* ca,
                  long long K, int h, int q0, int q1, int D, double de, double delta, int min_samples,
                  sc_lateral_fit* out_rows, double* out_mse) {
    if (K == 0) return SC_OK;
    const int nl = 2 * D + 1;
    long long chunk = PF_CHUNK;
    if (out_mse) chunk = std::min<long long>(chunk, std::max<long long>(1, LT_CURVE_DOUBLES / nl));

    // as many waves a workgroup as their LDS allows (the limits of lt_check leave room for LT_MAX_WAVES)
    const size_t wave_bytes = sizeof(double) * lt_wave_doubles(h, D);
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(LT_MAX_WAVES, LT_LDS_BYTES / wave_bytes));
    const size_t lds = wave_bytes * (size_t)waves;
    if (lds > LT_LDS_BYTES) return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_lateral_offsets: %zu bytes of LDS a station", wave_bytes);
    int rc;
    if ((rc = sc_lds_attr(ctx, (const void*)k_lt_fit, lds))) return rc;

    const pf_plane curve = {out_mse, &ctx->pf_sse, sizeof(double) * (size_t)nl}, none = {nullptr, nullptr, 0};
    return sc_pf_chunks(ctx, cells, sa, ca, K, chunk, sizeof(sc_lateral_fit), out_rows, curve, none,
                        [&](const pf_chunk& d, long long m) {
        const unsigned grid = (unsigned)std::min<long long>((m + waves - 1) / waves, LT_MAX_GRID);
        k_lt_fit<<<grid, 64 * waves, lds, ctx->stream>>>(z, ny, nx, d.cells, d.dir, m, h, q0, q1, D, de, delta, min_samples,
                                                        (sc_lateral_fit*)d.rows, (double*)d.plane[0]);
    });
}

// the two calls after their null checks: the argument checks, then the search on z - ny x nx on the host, uploaded - or
// on the context's DEM (z null)
static int lt_call(sc_ctx* ctx, const char* who, const double* z, int ny, int nx, const long long* cells, const double* sa,
                   const double* ca, long long K, int h, int q0, int q1, int D, double de, double delta, int min_samples,
                   sc_lateral_fit* out_rows, double* out_mse) {
    int rc = lt_check(ctx, who, ny, nx, cells, sa, ca, K, h, q0, q1, D, de, delta, min_samples, out_rows);
    if (rc) return rc;
    if (z && K == 0) return SC_OK;
    const double* z_dev;
    if ((rc = sc_pf_dem(ctx, ctx->pf_z, z, ny, nx, &z_dev))) return rc;
    return lt_run(ctx, z_dev, ny, nx, cells, sa, ca, K, h, q0, q1, D, de, delta, min_samples, out_rows, out_mse);
}

extern "C" int sc_lateral_offsets(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K, int h,
                                  int q0, int q1, int D, double de, double delta, int min_samples, sc_lateral_fit* out_rows,
                                  double* out_mse) {
    if (!ctx) return SC_ERR_INVALID;
    int rc = sc_pf_whole_grid(ctx, "sc_lateral_offsets");
    if (rc) return rc;
    return lt_call(ctx, "sc_lateral_offsets", nullptr, ctx->g.ny, ctx->g.nx, cells, sa, ca, K, h, q0, q1, D, de, delta,
                   min_samples, out_rows, out_mse);
}

extern "C" int sc_lateral_offsets_dem(sc_ctx* ctx, const double* z, int ny, int nx, const long long* cells, const double* sa,
                                      const double* ca, long long K, int h, int q0, int q1, int D, double de, double delta,
                                      int min_samples, sc_lateral_fit* out_rows, double* out_mse) {
    if (!ctx || !z) return SC_ERR_INVALID;
    return lt_call(ctx, "sc_lateral_offsets_dem", z, ny, nx, cells, sa, ca, K, h, q0, q1, D, de, delta, min_samples, out_rows,
                   out_mse);
}
