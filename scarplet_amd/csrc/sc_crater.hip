// sc_crater_windows: the reference's Crater template (WindowedTemplate.py:528-605) synthesised on the device, straight
// into window slots (docs/craters.md).
//
// Crater.template() is a sum of 359 thin strips tangent to a ring of radius R: for theta_k in ascending order a Scarp
// profile across the strip, kept where |xr| < 1 and |yr| < 5 / de, negated on the left half of the ring.  Every
// transcendental that decides one of the two compares - cos and sin of alpha = -theta, dx = R cos(theta),
// dy = R sin(theta), the two age terms, 5 / de - comes from the host, evaluated with numpy as the reference evaluates
// it; xr and yr are then formed from them by correctly rounded float64 operations in the reference's order, so the
// support W != 0 is the reference's cell for cell.  The one device transcendental is the exp, taken under the mask.
//   k_crater_window  grid (ceil(largest box / 256), templates), one thread per cell of the template's support box:
//                    the strips summed in ascending theta; writes the float64 window, its float32 copy and the
//                    W != 0 bytes - the three things sc_upload_window keeps for a slot
//   k_crater_sums    one workgroup per template: count(W != 0), sum(W * W) and sum |W| in float64, each thread over
//                    the cells tid, tid + 256, ... in ascending order, then a fixed tree in LDS
// No atomics: the same bytes on every run.  All windows of a call live in ONE allocation (tables, sums, the three
// planes), freed by sc_clear_windows: a 20 x 35 search is one hipMalloc, one upload of the tables and two launches.
#include "sc_internal.h"
#include <math.h>
#include <algorithm>
#include <vector>

#define CR_THREADS 256
#define CR_MAX_THETA 4096
#define CR_MAX_TEMPLATES 65535            // gridDim.y of k_crater_window

struct CrTempl {
    long long off;             // element offset of the window in the three planes (a multiple of 4)
    int32_t h, wd;             // the support box
    int32_t pmin, qmin;        // its first row / column, as offsets from (ny // 2, nx // 2)
    int32_t ir, ia;            // radius and age of the template
};

__global__ __launch_bounds__(CR_THREADS) void
k_crater_window(const CrTempl* __restrict__ tt, const double* __restrict__ th, const double* __restrict__ dxy,
                const double* __restrict__ ring, const double* __restrict__ atab, double d_half, int n_theta,
                const double* __restrict__ xaxis, const double* __restrict__ yaxis, int cy, int cx,
                double* __restrict__ w64, float* __restrict__ w32, uint8_t* __restrict__ wm) {
    const CrTempl t = tt[blockIdx.y];
    const int cell = blockIdx.x * CR_THREADS + threadIdx.x;
    if (cell >= t.h * t.wd) return;
    const int row = cell / t.wd, col = cell - row * t.wd;
    const double x = xaxis[cx + t.qmin + col], y = yaxis[cy + t.pmin + row];
    double W = 0.0;
    // every cell some strip keeps has (R - 1)^2 < x^2 + y^2 < (R + 1)^2 + (5 / de)^2 (xr = u - R, yr = v with (u, v) the
    // cell rotated by theta); the host widens the two bounds by 1e-9 of themselves, far beyond the rounding of rho2
    const double rho2 = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
    if (rho2 >= ring[2 * t.ir] && rho2 <= ring[2 * t.ir + 1]) {
        const double p0 = atab[2 * t.ia], p1 = atab[2 * t.ia + 1];
        const double* __restrict__ d = dxy + 2 * (size_t)n_theta * t.ir;
        for (int k = 0; k < n_theta; ++k) {
            const double ca = th[3 * k], sa = th[3 * k + 1];
            const double xm = __dsub_rn(x, d[2 * k]), yp = __dadd_rn(y, d[2 * k + 1]);
            const double xr = __dadd_rn(__dmul_rn(xm, ca), __dmul_rn(yp, sa));
            if (!(fabs(xr) < 1.0)) continue;                 // (a strip outside its mask adds +-0)
            const double yr = __dadd_rn(__dmul_rn(-xm, sa), __dmul_rn(yp, ca));
            if (!(fabs(yr) < d_half)) continue;
            const double v = __dmul_rn(__ddiv_rn(-xr, p0), exp(__ddiv_rn(-__dmul_rn(xr, xr), p1)));
            W = __dadd_rn(W, __dmul_rn(v, th[3 * k + 2]));   // the sign: -1 where pi/2 < theta < 3 pi/2
        }
    }
    const size_t o = (size_t)t.off + cell;
    w64[o] = W;
    w32[o] = (float)W;
    wm[o] = W != 0.0 ? 1 : 0;
}

__global__ __launch_bounds__(CR_THREADS) void
k_crater_sums(const CrTempl* __restrict__ tt, const double* __restrict__ w64, double* __restrict__ out) {
    __shared__ double s_n[CR_THREADS], s_2[CR_THREADS], s_1[CR_THREADS];
    const CrTempl t = tt[blockIdx.x];
    const int tid = threadIdx.x, cells = t.h * t.wd;
    const double* __restrict__ w = w64 + t.off;
    double n = 0.0, s2 = 0.0, s1 = 0.0;
    for (int i = tid; i < cells; i += CR_THREADS) {
        const double v = w[i];
        if (v != 0.0) {
            n = __dadd_rn(n, 1.0);
            s2 = __dadd_rn(s2, __dmul_rn(v, v));
            s1 = __dadd_rn(s1, fabs(v));
        }
    }
    s_n[tid] = n; s_2[tid] = s2; s_1[tid] = s1;
    __syncthreads();
    for (int s = CR_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            s_n[tid] = __dadd_rn(s_n[tid], s_n[tid + s]);
            s_2[tid] = __dadd_rn(s_2[tid], s_2[tid + s]);
            s_1[tid] = __dadd_rn(s_1[tid], s_1[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[3 * (size_t)blockIdx.x] = s_n[0];
        out[3 * (size_t)blockIdx.x + 1] = s_2[0];
        out[3 * (size_t)blockIdx.x + 2] = s_1[0];
    }
}

static bool cr_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

extern "C" int sc_crater_windows(sc_ctx* ctx, int n_radii, int n_ages, int n_theta, const double* theta_tab,
                                 const double* dxy, const double* ring, const double* age_tab, double d_half,
                                 const int32_t* boxes, int* slots, double* count, double* sumsq, double* w_out) {
    if (!ctx) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "sc_crater_windows: no DEM set (the windows are made on its axes)");
    if (n_radii < 1 || n_ages < 1 || n_theta < 1 || !theta_tab || !dxy || !ring || !age_tab || !boxes || !slots ||
        !count || !sumsq)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_crater_windows: bad argument");
    if (n_theta > CR_MAX_THETA || (long long)n_radii * n_ages > CR_MAX_TEMPLATES)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_crater_windows: more than %d strips or %d templates", CR_MAX_THETA,
                       CR_MAX_TEMPLATES);
    if (!(d_half > 0.0) || !isfinite(d_half) || !cr_finite(theta_tab, 3 * (size_t)n_theta) ||
        !cr_finite(dxy, 2 * (size_t)n_radii * n_theta) || !cr_finite(ring, 2 * (size_t)n_radii) ||
        !cr_finite(age_tab, 2 * (size_t)n_ages))
        return sc_fail(ctx, SC_ERR_INVALID, "sc_crater_windows: a table entry is not finite");
    for (int a = 0; a < n_ages; ++a)
        if (!(age_tab[2 * a] > 0.0) || !(age_tab[2 * a + 1] > 0.0))
            return sc_fail(ctx, SC_ERR_INVALID, "sc_crater_windows: age %d is not positive", a);
    const Geom& g = ctx->g;
    const int cy = g.ny / 2, cx = g.nx / 2;
    const int n = n_radii * n_ages;
    std::vector<CrTempl> tt(n);
    size_t total = 0, max_cells = 0;
    for (int r = 0; r < n_radii; ++r) {
        const int32_t* b = boxes + 4 * r;               // pmin, pmax, qmin, qmax
        if (b[1] < b[0] || b[3] < b[2] || cy + b[0] < 0 || cy + b[1] >= g.ny || cx + b[2] < 0 || cx + b[3] >= g.nx)
            return sc_fail(ctx, SC_ERR_INVALID, "sc_crater_windows: the support box of radius %d (rows %d..%d, columns "
                           "%d..%d about the centre) leaves the %d x %d grid", r, b[0], b[1], b[2], b[3], g.ny, g.nx);
        const size_t cells = (size_t)(b[1] - b[0] + 1) * (b[3] - b[2] + 1);
        max_cells = std::max(max_cells, cells);
        for (int a = 0; a < n_ages; ++a) {
            CrTempl& t = tt[(size_t)r * n_ages + a];
            t.off = (long long)total;
            t.h = b[1] - b[0] + 1; t.wd = b[3] - b[2] + 1;
            t.pmin = b[0]; t.qmin = b[2];
            t.ir = r; t.ia = a;
            total += (cells + 3) & ~(size_t)3;
        }
    }
    if (total > (size_t)INT_MAX)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_crater_windows: %zu window cells in one call", total);
    SC_HIP(ctx, hipSetDevice(ctx->device));

    // one allocation: [tables (doubles)] [sums 3 n] [w64] [template table] [w32] [bytes]
    const size_t n_th = 3 * (size_t)n_theta, n_dxy = 2 * (size_t)n_radii * n_theta, n_ring = 2 * (size_t)n_radii,
                 n_age = 2 * (size_t)n_ages;
    const size_t n_tab = n_th + n_dxy + n_ring + n_age;
    const size_t o_sums = n_tab * sizeof(double), o_w64 = o_sums + 3 * (size_t)n * sizeof(double),
                 o_tt = o_w64 + total * sizeof(double), o_w32 = o_tt + (size_t)n * sizeof(CrTempl),
                 o_m = o_w32 + total * sizeof(float), bytes = o_m + total;
    static_assert(sizeof(CrTempl) % 8 == 0, "the template table sits between the float64 and the float32 planes");
    std::vector<double> tab(n_tab);
    std::copy(theta_tab, theta_tab + n_th, tab.begin());
    std::copy(dxy, dxy + n_dxy, tab.begin() + n_th);
    std::copy(ring, ring + n_ring, tab.begin() + n_th + n_dxy);
    std::copy(age_tab, age_tab + n_age, tab.begin() + n_th + n_dxy + n_ring);
    char* pool = nullptr;
    SC_HIP(ctx, hipMalloc((void**)&pool, bytes));
    ctx->window_pools.push_back(pool);                  // (sc_clear_windows frees it, whatever way this call ends)
    double* d_tab = (double*)pool;
    double* d_sums = (double*)(pool + o_sums);
    double* d_w64 = (double*)(pool + o_w64);
    CrTempl* d_tt = (CrTempl*)(pool + o_tt);
    float* d_w32 = (float*)(pool + o_w32);
    uint8_t* d_m = (uint8_t*)(pool + o_m);
    // (the padding between windows is never read; zeroed all the same so that the pool holds no stale bytes)
    SC_HIP(ctx, hipMemsetAsync(pool + o_w64, 0, bytes - o_w64, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), n_tab * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(d_tt, tt.data(), (size_t)n * sizeof(CrTempl), hipMemcpyHostToDevice, ctx->stream));

    sc_prof_begin(ctx, SC_K_WINDOWS);
    const dim3 grid((unsigned)((max_cells + CR_THREADS - 1) / CR_THREADS), (unsigned)n);
    hipLaunchKernelGGL(k_crater_window, grid, dim3(CR_THREADS), 0, ctx->stream, d_tt, d_tab, d_tab + n_th,
                       d_tab + n_th + n_dxy, d_tab + n_th + n_dxy + n_ring, d_half, n_theta,
                       (const double*)ctx->xaxis.p, (const double*)ctx->yaxis.p, cy, cx, d_w64, d_w32, d_m);
    hipLaunchKernelGGL(k_crater_sums, dim3((unsigned)n), dim3(CR_THREADS), 0, ctx->stream, d_tt, d_w64, d_sums);
    sc_prof_end(ctx, 2);
    SC_HIP(ctx, hipGetLastError());
    std::vector<double> sums(3 * (size_t)n);
    SC_HIP(ctx, hipMemcpyAsync(sums.data(), d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sc_prof_collect(ctx);

    size_t out_off = 0;
    for (int k = 0; k < n; ++k) {
        const CrTempl& t = tt[k];
        WindowSlot s;
        s.pooled = true;
        s.l1 = sums[3 * (size_t)k + 2];
        s.h = t.h; s.wd = t.wd;
        s.w = d_w32 + t.off;
        s.w64 = d_w64 + t.off;
        s.m = d_m + t.off;
        ctx->windows.push_back(s);
        slots[k] = (int)ctx->windows.size() - 1;
        count[k] = sums[3 * (size_t)k];
        sumsq[k] = sums[3 * (size_t)k + 1];
        if (w_out) {
            const size_t cells = (size_t)t.h * t.wd;
            SC_HIP(ctx, hipMemcpy(w_out + out_off, s.w64, cells * sizeof(double), hipMemcpyDeviceToHost));
            out_off += cells;
        }
    }
    return SC_OK;
}
