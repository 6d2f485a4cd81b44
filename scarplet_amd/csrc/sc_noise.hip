// sc_curvature_noise: the moments behind CalculationMixin._estimate_curvature_noiselevel (dem.py:152-179).
//
// The reference filters the directional curvature of 180 orientations with gaussian_filter(del2z, sigma) (mode
// 'reflect') and takes nanmean / nanstd of the high-pass del2z - lowpass.  Curvature and filter are linear:
// del2z(a) = c2 A - 2 s c B + s2 C over the three stencil planes, so highpass(a) = c2 H_A - 2 s c H_B + s2 H_C with
// H_P = P - G * P, and the mean and variance of every orientation follow from the mean and 3 x 3 covariance of
// (H_A, H_B, H_C).  The device computes those moments, the host evaluates the orientations (scarplet_amd/noise.py).
//
// Pipeline (all on the context's stream, one profiling bracket SC_K_NOISE):
//   k_noise_dilate (x2)   only with a NaN mask: the cells within Chebyshev distance r of a NaN cell, a separable
//                         dilation (rows, then columns) - the cells the reference's first orientation drops
//   k_noise_rows          the stencil planes (k_curv_planes' arithmetic, computed while staging) filtered along x:
//                         a row segment staged in LDS, NZ_R outputs per lane, float64 FMAs, weights as scalar operands
//   k_noise_cols          the same filter along y, read from L1 / L2, then h = P - lowpass and per-workgroup moments
//                         (n, mean[3], co-moments[6]) of both cell sets, merged with Chan's pairwise update
//   k_noise_merge         one workgroup merges the partials in a fixed order: the same bits on every run
//
// Boundary: scipy's 'reflect' (d c b a | a b c d | d c b a), periodic in 2n, so radii beyond the grid side hold too.
// The filter order (x first) differs from scipy's (axis 0 first): the results agree to rounding, not to the bit.
#include "sc_internal.h"
#include <vector>

namespace {

constexpr int NZ_R = 8;                                       // outputs per lane along the filter axis
constexpr int NZ_ROW_LANES = 256;
constexpr int NZ_ROW_W = NZ_ROW_LANES * NZ_R;                 // outputs of one row per workgroup of the row pass
constexpr int NZ_CH = 1024;                                   // taps staged per round (a multiple of NZ_R)
constexpr int NZ_LDS = (NZ_ROW_W + NZ_CH) / NZ_R * (NZ_R + 1); // doubles: one pad after every NZ_R (conflict-free reads)
constexpr int NZ_COL_WAVES = 4;
constexpr int NZ_COL_ROWS = NZ_COL_WAVES * NZ_R;              // a column-pass workgroup: 64 columns x 32 rows
constexpr int NZ_MERGE = 256;
constexpr int NZ_STAT = 10;                                   // n, mean[3], co-moments[6] (upper triangle, row-major)

struct NzStat {
    double n, m[3], c[6];
};

// scipy.ndimage mode 'reflect': half-sample symmetric, period 2n
__device__ __forceinline__ int nz_reflect(int m, int n) {
    const int p = 2 * n;
    m %= p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// stencil plane p (0 d2z/dx2, 1 d2z/dxdy, 2 d2z/dy2) at cell (i, j) of the whole ny x nx grid: k_curv_planes'
// arithmetic (dem.py:88-101, zero borders, dx in the cross term), bit for bit
__device__ __forceinline__ double nz_plane(const double* __restrict__ z, int ny, int nx, double dx, double dy,
                                           int p, int i, int j) {
    const double* r1 = z + (size_t)i * nx;
    const double z11 = r1[j];
    if (p == 0) {
        if (j < 1 || j > nx - 2) return 0.0;
        return __ddiv_rn(__dsub_rn(__dsub_rn(r1[j + 1], z11), __dsub_rn(z11, r1[j - 1])), __dmul_rn(dx, dx));
    }
    if (p == 1) {
        if (i < 1 || j < 1) return 0.0;
        const double* r0 = r1 - nx;
        const double d1 = __ddiv_rn(__dsub_rn(z11, r1[j - 1]), dx);
        const double d0 = __ddiv_rn(__dsub_rn(r0[j], r0[j - 1]), dx);
        return __ddiv_rn(__dsub_rn(d1, d0), dx);
    }
    if (i < 1 || i > ny - 2) return 0.0;
    return __ddiv_rn(__dsub_rn(__dsub_rn((r1 + nx)[j], z11), __dsub_rn(z11, (r1 - nx)[j])),
                     __dmul_rn(dy, dy));
}

// Chan et al.'s pairwise update: a <- a (+) b
__device__ __forceinline__ void nz_merge(NzStat& a, const NzStat& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) {
        a = b;
        return;
    }
    const double n = a.n + b.n;
    const double f = b.n / n;
    const double g = a.n * f;
    double d[3];
    for (int k = 0; k < 3; ++k) {
        d[k] = b.m[k] - a.m[k];
        a.m[k] = a.m[k] + d[k] * f;
    }
    int o = 0;
    for (int k = 0; k < 3; ++k)
        for (int l = k; l < 3; ++l, ++o) a.c[o] = (a.c[o] + b.c[o]) + (d[k] * d[l]) * g;
    a.n = n;
}

// moments of the cells ok[] of one lane (two passes over registers)
__device__ __forceinline__ NzStat nz_lane_stat(const double (&h)[3][NZ_R], const bool (&ok)[NZ_R]) {
    NzStat s{};
    double sum[3] = {0.0, 0.0, 0.0};
    int n = 0;
    for (int q = 0; q < NZ_R; ++q)
        if (ok[q]) {
            ++n;
            for (int p = 0; p < 3; ++p) sum[p] += h[p][q];
        }
    if (n == 0) return s;
    s.n = (double)n;
    for (int p = 0; p < 3; ++p) s.m[p] = sum[p] / s.n;
    for (int q = 0; q < NZ_R; ++q)
        if (ok[q]) {
            double d[3];
            for (int p = 0; p < 3; ++p) d[p] = h[p][q] - s.m[p];
            int o = 0;
            for (int k = 0; k < 3; ++k)
                for (int l = k; l < 3; ++l, ++o) s.c[o] += d[k] * d[l];
        }
    return s;
}

__device__ __forceinline__ NzStat nz_shfl_xor(const NzStat& s, int off) {
    NzStat t;
    t.n = __shfl_xor(s.n, off);
    for (int k = 0; k < 3; ++k) t.m[k] = __shfl_xor(s.m[k], off);
    for (int k = 0; k < 6; ++k) t.c[k] = __shfl_xor(s.c[k], off);
    return t;
}

__device__ __forceinline__ void nz_store(double* o, const NzStat& s) {
    o[0] = s.n;
    for (int k = 0; k < 3; ++k) o[1 + k] = s.m[k];
    for (int k = 0; k < 6; ++k) o[4 + k] = s.c[k];
}

__device__ __forceinline__ NzStat nz_load(const double* o) {
    NzStat s;
    s.n = o[0];
    for (int k = 0; k < 3; ++k) s.m[k] = o[1 + k];
    for (int k = 0; k < 6; ++k) s.c[k] = o[4 + k];
    return s;
}

// Chebyshev dilation along one axis: out[e] = some in[e'] with |e - e'| <= r.  One thread per line (a row or a
// column), a forward and a backward sweep.
__global__ void __launch_bounds__(256)
k_noise_dilate(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int lines, int len, long long ls,
               long long es, int r) {
    const int L = blockIdx.x * 256 + threadIdx.x;
    if (L >= lines) return;
    const uint8_t* a = in + L * ls;
    uint8_t* b = out + L * ls;
    long long last = -(1LL << 40);
#pragma unroll 8
    for (int e = 0; e < len; ++e) {
        if (a[e * es]) last = e;
        b[e * es] = (e - last <= r) ? 1 : 0;
    }
    long long next = 1LL << 40;
#pragma unroll 8
    for (int e = len - 1; e >= 0; --e) {
        if (a[e * es]) next = e;
        if (next - e <= r) b[e * es] = 1;
    }
}

// Filter along x.  Workgroup: one plane (blockIdx.y), one row, NZ_ROW_W outputs; lane l owns outputs
// j0 + l NZ_R + q.  Output q takes staged element t with weight wp[t - q + NZ_R - 1] (wp: the 2r+1 weights with
// NZ_R - 1 zeros in front and zeros behind), so one LDS read feeds NZ_R FMAs.  The taps are staged NZ_CH at a time.
__global__ void __launch_bounds__(NZ_ROW_LANES)
k_noise_rows(const double* __restrict__ z, int ny, int nx, double dx, double dy, const double* __restrict__ wp,
             int r, int T, int nseg, double* __restrict__ low) {
    __shared__ double s[NZ_LDS];
    const int p = blockIdx.y;
    const int row = blockIdx.x / nseg;
    const int j0 = (blockIdx.x % nseg) * NZ_ROW_W;
    const int l = threadIdx.x;
    double acc[NZ_R];
#pragma unroll
    for (int q = 0; q < NZ_R; ++q) acc[q] = 0.0;
    const double* sl = s + l * (NZ_R + 1);
    for (int t0 = 0; t0 < T; t0 += NZ_CH) {
        const int ch = min(NZ_CH, T - t0);
        const int ne = NZ_ROW_W + ch;
        const int c0 = j0 - r + t0;                       // column of staged element 0
        __syncthreads();
        if (c0 >= 0 && c0 + ne <= nx) {
            for (int e = l; e < ne; e += NZ_ROW_LANES) s[e + e / NZ_R] = nz_plane(z, ny, nx, dx, dy, p, row, c0 + e);
        } else {
            for (int e = l; e < ne; e += NZ_ROW_LANES)
                s[e + e / NZ_R] = nz_plane(z, ny, nx, dx, dy, p, row, nz_reflect(c0 + e, nx));
        }
        __syncthreads();
        for (int tb = 0; tb < ch; tb += NZ_R) {
            const double* w = wp + t0 + tb + (NZ_R - 1);
            const double* src = sl + tb + tb / NZ_R;
            double v[NZ_R];
#pragma unroll
            for (int u = 0; u < NZ_R; ++u) v[u] = src[u];
#pragma unroll
            for (int u = 0; u < NZ_R; ++u)
#pragma unroll
                for (int q = 0; q < NZ_R; ++q) acc[q] = __fma_rn(w[u - q], v[u], acc[q]);
        }
    }
    const int jb = j0 + l * NZ_R;
    double* o = low + (size_t)p * ny * nx + (size_t)row * nx;
#pragma unroll
    for (int q = 0; q < NZ_R; ++q)
        if (jb + q < nx) o[jb + q] = acc[q];
}

// the column pass's taps: rows top + t, t < T, of the three x-filtered planes at column j
template <bool INNER>
__device__ __forceinline__ void nz_cols_taps(const double* __restrict__ low, size_t plane, int ny, int nx, int j,
                                             const double* __restrict__ wp, int top, int T, double (&acc)[3][NZ_R]) {
    for (int tb = 0; tb < T; tb += NZ_R) {
        const double* w = wp + tb + (NZ_R - 1);
        double v[3][NZ_R];
#pragma unroll
        for (int u = 0; u < NZ_R; ++u) {
            const int i = INNER ? top + tb + u : nz_reflect(top + tb + u, ny);
            const double* src = low + (size_t)i * nx + j;
            v[0][u] = src[0];
            v[1][u] = src[plane];
            v[2][u] = src[2 * plane];
        }
#pragma unroll
        for (int u = 0; u < NZ_R; ++u)
#pragma unroll
            for (int q = 0; q < NZ_R; ++q)
#pragma unroll
                for (int p = 0; p < 3; ++p) acc[p][q] = __fma_rn(w[u - q], v[p][u], acc[p][q]);
    }
}

// Filter along y, high-pass, moments.  Workgroup: 64 columns x NZ_COL_ROWS rows, each wave NZ_R rows (its waves read
// overlapping rows: L1 hits).  part[blockIdx.x]: the two cell sets' NzStat (the second only with a box).
__global__ void __launch_bounds__(NZ_COL_WAVES * 64)
k_noise_cols(const double* __restrict__ z, int ny, int nx, double dx, double dy, const double* __restrict__ wp,
             int r, int T, const double* __restrict__ low, const uint8_t* __restrict__ box, int ncb,
             double* __restrict__ part) {
    __shared__ double red[NZ_COL_WAVES][2 * NZ_STAT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = (blockIdx.x % ncb) * 64 + lane;
    const int jl = min(j, nx - 1);                        // (columns past the grid: loads kept inside, cells not counted)
    const int i0 = (blockIdx.x / ncb) * NZ_COL_ROWS + wv * NZ_R;
    const size_t plane = (size_t)ny * nx;
    double acc[3][NZ_R];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < NZ_R; ++q) acc[p][q] = 0.0;
    const int top = i0 - r;                               // input row of tap 0 of output row i0
    if (top >= 0 && top + T <= ny)
        nz_cols_taps<true>(low, plane, ny, nx, jl, wp, top, T, acc);
    else
        nz_cols_taps<false>(low, plane, ny, nx, jl, wp, top, T, acc);
    bool ok[NZ_R], ok2[NZ_R];
#pragma unroll
    for (int q = 0; q < NZ_R; ++q) {
        const int i = i0 + q;
        ok[q] = i < ny && j < nx;
        ok2[q] = ok[q] && !(box && box[(size_t)i * nx + j]);
        const int ic = min(i, ny - 1);
#pragma unroll
        for (int p = 0; p < 3; ++p) acc[p][q] = nz_plane(z, ny, nx, dx, dy, p, ic, jl) - acc[p][q];   // h = P - lowpass
    }
    NzStat st[2] = {nz_lane_stat(acc, ok), NzStat{}};
    if (box) st[1] = nz_lane_stat(acc, ok2);
    // the wave's 64 lanes, a fixed butterfly: the lower lane's statistics always go first
    for (int off = 1; off < 64; off <<= 1) {
        const bool hi = (lane & off) != 0;
        for (int k = 0; k < 2; ++k) {
            NzStat o = nz_shfl_xor(st[k], off);
            if (hi) {
                nz_merge(o, st[k]);
                st[k] = o;
            } else {
                nz_merge(st[k], o);
            }
        }
    }
    if (lane == 0) {
        nz_store(red[wv], st[0]);
        nz_store(red[wv] + NZ_STAT, st[1]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 2; ++k) {
            NzStat a = nz_load(red[0] + k * NZ_STAT);
            for (int w = 1; w < NZ_COL_WAVES; ++w) nz_merge(a, nz_load(red[w] + k * NZ_STAT));
            nz_store(part + (size_t)blockIdx.x * 2 * NZ_STAT + k * NZ_STAT, a);
        }
    }
}

// all partials, fixed order: thread t merges partials t, t + 256, ..., then a tree over the threads.  sets = 1: the
// second set is the first (no NaN mask).
__global__ void __launch_bounds__(NZ_MERGE)
k_noise_merge(const double* __restrict__ part, int nparts, int sets, double* __restrict__ out) {
    __shared__ double s[NZ_MERGE][NZ_STAT];
    const int t = threadIdx.x;
    for (int k = 0; k < sets; ++k) {
        NzStat a{};
        for (int i = t; i < nparts; i += NZ_MERGE) nz_merge(a, nz_load(part + (size_t)i * 2 * NZ_STAT + k * NZ_STAT));
        nz_store(s[t], a);
        __syncthreads();
        for (int st = NZ_MERGE / 2; st > 0; st >>= 1) {
            if (t < st) {
                NzStat b = nz_load(s[t]);
                nz_merge(b, nz_load(s[t + st]));
                nz_store(s[t], b);
            }
            __syncthreads();
        }
        if (t == 0) {
            NzStat b = nz_load(s[0]);
            nz_store(out + k * NZ_STAT, b);
            if (sets == 1) nz_store(out + NZ_STAT, b);
        }
        __syncthreads();
    }
}

struct NzBufs {
    sc_ctx* ctx;
    DevBuf b[3];
    ~NzBufs() {                       // the filtered planes are 24 bytes a cell: not kept between calls
        for (DevBuf& d : b)
            if (d.p) (void)hipFree(d.p);
    }
};

}  // namespace

extern "C" int sc_curvature_noise(sc_ctx* ctx, const double* weights, int radius, const uint8_t* nan_mask,
                                  double* out) {
    if (!ctx || !weights || !out || radius < 0) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const Geom g = ctx->g;
    if (g.ly != g.ny || g.lx != g.nx || g.gy0 != 0 || g.gx0 != 0)
        return sc_fail(ctx, SC_ERR_INVALID, "sc_curvature_noise: the context holds a block of the DEM, not the whole grid");
    if (radius > SC_NOISE_MAX_RADIUS)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_curvature_noise: radius %d > %d", radius, SC_NOISE_MAX_RADIUS);
    const int ny = g.ny, nx = g.nx;
    const size_t nc = (size_t)ny * nx;
    const int T = (2 * radius + NZ_R + NZ_R - 1) / NZ_R * NZ_R;      // taps per output, rounded up to NZ_R
    const long long nseg = (nx + NZ_ROW_W - 1) / NZ_ROW_W;
    const long long ncb = (nx + 63) / 64;
    const long long nparts = ncb * ((ny + NZ_COL_ROWS - 1) / NZ_COL_ROWS);
    if (nseg * ny > INT_MAX || nparts > INT_MAX)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_curvature_noise: grid of %d x %d too large", ny, nx);
    SC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> wp((size_t)T + NZ_R, 0.0);
    for (int k = 0; k <= 2 * radius; ++k) wp[(size_t)k + NZ_R - 1] = weights[k];

    NzBufs nb{ctx, {}};
    const size_t wbytes = (wp.size() * sizeof(double) + 255) & ~(size_t)255;
    const size_t pbytes = (size_t)nparts * 2 * NZ_STAT * sizeof(double);
    int rc = sc_ensure(ctx, nb.b[0], wbytes + pbytes + 2 * NZ_STAT * sizeof(double));
    if (rc) return rc;
    if ((rc = sc_ensure(ctx, nb.b[1], 3 * nc * sizeof(double)))) return rc;
    double* d_w = (double*)nb.b[0].p;
    double* d_part = (double*)((char*)nb.b[0].p + wbytes);
    double* d_out = d_part + (size_t)nparts * 2 * NZ_STAT;
    double* d_low = (double*)nb.b[1].p;
    uint8_t* d_box = nullptr;

    sc_prof_begin(ctx, SC_K_NOISE);               // (one bracket over the whole call: every return below closes it)
    struct ProfEnd { sc_ctx* c; ~ProfEnd() { sc_prof_end(c); } } prof_end{ctx};
    SC_HIP(ctx, hipMemcpyAsync(d_w, wp.data(), wp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (nan_mask) {
        if ((rc = sc_ensure(ctx, nb.b[2], 3 * nc))) return rc;
        uint8_t* d_mask = (uint8_t*)nb.b[2].p;
        uint8_t* d_rows = d_mask + nc;
        d_box = d_mask + 2 * nc;
        SC_HIP(ctx, hipMemcpyAsync(d_mask, nan_mask, nc, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_noise_dilate, dim3((ny + 255) / 256), dim3(256), 0, ctx->stream,
                           (const uint8_t*)d_mask, d_rows, ny, nx, (long long)nx, 1LL, radius);
        SC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_noise_dilate, dim3((nx + 255) / 256), dim3(256), 0, ctx->stream,
                           (const uint8_t*)d_rows, d_box, nx, ny, 1LL, (long long)nx, radius);
        SC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_noise_rows, dim3((unsigned)(nseg * ny), 3), dim3(NZ_ROW_LANES), 0, ctx->stream,
                       ctx->z_dev, ny, nx, ctx->dx, ctx->dy, (const double*)d_w, radius, T, (int)nseg, d_low);
    SC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_noise_cols, dim3((unsigned)nparts), dim3(NZ_COL_WAVES * 64), 0, ctx->stream,
                       ctx->z_dev, ny, nx, ctx->dx, ctx->dy, (const double*)d_w, radius, T, (const double*)d_low,
                       (const uint8_t*)d_box, (int)ncb, d_part);
    SC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_noise_merge, dim3(1), dim3(NZ_MERGE), 0, ctx->stream,
                       (const double*)d_part, (int)nparts, d_box ? 2 : 1, d_out);
    SC_HIP(ctx, hipGetLastError());
    SC_HIP(ctx, hipMemcpyAsync(out, d_out, 2 * NZ_STAT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (wp, the caller's mask and nb's buffers outlive the work)
    return SC_OK;
}
