// sc_trace_planes / sc_trace_result / sc_trace_segments: the traces of a result (docs/traces.md).
//
// From the four float64 planes (amp, age, angle, snr) of a search to a line one cell wide along the strike, cut into
// connected segments, each reduced to a row of a table.  Pipeline (all on the context's stream; one profiling
// bracket SC_K_TRACE before the read-back of K, one after):
//   k_tr_thin          non-maximum suppression across the profile of the cell's winning template -> thin (u8)
//   k_tr_local         union-find in LDS inside 32 x 32 tiles; every cell's parent = its tile component's smallest
//                      index, whose counter is cleared
//   k_tr_merge         the tile borders joined by agent-scope atomicMin on the global parent array
//   k_tr_flatten       parent = root (the component's smallest index); n_cells | n_strong << 32 into the root's counter
//   scan (roots)       components with a strong cell and min_cells cells, numbered 1..K in index order: labels[root]
//   scan (cells)       every segment cell's label, and the cells compacted in row-major order (the read-back of K and
//                      M, the cell count, sizes the rest)
//   k_tr_rs_*          stable LSD radix sort of the compacted cells by label, 8 bits per pass
//   k_tr_reduce        one wave per segment, contiguous now: a fixed shape per length, so the same bits every run
// Integer atomics only (their result does not depend on arrival order); no float atomics.
#include "sc_internal.h"
#include <math.h>
#include <algorithm>

#define TR_PI 3.141592653589793
#define TR_TILE 32                       // union-find tile edge: 32 x 32 cells, 256 threads
#define TR_SCAN_T 256                    // scan block: 16 rows of 256 values
#define TR_SCAN_ROWS 16
#define TR_SCAN_B (TR_SCAN_T * TR_SCAN_ROWS)
#define TR_TOP_T 1024                    // the one workgroup that scans the block sums
#define TR_RS_B 4096                     // radix block: one wave, 64 steps of 64 keys
#define TR_MAX_GRID (1u << 20)           // grids beyond this stride

static unsigned tr_grid(long long work, long long per) {
    long long b = (work + per - 1) / per;
    return (unsigned)std::max<long long>(1, std::min<long long>(b, TR_MAX_GRID));
}

// ---------------------------------------------------------------------------------------------------------------
// 1. thinning
// ---------------------------------------------------------------------------------------------------------------
// The template that won a cell at orientation a has its profile along (cos a, -sin a) in (column, row) units: its
// alpha is -a (WindowedTemplate.py:151) and its xr = x cos(alpha) + y sin(alpha), y running with the row index.  The
// four sectors step (drow, dcol) along that direction; the quantisation uses correctly rounded operations only, so
// that numpy (tests/trace_reference.py) gives the same sector for every angle.
__device__ __forceinline__ int tr_sector(double a) {
    const double q = floor(__dadd_rn(__dmul_rn(__ddiv_rn(a, TR_PI), 4.0), 0.5));
    const double s = __dsub_rn(q, __dmul_rn(4.0, floor(__ddiv_rn(q, 4.0))));
    return (int)s;
}

__device__ __forceinline__ double tr_v(const double* __restrict__ snr, long long r, long long c, int ny, int nx) {
    if (r < 0 || r >= ny || c < 0 || c >= nx) return -INFINITY;
    const double v = snr[r * nx + c];
    return isfinite(v) ? v : -INFINITY;
}

__global__ __launch_bounds__(256) void k_tr_thin(const double* __restrict__ ang, const double* __restrict__ snr,
                                                 int ny, int nx, long long n, double lo, uint8_t* __restrict__ thin) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / nx, c = i - r * nx;
        const double s = snr[i], a = ang[i];
        bool t = false;
        if (isfinite(s) && s > 0.0 && isfinite(a) && fabs(a) <= 1e6 && s >= lo) {
            const int k = tr_sector(a);
            const int dr = k == 0 ? 0 : 1;
            const int dc = k == 0 ? 1 : (k == 1 ? -1 : (k == 2 ? 0 : 1));
            t = s > tr_v(snr, r - dr, c - dc, ny, nx) && s >= tr_v(snr, r + dr, c + dc, ny, nx);
        }
        thin[i] = t ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 2. connected components (8-connectivity), every root the component's smallest linear index
// ---------------------------------------------------------------------------------------------------------------
// Union by atomicMin: a parent only ever decreases and a root is only ever linked below a smaller root, so the
// final root of a component is its smallest member whatever the schedule.
__device__ __forceinline__ int tr_find_lds(volatile int* p, int x) {
    int y = p[x];
    while (y != x) { x = y; y = p[x]; }
    return x;
}

__device__ void tr_union_lds(int* p, int a, int b) {
    volatile int* vp = p;
    bool done;
    do {
        a = tr_find_lds(vp, a);
        b = tr_find_lds(vp, b);
        if (a < b) {
            const int old = atomicMin(&p[b], a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&p[a], b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

// Another workgroup may change any entry of the global array inside the same kernel, and the XCDs' L2s are not
// coherent: every read of it is an agent-scope atomic load.
__device__ __forceinline__ int tr_load(int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int tr_find_g(int* p, int x) {
    int y = tr_load(p + x);
    while (y != x) { x = y; y = tr_load(p + x); }
    return x;
}

__device__ void tr_union_g(int* p, int a, int b) {
    bool done;
    do {
        a = tr_find_g(p, a);
        b = tr_find_g(p, b);
        if (a < b) {
            const int old = __hip_atomic_fetch_min(p + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

// One workgroup per 32 x 32 tile: components inside the tile in LDS.  Row-major order inside a tile is the global
// order, so the tile component's smallest local index is its smallest global index; a global root is always a tile
// root, and the tile roots' counters are cleared here for k_tr_flatten.
__global__ __launch_bounds__(256) void k_tr_local(const uint8_t* __restrict__ thin, int ny, int nx, long long tiles_x,
                                                  long long ntiles, int* __restrict__ parent,
                                                  unsigned long long* __restrict__ cnt) {
    __shared__ int lp[TR_TILE * TR_TILE];
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long ty = t / tiles_x, tx = t - ty * tiles_x;
        const long long r0 = ty * TR_TILE, c0 = tx * TR_TILE;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int li = tid + 256 * k;
            const long long r = r0 + (li >> 5), c = c0 + (li & 31);
            const bool on = r < ny && c < nx && thin[r * nx + c];
            lp[li] = on ? li : -1;
        }
        __syncthreads();
        volatile int* vp = lp;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int li = tid + 256 * k;
            if (vp[li] < 0) continue;
            const int lr = li >> 5, lc = li & 31;
            if (lc > 0 && vp[li - 1] >= 0) tr_union_lds(lp, li, li - 1);
            if (lr > 0) {
                if (lc > 0 && vp[li - 33] >= 0) tr_union_lds(lp, li, li - 33);
                if (vp[li - 32] >= 0) tr_union_lds(lp, li, li - 32);
                if (lc < 31 && vp[li - 31] >= 0) tr_union_lds(lp, li, li - 31);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int li = tid + 256 * k;
            const long long r = r0 + (li >> 5), c = c0 + (li & 31);
            if (r >= ny || c >= nx) continue;
            const long long g = r * nx + c;
            if (lp[li] < 0) {
                parent[g] = -1;
                continue;
            }
            const int root = tr_find_lds(vp, li);
            parent[g] = (int)((r0 + (root >> 5)) * nx + c0 + (root & 31));
            if (root == li) cnt[g] = 0ull;
        }
        __syncthreads();
    }
}

// The cells on a tile border joined with their neighbours in other tiles (each pair once: the four neighbours
// before the cell in row-major order).
__global__ __launch_bounds__(256) void k_tr_merge(const uint8_t* __restrict__ thin, int ny, int nx, long long n,
                                                  int* parent) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / nx, c = i - r * nx;
        const int lr = (int)(r & 31), lc = (int)(c & 31);
        if (!(lr == 0 || lc == 0 || lc == 31) || !thin[i]) continue;
        const int nb[4][2] = {{0, -1}, {-1, -1}, {-1, 0}, {-1, 1}};
        for (int k = 0; k < 4; ++k) {
            const long long rr = r + nb[k][0], cc = c + nb[k][1];
            if (rr < 0 || cc < 0 || cc >= nx) continue;
            if ((rr >> 5) == (r >> 5) && (cc >> 5) == (c >> 5)) continue;
            const long long j = rr * nx + cc;
            if (thin[j]) tr_union_g(parent, (int)i, (int)j);
        }
    }
}

// parent = root, and the root's counter gains 1 | strong << 32 (integer atomics: the same counts every run)
__global__ __launch_bounds__(256) void k_tr_flatten(const double* __restrict__ snr, long long n, double hi, int* parent,
                                                    unsigned long long* cnt) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int p = tr_load(parent + i);
        if (p < 0) continue;
        const int root = tr_find_g(parent, p);
        if (root != p) __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long add = 1ull | (snr[i] >= hi ? (1ull << 32) : 0ull);
        atomicAdd(cnt + root, add);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 3. exclusive scans over the cells in index order (three launches: block sums, their scan in one workgroup, apply)
// ---------------------------------------------------------------------------------------------------------------
// Component roots that are segments: one count each; the sink numbers them 1..K into labels[root] (0 elsewhere).
struct OpRoots {
    const int* parent;
    const unsigned long long* cnt;
    long long min_cells;
    int* labels;
    __device__ int value(long long i) const {
        if (parent[i] != (int)i) return 0;
        const unsigned long long c = cnt[i];
        return ((c >> 32) >= 1ull && (long long)(c & 0xffffffffull) >= min_cells) ? 1 : 0;
    }
    __device__ void sink(long long i, int excl, int v) const { labels[i] = v ? excl + 1 : 0; }
};

// Segment cells: the sink compacts them in row-major order (cell, label - 1) and writes the labels of the non-root
// cells (a root's label is only read here, and only non-root entries are written).
struct OpCells {
    const int* parent;
    int* labels;
    int* cells;
    int* keys;
    __device__ int value(long long i) const {
        const int p = parent[i];
        return (p >= 0 && labels[p] > 0) ? 1 : 0;
    }
    __device__ void sink(long long i, int excl, int v) const {
        if (!v) return;
        const int p = parent[i];
        const int l = labels[p];
        cells[excl] = (int)i;
        keys[excl] = l - 1;
        if (p != (int)i) labels[i] = l;
    }
};

// A plain array (the radix histograms): out[i] = exclusive prefix
struct OpArray {
    int* a;
    __device__ int value(long long i) const { return a[i]; }
    __device__ void sink(long long i, int excl, int) const { a[i] = excl; }
};

// inclusive scan of v over a workgroup of NW waves; *total = the workgroup's sum
template <int NW>
__device__ __forceinline__ int tr_block_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int s = lds[k];
        pre += k < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return x + pre;
}

template <class Op>
__global__ __launch_bounds__(TR_SCAN_T) void k_tr_scan_reduce(Op op, long long n, long long nb, int* __restrict__ bsum) {
    __shared__ int lds[TR_SCAN_T / 64];
    for (long long b = blockIdx.x; b < nb; b += gridDim.x) {
        int s = 0;
        for (int row = 0; row < TR_SCAN_ROWS; ++row) {
            const long long i = b * TR_SCAN_B + row * TR_SCAN_T + threadIdx.x;
            if (i < n) s += op.value(i);
        }
        int tot;
        (void)tr_block_scan<TR_SCAN_T / 64>(s, lds, tot);
        if (threadIdx.x == 0) bsum[b] = tot;
    }
}

// one workgroup: bsum[0..nb) -> exclusive prefix, *total = the sum
__global__ __launch_bounds__(TR_TOP_T) void k_tr_scan_top(int* __restrict__ bsum, long long nb, long long* __restrict__ total) {
    __shared__ int lds[TR_TOP_T / 64];
    const long long per = (nb + TR_TOP_T - 1) / TR_TOP_T;
    const long long i0 = std::min<long long>(nb, per * threadIdx.x), i1 = std::min<long long>(nb, i0 + per);
    int s = 0;
    for (long long i = i0; i < i1; ++i) s += bsum[i];
    int tot;
    int run = tr_block_scan<TR_TOP_T / 64>(s, lds, tot) - s;
    for (long long i = i0; i < i1; ++i) {
        const int v = bsum[i];
        bsum[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total = tot;
}

template <class Op>
__global__ __launch_bounds__(TR_SCAN_T) void k_tr_scan_apply(Op op, long long n, long long nb, const int* __restrict__ bsum) {
    __shared__ int lds[TR_SCAN_T / 64];
    for (long long b = blockIdx.x; b < nb; b += gridDim.x) {
        int carry = bsum[b];
        for (int row = 0; row < TR_SCAN_ROWS; ++row) {
            const long long i = b * TR_SCAN_B + row * TR_SCAN_T + threadIdx.x;
            const int v = i < n ? op.value(i) : 0;
            int tot;
            const int incl = tr_block_scan<TR_SCAN_T / 64>(v, lds, tot);
            if (i < n) op.sink(i, carry + incl - v, v);
            carry += tot;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 4. stable LSD radix sort of (key, value) by key, 8 bits per pass; one wave per block of 4096 keys
// ---------------------------------------------------------------------------------------------------------------
// ghist[d * nb + b]: keys of block b whose digit is d (digit-major, so that the exclusive scan gives every (digit,
// block) its first output position)
__global__ __launch_bounds__(64) void k_tr_rs_hist(const int* __restrict__ keys, long long m, int shift, long long nb,
                                                   int* __restrict__ ghist) {
    __shared__ int h[256];
    const int lane = threadIdx.x;
    for (long long b = blockIdx.x; b < nb; b += gridDim.x) {
        for (int d = lane; d < 256; d += 64) h[d] = 0;
        __syncthreads();
        for (int step = 0; step < TR_RS_B / 64; ++step) {
            const long long i = b * TR_RS_B + step * 64 + lane;
            if (i < m) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
        }
        __syncthreads();
        for (int d = lane; d < 256; d += 64) ghist[(long long)d * nb + b] = h[d];
        __syncthreads();
    }
}

// Keys in order, 64 at a time: a key's rank among the equal digits of its step (ballots over the 8 digit bits) plus
// what the earlier steps of the block placed - the order of equal digits is kept.
__global__ __launch_bounds__(64) void k_tr_rs_scatter(const int* __restrict__ kin, const int* __restrict__ vin, long long m,
                                                      int shift, long long nb, const int* __restrict__ ghist,
                                                      int* __restrict__ kout, int* __restrict__ vout) {
    __shared__ int base[256];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long b = blockIdx.x; b < nb; b += gridDim.x) {
        for (int d = lane; d < 256; d += 64) base[d] = ghist[(long long)d * nb + b];
        __syncthreads();
        for (int step = 0; step < TR_RS_B / 64; ++step) {
            const long long i = b * TR_RS_B + step * 64 + lane;
            const bool act = i < m;
            const int key = act ? kin[i] : 0;
            const int d = (key >> shift) & 255;
            unsigned long long peers = __ballot(act);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool on = (d >> bit) & 1;
                const unsigned long long bb = __ballot(on);
                peers &= on ? bb : ~bb;
            }
            const int pos = base[d] + __popcll(peers & below);
            __syncthreads();
            if (act) {
                kout[pos] = key;
                vout[pos] = vin[i];
                if ((peers >> lane) == 1ull) base[d] += __popcll(peers);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 5. the table: one wave per segment over its contiguous cells (lane-strided sums, then a fixed butterfly)
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double tr_xor(double v, int o) { return __shfl_xor(v, o, 64); }

__global__ __launch_bounds__(64) void k_tr_reduce(const int* __restrict__ keys, const int* __restrict__ cells, long long m,
                                                  long long K, const double* __restrict__ planes, long long nc, int nx,
                                                  const unsigned long long* __restrict__ cnt, sc_segment* __restrict__ out) {
    const int lane = threadIdx.x;
    const double* amp = planes;
    const double* age = planes + nc;
    const double* ang = planes + 2 * nc;
    const double* snr = planes + 3 * nc;
    for (long long s = blockIdx.x; s < K; s += gridDim.x) {
        long long lo = 0, hi = m;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (keys[mid] < s) lo = mid + 1; else hi = mid;
        }
        const long long start = lo;
        const int first = cells[start];
        const unsigned long long c = cnt[first];
        const long long ncell = (long long)(c & 0xffffffffull);
        double s_amp = 0.0, s_abs = 0.0, s_age = 0.0, s_snr = 0.0, s_c2 = 0.0, s_s2 = 0.0;
        double pk_snr = -INFINITY;
        int pk = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
        for (long long k = start + lane; k < start + ncell; k += 64) {
            const int x = cells[k];
            const int r = x / nx, col = x - r * nx;
            const double va = amp[x], vs = snr[x], a2 = 2.0 * ang[x];
            s_amp += va;
            s_abs += fabs(va);
            s_age += age[x];
            s_snr += vs;
            s_c2 += cos(a2);
            s_s2 += sin(a2);
            if (vs > pk_snr || (vs == pk_snr && x < pk)) { pk_snr = vs; pk = x; }
            rmax = max(rmax, r);
            cmin = min(cmin, col);
            cmax = max(cmax, col);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            s_amp += tr_xor(s_amp, o);
            s_abs += tr_xor(s_abs, o);
            s_age += tr_xor(s_age, o);
            s_snr += tr_xor(s_snr, o);
            s_c2 += tr_xor(s_c2, o);
            s_s2 += tr_xor(s_s2, o);
            const double os = tr_xor(pk_snr, o);
            const int op = __shfl_xor(pk, o, 64);
            if (os > pk_snr || (os == pk_snr && op < pk)) { pk_snr = os; pk = op; }
            rmax = max(rmax, __shfl_xor(rmax, o, 64));
            cmin = min(cmin, __shfl_xor(cmin, o, 64));
            cmax = max(cmax, __shfl_xor(cmax, o, 64));
        }
        if (lane == 0) {
            sc_segment g;
            g.first = first;
            g.n_cells = ncell;
            g.n_strong = (long long)(c >> 32);
            g.row_min = first / nx;
            g.row_max = rmax;
            g.col_min = cmin;
            g.col_max = cmax;
            g.peak = pk;
            g.snr_peak = snr[pk];
            g.amp_peak = amp[pk];
            g.age_peak = age[pk];
            g.angle_peak = ang[pk];
            g.sum_amp = s_amp;
            g.sum_abs_amp = s_abs;
            g.sum_age = s_age;
            g.sum_snr = s_snr;
            g.sum_cos2a = s_c2;
            g.sum_sin2a = s_s2;
            out[s] = g;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
template <class Op>
static int tr_scan_blocks(sc_ctx* ctx, const Op& op, long long n, long long* total_dev, int* bsum, bool apply) {
    const long long nb = (n + TR_SCAN_B - 1) / TR_SCAN_B;
    k_tr_scan_reduce<Op><<<tr_grid(nb, 1), TR_SCAN_T, 0, ctx->stream>>>(op, n, nb, bsum);
    k_tr_scan_top<<<1, TR_TOP_T, 0, ctx->stream>>>(bsum, nb, total_dev);
    if (apply) k_tr_scan_apply<Op><<<tr_grid(nb, 1), TR_SCAN_T, 0, ctx->stream>>>(op, n, nb, bsum);
    SC_HIP(ctx, hipGetLastError());
    return SC_OK;
}

static size_t tr_bsum_bytes(long long n) { return sizeof(int) * (size_t)((n + TR_SCAN_B - 1) / TR_SCAN_B + 1); }

// the whole sequence on four float64 planes of ny x nx cells already on the device
static int tr_run(sc_ctx* ctx, const double* planes, int ny, int nx, double lo, double hi, long long min_cells,
                  uint8_t* thin_out, int32_t* labels_out, long long* n_segments) {
    const long long n = (long long)ny * nx;
    const double* ang = planes + 2 * n;
    const double* snr = planes + 3 * n;
    int rc;
    if ((rc = sc_ensure(ctx, ctx->tr_thin, (size_t)n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->tr_par, sizeof(int) * (size_t)n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->tr_lab, sizeof(int) * (size_t)n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->tr_cnt, sizeof(unsigned long long) * (size_t)n))) return rc;
    if ((rc = sc_ensure(ctx, ctx->tr_bsum, tr_bsum_bytes(n)))) return rc;
    if ((rc = sc_ensure(ctx, ctx->tr_tot, 4 * sizeof(long long)))) return rc;
    uint8_t* thin = (uint8_t*)ctx->tr_thin.p;
    int* parent = (int*)ctx->tr_par.p;
    int* labels = (int*)ctx->tr_lab.p;
    unsigned long long* cnt = (unsigned long long*)ctx->tr_cnt.p;
    int* bsum = (int*)ctx->tr_bsum.p;
    long long* tot = (long long*)ctx->tr_tot.p;
    ctx->tr_k = 0;

    sc_prof_begin(ctx, SC_K_TRACE);
    k_tr_thin<<<tr_grid(n, 256), 256, 0, ctx->stream>>>(ang, snr, ny, nx, n, lo, thin);
    const long long tiles_x = (nx + TR_TILE - 1) / TR_TILE, ntiles = tiles_x * ((ny + TR_TILE - 1) / TR_TILE);
    k_tr_local<<<tr_grid(ntiles, 1), 256, 0, ctx->stream>>>(thin, ny, nx, tiles_x, ntiles, parent, cnt);
    k_tr_merge<<<tr_grid(n, 256), 256, 0, ctx->stream>>>(thin, ny, nx, n, parent);
    k_tr_flatten<<<tr_grid(n, 256), 256, 0, ctx->stream>>>(snr, n, hi, parent, cnt);
    SC_HIP(ctx, hipGetLastError());
    OpRoots roots{parent, cnt, min_cells, labels};
    if ((rc = tr_scan_blocks(ctx, roots, n, tot, bsum, true))) return rc;
    // the cells' scan up to its block sums; the apply pass follows once M has sized the compacted list
    OpCells cells_op{parent, labels, nullptr, nullptr};
    if ((rc = tr_scan_blocks(ctx, cells_op, n, tot + 1, bsum, false))) return rc;
    sc_prof_end(ctx, 9);

    // the one read-back: K and M
    long long km[2] = {0, 0};
    SC_HIP(ctx, hipMemcpyAsync(km, tot, sizeof(km), hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const long long K = km[0], M = km[1];

    if (M > 0) {
        if ((rc = sc_ensure(ctx, ctx->tr_sort, sizeof(int) * 4 * (size_t)M))) return rc;
        int* k0 = (int*)ctx->tr_sort.p;
        int* v0 = k0 + M;
        int* k1 = v0 + M;
        int* v1 = k1 + M;
        const long long nbr = (M + TR_RS_B - 1) / TR_RS_B;
        int passes = 0;
        for (long long top = K - 1; top > 0; top >>= 8) ++passes;
        if ((rc = sc_ensure(ctx, ctx->tr_hist, sizeof(int) * 256 * (size_t)nbr))) return rc;
        if ((rc = sc_ensure(ctx, ctx->tr_rbsum, tr_bsum_bytes(256 * nbr)))) return rc;
        if ((rc = sc_ensure(ctx, ctx->tr_seg, sizeof(sc_segment) * (size_t)K))) return rc;
        sc_prof_begin(ctx, SC_K_TRACE);
        cells_op.cells = v0;
        cells_op.keys = k0;
        {
            const long long nb = (n + TR_SCAN_B - 1) / TR_SCAN_B;
            k_tr_scan_apply<OpCells><<<tr_grid(nb, 1), TR_SCAN_T, 0, ctx->stream>>>(cells_op, n, nb, bsum);
        }
        int* hist = (int*)ctx->tr_hist.p;
        for (int p = 0; p < passes; ++p) {
            k_tr_rs_hist<<<tr_grid(nbr, 1), 64, 0, ctx->stream>>>(k0, M, 8 * p, nbr, hist);
            if ((rc = tr_scan_blocks(ctx, OpArray{hist}, 256 * nbr, tot + 2, (int*)ctx->tr_rbsum.p, true))) return rc;
            k_tr_rs_scatter<<<tr_grid(nbr, 1), 64, 0, ctx->stream>>>(k0, v0, M, 8 * p, nbr, hist, k1, v1);
            std::swap(k0, k1);
            std::swap(v0, v1);
        }
        k_tr_reduce<<<tr_grid(K, 1), 64, 0, ctx->stream>>>(k0, v0, M, K, planes, n, nx, cnt, (sc_segment*)ctx->tr_seg.p);
        SC_HIP(ctx, hipGetLastError());
        sc_prof_end(ctx, 2 + 5 * passes);
    }
    // (no segment cell: the labels are what the roots' scan left, all zero)
    if (thin_out) SC_HIP(ctx, hipMemcpyAsync(thin_out, thin, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (labels_out) SC_HIP(ctx, hipMemcpyAsync(labels_out, labels, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tr_k = K;
    if (n_segments) *n_segments = K;
    return SC_OK;
}

static int tr_check(sc_ctx* ctx, long long ny, long long nx, double lo, double hi, long long min_cells) {
    if (ny <= 0 || nx <= 0) return sc_fail(ctx, SC_ERR_INVALID, "sc_trace: empty grid");
    if (!(isfinite(lo) && lo > 0.0)) return sc_fail(ctx, SC_ERR_INVALID, "sc_trace: snr_low must be finite and > 0");
    if (!(isfinite(hi) && hi >= lo)) return sc_fail(ctx, SC_ERR_INVALID, "sc_trace: snr_high must be finite and >= snr_low");
    if (min_cells < 1) return sc_fail(ctx, SC_ERR_INVALID, "sc_trace: min_cells must be >= 1");
    if (ny * nx > (long long)INT_MAX)
        return sc_fail(ctx, SC_ERR_UNSUPPORTED, "sc_trace: %lld cells, more than 2^31 - 1", ny * nx);
    return SC_OK;
}

extern "C" int sc_trace_planes(sc_ctx* ctx, const double* planes, int ny, int nx, double snr_low, double snr_high,
                               long long min_cells, uint8_t* thin, int32_t* labels, long long* n_segments) {
    if (!ctx || !planes) return SC_ERR_INVALID;
    int rc = tr_check(ctx, ny, nx, snr_low, snr_high, min_cells);
    if (rc) return rc;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 4 * (size_t)ny * (size_t)nx;
    if ((rc = sc_ensure(ctx, ctx->tr_planes, bytes))) return rc;
    SC_HIP(ctx, hipMemcpyAsync(ctx->tr_planes.p, planes, bytes, hipMemcpyHostToDevice, ctx->stream));
    return tr_run(ctx, (const double*)ctx->tr_planes.p, ny, nx, snr_low, snr_high, min_cells, thin, labels, n_segments);
}

extern "C" int sc_trace_result(sc_ctx* ctx, const double* param_of_id, const double* angle_of_id, int n_ids,
                               double snr_low, double snr_high, long long min_cells, uint8_t* thin, int32_t* labels,
                               long long* n_segments) {
    if (!ctx || !param_of_id || !angle_of_id || n_ids <= 0) return SC_ERR_INVALID;
    if (!ctx->have_dem) return sc_fail(ctx, SC_ERR_NO_DEM, "no DEM set");
    const long long ny = ctx->g.cy1 - ctx->g.cy0, nx = ctx->g.cx1 - ctx->g.cx0;
    int rc = tr_check(ctx, ny, nx, snr_low, snr_high, min_cells);
    if (rc) return rc;
    double* planes = nullptr;
    size_t nc = 0;
    if ((rc = sc_result_planes(ctx, param_of_id, angle_of_id, n_ids, &planes, &nc))) return rc;
    return tr_run(ctx, planes, (int)ny, (int)nx, snr_low, snr_high, min_cells, thin, labels, n_segments);
}

extern "C" int sc_trace_segments(sc_ctx* ctx, sc_segment* out, long long n) {
    if (!ctx || n < 0 || n > ctx->tr_k || (n > 0 && !out)) return SC_ERR_INVALID;
    if (n == 0) return SC_OK;
    SC_HIP(ctx, hipSetDevice(ctx->device));
    SC_HIP(ctx, hipMemcpyAsync(out, ctx->tr_seg.p, sizeof(sc_segment) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SC_OK;
}
