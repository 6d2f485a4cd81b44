// What sc_fit_strike* (sc_strike.hip) and sc_channel_strike* (sc_channel_strike.hip) share (docs/strike.md; docs/channels.md,
// "Width along a reach"): the shape of the window kernels' launches, the checks of the window arrays, the windows of one
// chunk on the device and the launch of k_st_spp.  And what the two bootstraps per station share - sc_strike_bootstrap*
// (sc_strike_bootstrap.hip) and sc_channel_strike_bootstrap* (sc_channel_strike_bootstrap.hip) -: the generator's
// finaliser, the length of the sort and the checks of the block arrays.
#pragma once
#include "sc_fit.h"
#include <limits.h>

#define ST_RUN 64                        // usable profiles per run of a window's sum: sc_fit_segments' SG_BLOCK
#define ST_WAVES 4                       // consecutive stations per workgroup
#define ST_THREADS (64 * ST_WAVES)
#define ST_MAX_GRID 65536
#define ST_MAX_SEGS (1ll << 20)
#define ST_MAX_WIN (1ll << 21)           // windows of a chunk: 0.2 GB of rows, up to 1 GB of curves

static inline unsigned st_grid(long long n) {
    const long long g = (n + ST_WAVES - 1) / ST_WAVES;
    return (unsigned)(g < 1 ? 1 : g > ST_MAX_GRID ? ST_MAX_GRID : g);
}

// the rules of the window arrays: CSR arrays and ranges that fit together (seg_start[s] <= win_lo <= win_hi <=
// seg_start[s + 1]), NW <= 2^31 - 1
int sc_st_check(sc_ctx* ctx, const char* who, const long long* seg_start, long long S, const long long* seg_win_start,
                const long long* win_lo, const long long* win_hi, long long NW, const void* out_rows);
// The windows of the chunk k, cut to its cells and segments, in the context's st_win and st_wstart: win holds (lo, hi,
// segment) of every window, cells and segments counted within the chunk, wstart the segments' CSR array over the windows.
// spp: st_spp is sized for Spp of every cell of the chunk (d_spp; null without).  The host arrays stay with the caller until
// the stream is synchronised
struct st_windows {
    std::vector<int> win, wstart;
    long long NWc = 0;
    int *d_win = nullptr, *d_wstart = nullptr;
    double* d_spp = nullptr;
};
int sc_st_windows(sc_ctx* ctx, const sg_chunk& k, const long long* seg_win_start, const long long* win_lo,
                  const long long* win_hi, bool spp, st_windows& w);
// k_st_spp on the parked profiles of the stage's chunk (st.m >= 1 cells), inside the chunk's timing bracket: Spp_c of every
// usable cell into d_spp
void sc_st_spp_launch(sc_ctx* ctx, const sg_stage& st, int h, double de, double* d_spp);

// ---- the bootstraps per station: sc_strike_bootstrap.hip, shared with sc_channel_strike_bootstrap.hip --------------------------
// the splitmix64 finaliser (sc_bootstrap.h's bs_mix)
__host__ __device__ __forceinline__ unsigned long long sb_mix(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the length of the sort: a power of two >= R
__host__ __device__ __forceinline__ int sb_sort_len(int R) {
    int P2 = 2;
    while (P2 < R) P2 <<= 1;
    return P2;
}

// the rules of R, level and min_blocks, sc_fit_strike's of the windows (sc_st_check), then the blocks: they tile their
// windows exactly, and the block terms of a window - 16 bytes per block and column, A columns - fit lds_terms bytes
static inline int sc_sb_check(sc_ctx* ctx, const char* who, const long long* seg_start, long long S,
                              const long long* seg_win_start, const long long* win_lo, const long long* win_hi, long long NW,
                              const long long* win_blk_start, const long long* blk_hi, long long NWB, int A, int min_blocks,
                              int R, double level, const void* out_rows, long long lds_terms) {
    if (!win_blk_start || (NWB > 0 && !blk_hi)) return sc_fail(ctx, SC_ERR_INVALID, "%s: null argument", who);
    if (R < 1 || R > SC_BOOT_MAX_REPLICATES)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: R must lie in 1..%d", who, SC_BOOT_MAX_REPLICATES);
    if (!(level > 0.0 && level < 1.0)) return sc_fail(ctx, SC_ERR_INVALID, "%s: level must lie strictly between 0 and 1", who);
    if (min_blocks < 2) return sc_fail(ctx, SC_ERR_INVALID, "%s: min_blocks must be >= 2", who);
    int rc = sc_st_check(ctx, who, seg_start, S, seg_win_start, win_lo, win_hi, NW, out_rows);
    if (rc) return rc;
    if (NWB < 0 || NWB > (long long)INT_MAX) return sc_fail(ctx, SC_ERR_INVALID, "%s: NWB must lie in 0..2^31 - 1", who);
    if (win_blk_start[0] != 0 || win_blk_start[NW] != NWB)
        return sc_fail(ctx, SC_ERR_INVALID, "%s: win_blk_start must run from 0 to NWB", who);
    for (long long g = 0; g < NW; ++g)
        if (win_blk_start[g + 1] < win_blk_start[g] || win_blk_start[g + 1] > NWB)
            return sc_fail(ctx, SC_ERR_INVALID, "%s: win_blk_start decreases or leaves 0..NWB at window %lld", who, g);
    for (long long g = 0; g < NW; ++g) {
        long long at = win_lo[g];                        // every block holds a cell and begins where the one before ends
        for (long long b = win_blk_start[g]; b < win_blk_start[g + 1]; ++b) {
            if (blk_hi[b] <= at || blk_hi[b] > win_hi[g])
                return sc_fail(ctx, SC_ERR_INVALID, "%s: block %lld does not lie in window %lld behind the block before it", who, b, g);
            at = blk_hi[b];
        }
        if (at != win_hi[g]) return sc_fail(ctx, SC_ERR_INVALID, "%s: the blocks of window %lld do not cover its cells", who, g);
    }
    for (long long g = 0; g < NW; ++g) {
        const long long nb = win_blk_start[g + 1] - win_blk_start[g];
        if (nb * A * (long long)sizeof(double2) > lds_terms)
            return sc_fail(ctx, SC_ERR_UNSUPPORTED, "%s: window %lld has %lld blocks, more than the %d that %d bytes hold at A = %d",
                           who, g, nb, (int)(lds_terms / (long long)(sizeof(double2) * A)), (int)lds_terms, A);
    }
    return SC_OK;
}

// The windows and the blocks of the chunk k, cut to its cells and segments, in the context's sb_ buffers: win holds (lo, hi,
// segment) of every window, wstart the segments' CSR array over the windows, wblk the windows' CSR array over the blocks -
// counted from the chunk's first -, bhi the end cell of every block within the chunk.  nb_chunk: the blocks of the chunk's
// largest window.  The host arrays stay with the caller until the stream is synchronised
struct sb_windows {
    std::vector<int> win, wstart, wblk, bhi;
    long long NWc = 0;
    int nb_chunk = 0;
    int *d_win = nullptr, *d_wstart = nullptr, *d_wblk = nullptr, *d_bhi = nullptr;
};
static inline int sc_sb_windows(sc_ctx* ctx, const sg_chunk& k, const long long* seg_win_start, const long long* win_lo,
                                const long long* win_hi, const long long* win_blk_start, const long long* blk_hi,
                                sb_windows& w) {
    const long long Sc = k.st.Sc, g0 = seg_win_start[k.s0], b0 = win_blk_start[g0];
    const long long NWc = seg_win_start[k.s1] - g0;
    const long long NBc = win_blk_start[g0 + NWc] - b0;
    int rc;
    w.NWc = NWc;
    w.win.resize(3 * (size_t)NWc);
    w.wstart.resize((size_t)Sc + 1);
    w.wblk.resize((size_t)NWc + 1);
    w.bhi.resize((size_t)NBc);
    w.nb_chunk = 0;
    for (long long s = 0; s <= Sc; ++s) w.wstart[s] = (int)(seg_win_start[k.s0 + s] - g0);
    for (long long s = 0; s < Sc; ++s)
        for (long long g = w.wstart[s]; g < w.wstart[s + 1]; ++g) {
            w.win[3 * g] = (int)(win_lo[g0 + g] - k.k0);
            w.win[3 * g + 1] = (int)(win_hi[g0 + g] - k.k0);
            w.win[3 * g + 2] = (int)s;
        }
    // the block arrays re-based: blocks counted from the chunk's first, cells from the chunk's first
    for (long long g = 0; g <= NWc; ++g) w.wblk[g] = (int)(win_blk_start[g0 + g] - b0);
    for (long long g = 0; g < NWc; ++g) w.nb_chunk = w.wblk[g + 1] - w.wblk[g] > w.nb_chunk ? w.wblk[g + 1] - w.wblk[g] : w.nb_chunk;
    for (long long b = 0; b < NBc; ++b) w.bhi[b] = (int)(blk_hi[b0 + b] - k.k0);
    if ((rc = sc_ensure(ctx, ctx->sb_win, sizeof(int) * 3 * (size_t)NWc))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sb_wstart, sizeof(int) * ((size_t)Sc + 1)))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sb_wblk, sizeof(int) * ((size_t)NWc + 1)))) return rc;
    if ((rc = sc_ensure(ctx, ctx->sb_bhi, sizeof(int) * (size_t)NBc))) return rc;
    w.d_win = (int*)ctx->sb_win.p;
    w.d_wstart = (int*)ctx->sb_wstart.p;
    w.d_wblk = (int*)ctx->sb_wblk.p;
    w.d_bhi = (int*)ctx->sb_bhi.p;
    if (NWc) SC_HIP(ctx, hipMemcpyAsync(w.d_win, w.win.data(), sizeof(int) * 3 * (size_t)NWc, hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(w.d_wstart, w.wstart.data(), sizeof(int) * ((size_t)Sc + 1), hipMemcpyHostToDevice, ctx->stream));
    SC_HIP(ctx, hipMemcpyAsync(w.d_wblk, w.wblk.data(), sizeof(int) * ((size_t)NWc + 1), hipMemcpyHostToDevice, ctx->stream));
    if (NBc) SC_HIP(ctx, hipMemcpyAsync(w.d_bhi, w.bhi.data(), sizeof(int) * (size_t)NBc, hipMemcpyHostToDevice, ctx->stream));
    return SC_OK;
}
