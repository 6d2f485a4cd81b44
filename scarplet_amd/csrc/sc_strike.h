// What sc_fit_strike* (sc_strike.hip) and sc_channel_strike* (sc_channel_strike.hip) share (docs/strike.md; docs/channels.md,
// "Width along a reach"): the shape of the window kernels' launches, the checks of the window arrays, the windows of one
// chunk on the device and the launch of k_st_spp.
#pragma once
#include "sc_fit.h"

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
