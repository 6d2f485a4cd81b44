// Where a fit driver closes a chunk (sc_set_option "fit_chunk") and what the host computes of a chunk of whole segments,
// decided in one place: plain C++ with nothing of HIP in it, so that tests/fit_chunk_check.cpp enumerates it on the host.
// The per-cell calls launch on at most sc_fit_chunk_bound(their chunk, n) cells; the segment calls (sc_fit_segments*,
// sc_bootstrap_segments, sc_fit_along_strike, sc_strike_bootstrap) take whole segments up to sc_fit_chunk_end, and sc_sg_chunks (sc_segment.hip)
// sends up the chunk's arrays as they are made here.
#pragma once
#include <stddef.h>
#include <vector>

#define SG_BLOCK 64                      // usable profiles per block of the segmented sum

// the cells of a chunk: the built-in bound `cap`, lowered - never raised - by the option n > 0
static inline long long sc_fit_chunk_bound(long long cap, long long n) { return n > 0 && n < cap ? n : cap; }

// The cells of one segment that a park of max_park bytes holds: per cell `prof` doubles of the profile (2h + 1, twice that
// with a weight plane) and `planes` doubles for each of the C columns (4, or the 9 of the robust fit; C = A ages, or the
// A (M + 1) pairs of the initial slope), and - shift - one byte a column for d_ci
static inline long long sc_fit_park_cap(long long max_park, long long prof, long long planes, long long C, bool shift) {
    return max_park / (8 * (prof + planes * C) + (shift ? C : 0));
}

// The segment after the last one of the chunk that begins at segment s0 < S.  seg_start is the CSR array of the cells over
// the S segments.  The chunk holds segment s0 whatever its size, and then every next segment while it stays within max_segs
// segments, within max_cells cells and - aux_start given: a second CSR array over the same segments (the windows of
// sc_fit_along_strike, the totals of sc_fit_segments_ramp) - within max_aux of its items.  A segment above a bound
// therefore goes alone, and an empty one joins whatever chunk has room for a segment
static inline long long sc_fit_chunk_end(const long long* seg_start, long long s0, long long S, long long max_segs,
                                         long long max_cells, const long long* aux_start = nullptr, long long max_aux = 0) {
    long long s1 = s0 + 1;
    while (s1 < S && s1 - s0 < max_segs && seg_start[s1 + 1] - seg_start[s0] <= max_cells &&
           (!aux_start || aux_start[s1 + 1] - aux_start[s0] <= max_aux))
        ++s1;
    return s1;
}

// ---- the host arrays of the chunk of segments s0..s1, its cells counted from its first -------------------------------------
// the CSR array of the cells over the chunk's segments
static inline void sc_fit_chunk_start(const long long* seg_start, long long s0, long long s1, std::vector<int>& start) {
    start.resize((size_t)(s1 - s0) + 1);
    for (long long s = s0; s <= s1; ++s) start[s - s0] = (int)(seg_start[s] - seg_start[s0]);
}

// (sa, ca) of the chunk's cells, interleaved
static inline void sc_fit_chunk_dir(const double* sa, const double* ca, long long k0, long long m, std::vector<double>& dir) {
    dir.resize(2 * (size_t)m);
    for (long long k = 0; k < m; ++k) {
        dir[2 * k] = sa[k0 + k];
        dir[2 * k + 1] = ca[k0 + k];
    }
}

// the blocks of SG_BLOCK cells that a segment of n cells is summed in
static inline long long sc_fit_blocks_of(long long n) { return (n + SG_BLOCK - 1) / SG_BLOCK; }

// The segment of every cell (cseg) and the CSR array of the blocks over the chunk's segments (blk): an empty segment has
// no cell and no block.  Returns the number of blocks G = blk[s1 - s0]
static inline long long sc_fit_chunk_blocks(const long long* seg_start, long long s0, long long s1, std::vector<int>& cseg,
                                            std::vector<int>& blk) {
    const long long Sc = s1 - s0, k0 = seg_start[s0];
    blk.resize((size_t)Sc + 1);
    cseg.resize((size_t)(seg_start[s1] - k0));
    blk[0] = 0;
    for (long long s = 0; s < Sc; ++s) {
        const long long a0 = seg_start[s0 + s] - k0, a1 = seg_start[s0 + s + 1] - k0;
        blk[s + 1] = blk[s] + (int)sc_fit_blocks_of(a1 - a0);
        for (long long k = a0; k < a1; ++k) cseg[k] = (int)s;
    }
    return blk[Sc];
}

// the block totals of sc_fit_segments_ramp as a CSR array over all S segments: a segment's blocks and one more
static inline void sc_fit_block_totals(const long long* seg_start, long long S, std::vector<long long>& tot_start) {
    tot_start.assign((size_t)S + 1, 0);
    for (long long s = 0; s < S; ++s) tot_start[s + 1] = tot_start[s] + sc_fit_blocks_of(seg_start[s + 1] - seg_start[s]) + 1;
}
