// Where a fit driver closes a chunk (sc_set_option "fit_chunk"), decided in one place: plain C++ with nothing of HIP in
// it, so that tests/fit_chunk_check.cpp enumerates it on the host.  The per-cell calls launch on at most
// sc_fit_chunk_bound(their chunk, n) cells; the segment calls (sc_fit_segments*, sc_bootstrap_segments,
// sc_fit_along_strike) take whole segments up to sc_fit_chunk_end.
#pragma once

// the cells of a chunk: the built-in bound `cap`, lowered - never raised - by the option n > 0
static inline long long sc_fit_chunk_bound(long long cap, long long n) { return n > 0 && n < cap ? n : cap; }

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
