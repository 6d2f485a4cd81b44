// The FFT path's route: which kernels a chunk of templates takes, decided in ONE place.
//
// fft_route() is a pure function of the tile plan, the chunk and the options - nothing of HIP, so that a host
// compiler can build it alone (tests/fft_route_check.cpp enumerates it under AddressSanitizer / UBSan).  The host
// code of sc_fft.hip and its launchers, one per kernel family, ask it and test no tile size and no
// "variant" for themselves.  The shape of the launches is here too, as integer arithmetic on the tile plan, the chunk
// and the route: tile pairs per column launch and their interleave (fft_route_col_pairs), parts of an under-filled
// column pass (fft_route_parts), slices and shares of the row pass (fft_route_nsplit_max, fft_route_row_slice,
// fft_route_nsplit).  ONE input depends on the device: how many tile pairs the hand-off buffers hold (fft_pb, from the
// free memory: fft_prepare) - it arrives here as `pc`, the tile pairs of a chunk.  fft_inverse_fold keeps the pointer
// arithmetic, the buffers and the launches.
#pragma once
#include "../../include/scarplet_hip.h"      // (the error codes: plain C)

// templates per inverse launch (sc_match batches an orientation run in chunks)
#define SC_MAX_GROUP 64
// templates one batched launch SEQUENCE can carry (forward passes and column pass of nb orientations x n
// templates each); the row pass folds them in launches of at most SC_MAX_GROUP, orientation slice after slice
#define SC_MAX_BATCH 256
#define SC_MAX_ORIENT 64         // orientations (curvature planes) one launch sequence can carry

enum FftColKernel {              // I1
    FFT_COL_GENERIC,             // k_inv_cols: complex spectra, own columns + mirrors in two launches
    FFT_COL_SYM,                 // k_inv_cols_sym: symmetric templates, two launches (small tiles; cross-check variant 6)
    FFT_COL_SYMX,                // k_inv_cols_symx: the same in one launch, paired per XCD
    FFT_COL_SYMX_XP,             //   ... with paired orientations
    FFT_COL_W8,                  // k_inv_cols_w8: one wave per column, length 1024 / 2048
    FFT_COL_W4,                  // k_inv_cols_w4: the four-wave form, paired templates at 2048
    FFT_COL_H2,                  // k_inv_cols_h2: half a wave per column, length 512
    FFT_COL_H2_XP                //   ... with paired orientations (variant 19)
};
enum FftRowKernel {              // I2
    FFT_ROW_GENERIC,             // k_inv_rows
    FFT_ROW_FAST,                // k_inv_rows_fast
    FFT_ROW_NEAR,                //   ... with near-tie flags
    FFT_ROW_SPLIT                //   ... dealt out over up to split_max workgroups per row + k_merge_split (with near-tie
                                 //   flags where `near`), for the groups of at least split_min_g templates whose launch
                                 //   comes to more than one share; the plain or near-tie form for the others
};
enum FftTemplFwd {               // the templates' column transform and split
    FFT_TEMPL_SPLIT,             // k_fwd_cols + k_split_templ
    FFT_TEMPL_SPLIT_SYM,         // k_fwd_cols + k_split_templ_sym (variant 7)
    FFT_TEMPL_COLS_SYM           // k_fwd_cols_tsym: both in one kernel
};

struct FftRouteIn {
    int Ty, Tx, ntiles;
    int parity;                  // of the chunk's templates: 0 none (complex spectra), 1 odd, 2 even
    bool full_masks, to_maps;
    bool near;                   // near-tie flags on (option "near_window" > 0)
    bool kept;                   // curvature spectra are kept across searches (they live in uc / uc2)
    int nb, n, group;            // batched orientations, templates per orientation, templates per inverse launch
    int variant, sib, i1_pairs, split_i1;
    long long split_fill;
    int fuse_fwd, batch_off, batch_templ, batch_fill;
};
struct FftChunkRoute {
    FftColKernel col;
    FftRowKernel row;
    int jil;                     // w8: tile pairs interleaved along x per launch, at most (1: one pair after the other)
    int split_min_g, split_max;  // FFT_ROW_SPLIT: see there
    long long split_waves;       //   ... and the waves such a launch may come to
};
struct FftRoute {
    int err;                     // SC_OK, or the refusal: what fft_inverse_fold / fft_prepare answer, with `msg`
    const char* msg;             // (a format: the unsupported sizes take Ty, Tx)
    FftTemplFwd templ;
    bool fused;                  // option "fuse_fwd", asked when the search is prepared: fft_forward_curv leaves the
                                 // curvature's row spectra in cblk.  Answered for the parity that gives the most - the
                                 // templates' parity is not known yet then -, so a chunk may still need k_fwd_cols
                                 // (answered in a refusal too, but for the sizes'):
    bool fwd;                    // this chunk's column pass (w8 / w4) transforms the curvature columns it parks, from cblk
    bool cols_first;             // fused, but not for this chunk: k_fwd_cols runs first, from cblk, once
    bool row_skip;               // rows masked by the templates' window limits are neither stored nor scored
    bool near;                   // the row pass flags near-ties
    bool sib_rows;               // the fast row kernel's sibling rendezvous (option "sib", bit 0)
    int split_i1;                // option "split_i1", for the column launchers' fft_route_parts
    bool pt;                     // the odd tile rides alone in a chunk of its own, templates in pairs
    FftChunkRoute main, ptc;     // the chunks of whole tile pairs; the paired-template chunk (where pt)
};

inline bool fft_route_size_ok(int T) { return T >= 64 && T <= 4096 && (T & (T - 1)) == 0; }
// the fast row kernel: its sizes (variant 9: the generic kernel everywhere)
inline bool fft_route_fast(const FftRouteIn& in) {
    return (in.Tx == 512 || in.Tx == 1024 || in.Tx == 2048) && in.variant != 9;
}
inline bool fft_route_xp(FftColKernel k) { return k == FFT_COL_SYMX_XP || k == FFT_COL_H2_XP; }

static const char* const FFT_REFUSE_SIZE = "FFT tile %dx%d not supported";
static const char* const FFT_REFUSE_BATCH = "orientation batching outside its conditions";
static const char* const FFT_REFUSE_NEAR = "near-tie flags need the fast row kernel without per-cell masks";

inline FftRoute fft_route(const FftRouteIn& in) {
    FftRoute r{};
    const int Ty = in.Ty, Tx = in.Tx, v = in.variant;
    if (!fft_route_size_ok(Ty) || !fft_route_size_ok(Tx)) {
        r.err = SC_ERR_UNSUPPORTED; r.msg = FFT_REFUSE_SIZE;
        return r;
    }
    const bool fast = fft_route_fast(in);
    // Symmetric templates (k_inv_cols_sym ...): all templates of the chunk share one parity and the tile is small
    // enough for the parked spectrum.  symx: block and mirror workgroups in one launch, paired per XCD.  w8: one
    // wave per column - column length 1024 / 2048, eight column blocks and their mirrors per sixteen workgroup ids.
    auto sym_at = [&](int parity) { return parity != 0 && Ty <= 2048 && v != 8; };
    auto symx_at = [&](int parity) { return sym_at(parity) && v != 6 && Ty >= 512 && (Tx / 8) % 8 == 0; };
    auto w8_at = [&](int parity) {
        return symx_at(parity) && v != 2 && (Ty == 2048 || Ty == 1024) && (Tx / 16) % 8 == 0;
    };
    const bool sym = sym_at(in.parity), symx = symx_at(in.parity), w8 = w8_at(in.parity);
    r.templ = !sym ? FFT_TEMPL_SPLIT : v == 7 ? FFT_TEMPL_SPLIT_SYM : FFT_TEMPL_COLS_SYM;
    // the forward column transform of the curvature is left to the wave-per-column pass where a chunk of symmetric
    // templates would take it (any non-zero parity: the most a chunk can give) and uc / uc2 need not exist
    r.fused = in.fuse_fwd && !in.kept && w8_at(1) && v != 1;
    r.fwd = r.fused && w8 && !in.to_maps;
    r.cols_first = r.fused && !r.fwd;
    r.row_skip = !in.full_masks && !in.to_maps && v != 13;      // (masks and maps write every cell; variant 13: off)
    r.near = in.near && !in.to_maps;
    r.sib_rows = fast && (in.sib & 1);
    r.split_i1 = in.split_i1;
    r.pt = sym && fast && (in.ntiles & 1) && v != 5;
    if (in.nb > 1 && (!fast || in.n > in.group || in.nb * in.n > SC_MAX_BATCH || in.n > SC_MAX_GROUP)) {
        r.err = SC_ERR_INVALID; r.msg = FFT_REFUSE_BATCH;
        return r;
    }
    // (the chunks are named all the same: fft_inverse_fold answers this refusal where the row pass would be launched,
    //  after the chunk's column pass - a search of no templates is not refused)
    if (r.near && (!fast || in.full_masks)) { r.err = SC_ERR_UNSUPPORTED; r.msg = FFT_REFUSE_NEAR; }
    auto chunk = [&](bool pt) {
        FftChunkRoute c{};
        // Paired orientations: a paired-template chunk with ONE template per orientation and a batch of orientations
        // would run every transform half empty (variant 12: off).  They stay on the four-column kernel - one transform
        // per plane and job, all prologue; variant 19 takes the sixteen-column one anyway.
        const bool xp = pt && in.n == 1 && in.nb >= 2 && symx && Ty == 512 && v != 12 && !in.to_maps;
        // column length 512: half a wave per column where the grid pairs up per XCD (variant 18: the four-column kernels)
        const bool h2 = symx && Ty == 512 && (Tx / 32) % 8 == 0 && v != 18 && v != 1 && v != 2;
        // paired templates at 2048 take the four-wave form: with eight waves the second coefficient plane does not fit
        c.col = xp                                        ? (h2 && v == 19 ? FFT_COL_H2_XP : FFT_COL_SYMX_XP)
                : h2                                      ? FFT_COL_H2
                : w8 && (!pt || (Ty == 1024 && v != 1))   ? FFT_COL_W8
                : w8 && pt && Ty == 2048 && v != 1        ? FFT_COL_W4
                : symx                                    ? FFT_COL_SYMX
                : sym                                     ? FFT_COL_SYM
                                                          : FFT_COL_GENERIC;
        c.jil = c.col == FFT_COL_W8 && in.nb == 1 && v != 1 && in.i1_pairs > 1 ? in.i1_pairs : 1;
        // The dealt-out row pass (small grids; variant 15: off).  With near-tie flags on only for groups of four
        // templates and more and never for paired orientations: a share meets the record as the launch found it
        // and lists near-ties against that floor that the sequential fold would not.  Variant 20: one share
        // whatever the grid - the launch is still held to what one share may carry.
        const bool split = fast && !(in.near && xp) && !in.to_maps && !in.full_masks && Tx <= 1024 && v != 15 &&
                           !(in.sib & 1);
        c.row = !fast ? FFT_ROW_GENERIC : split ? FFT_ROW_SPLIT : r.near ? FFT_ROW_NEAR : FFT_ROW_FAST;
        c.split_min_g = in.near ? 4 : 1;
        c.split_max = v == 20 ? 1 : 4;
        c.split_waves = in.split_fill > 0 ? in.split_fill : 4300;
        return c;
    };
    r.main = chunk(false);
    r.ptc = chunk(true);
    return r;
}

// Orientations one launch sequence carries (asked by sc_match_plan; in.n templates per orientation).  Conditions:
// the fast row kernel (its scalar table and winner byte hold SC_MAX_GROUP templates), all templates of an
// orientation in one inverse launch (group >= n), and at most ~4096 column workgroups.
inline int fft_route_batch(const FftRouteIn& in) {
    if (in.batch_off || in.n < 1 || in.n > in.group || !fft_route_fast(in)) return 1;
    const int np = (in.ntiles + 1) / 2;
    // What one launch sequence may carry.  The row pass folds at most SC_MAX_GROUP templates per launch: where three
    // or more orientations fit that (C2: six of ten templates), the batch stops there and the row pass takes it in ONE
    // launch (more, sliced over two row-pass launches, cost C2's row pass 14 %); where they do not (C1F: 35 ages, one
    // orientation per row-pass launch either way) the forward passes and the column pass batch up to SC_MAX_BATCH
    // templates - 181 five-kernel launch sequences of a few microseconds each were 15 of C1F's 52 ms, now 6
    const int cap = in.batch_templ > 0 ? in.batch_templ : SC_MAX_BATCH;
    const int capg = cap < SC_MAX_GROUP ? cap : SC_MAX_GROUP;
    const int by_table = (SC_MAX_GROUP / in.n >= 3 || cap <= SC_MAX_GROUP) ? capg / in.n : cap / in.n;
    // (4096 workgroups and up to SC_MAX_ORIENT orientations - BASELINE config C5, one template per orientation on a
    //  512 x 512 tile, runs 64 orientations per launch sequence instead of 32: 5.95 -> 5.2 ms)
    const int wgs = np * (in.Tx / 8);
    const int by_fill = (in.batch_fill > 0 ? in.batch_fill : 4096) / (wgs > 1 ? wgs : 1);
    int nb = by_table < by_fill ? by_table : by_fill;
    if (nb > SC_MAX_ORIENT) nb = SC_MAX_ORIENT;
    return nb > 1 ? nb : 1;
}

// Parts (grid.z) of an under-filled column pass: so that the launch's workgroups come up to the chip's resident
// capacity for the kernel, every part at least four transforms.  Option "split_i1" 0: off.
inline int fft_route_parts(int split_i1, long long workgroups, long long capacity, int transforms) {
    if (!split_i1 || workgroups <= 0) return 1;
    if (split_i1 > 1) return transforms < 1 ? 1 : (split_i1 < transforms ? split_i1 : transforms);   // (lab: a given number of parts)
    // the number of parts (1 .. 8, every part at least four transforms) that fills the launch's rounds of
    // resident workgroups best: 672 workgroups on 512 slots are 1.31 rounds - a third of the chip idles through
    // the second -, in three parts 2 016 workgroups are 3.94 rounds of a third the length (C1F: seven batched
    // orientations x three tile pairs x 32 column blocks).  Fewer parts win ties: every part parks the spectrum.
    int best = 1;
    double best_u = 0.0;
    for (int nz = 1; nz <= 8 && transforms / nz >= 4; ++nz) {
        const long long w = workgroups * nz, rounds = (w + capacity - 1) / capacity;
        const double u = (double)w / (double)(rounds * capacity);
        if (u > best_u + 0.03) { best_u = u; best = nz; }
    }
    return best;
}

// ---- the shape of a chunk's launches (fft_inverse_fold): pc tile pairs through the column pass (I1) and the row pass
// (I2), group by group; G templates of an orientation in the group, nb batched orientations ----

// float2 cells of a transform's line in LDS (fft_line, sc_fft.hip: tied to it by a static_assert there)
constexpr int fft_route_lds_line(int T) { return T + T / 16 + 8; }
// transforms of a group of G templates: in the paired-template chunk they ride in pairs
inline int fft_route_transforms(int G, bool pt) { return pt ? (G + 1) / 2 : G; }

// Tile pairs per column launch, and whether they are interleaved along x.  As many pairs as it takes to fill the chip
// once (one 2048-tile pair does; longer launches lost 6 % on the sustained C3 run); batched orientations: every job of
// the chunk in one launch - job ob * pc + q, the numbering the row kernel expects.  Wave-per-column kernel, one
// orientation: c.jil tile pairs per launch, INTERLEAVED along x (k_inv_cols_w8) - a launch of several pairs one after
// the other along y lost 6 % (the pairs' workgroups drift apart); interleaved, the 2 x i1_pairs workgroups that stream
// the same coefficient lines run together on one XCD.
struct FftColPairs {
    int pairs;                   // tile pairs per launch (the last launch of a chunk may hold fewer)
    bool interleaved;
};
inline FftColPairs fft_route_col_pairs(const FftChunkRoute& c, int Ty, int Tx, int nb, int pc) {
    if (c.jil > 1) return {pc < c.jil ? pc : c.jil, true};
    if (nb > 1) return {pc, false};
    const long long lds_c = 4LL * fft_route_lds_line(Ty) * 8 + (Ty <= 2048 ? 4LL * Ty * 8 : 0);   // (float2: 8 bytes)
    const long long per_cu = 160 * 1024 / lds_c;
    const int slots = 256 * (int)(per_cu > 1 ? per_cu : 1);
    const int fill = (slots + Tx / 8 - 1) / (Tx / 8);
    const int pairs = pc < fill ? pc : fill;
    return {pairs > 1 ? pairs : 1, false};
}

// The row pass folds at most SC_MAX_GROUP templates per launch (its scalar table, its 64-bit mask of transforms, the
// winner's byte): a batch of more - nb orientations of G templates each - goes through it in slices of whole
// orientations, in order; the running best lives in the record between launches, so the fold is the one of a single
// launch (and of no batching at all).  Slices of equal size: 8 orientations of 10 templates go 4 + 4, not 6 + 2 - a
// short last launch leaves the chip part empty.
// Where the dealt-out row pass applies (small grids: FFT_ROW_SPLIT) a launch carries up to 255 templates - the winner's
// byte - in shares of at most SC_MAX_GROUP transforms each; C1F's 7 batched orientations of 35 ages are then ONE
// row-pass launch of four shares at four waves per SIMD instead of seven launches of two.  (With near-tie flags on the
// route allows it from four templates per orientation only: on C5, one template per orientation, the split cost more
// in float64 pairs than it saved in the pass: 14.0 -> 17.3 ms; C1F 51.7 -> 46.6)
// How many shares: up to four (any number, not only powers of two) while the launch stays within ~4 300 waves - the
// four per SIMD the kernel's 128 registers allow and 5 % (measured at C1F, 1 044 single-wave rows: two shares 19.0 ms,
// three 13.8, four 13.5; option "split_fill" sets another bound).

// is a group of G templates dealt out at all
inline bool fft_route_row_split(const FftChunkRoute& c, int G) { return c.row == FFT_ROW_SPLIT && G >= c.split_min_g; }
// the most shares a row-pass launch of this group may have: rp_n row pairs of a tile hold valid outputs, a row
// workgroup is Tx / 512 waves (FFT_ROW_SPLIT: Tx is 512 or 1024)
inline int fft_route_nsplit_max(const FftChunkRoute& c, int Tx, int G, int rp_n, int pc) {
    if (!fft_route_row_split(c, G)) return 1;
    const long long row_wgs = (long long)rp_n * 2 * pc, cap_wg = c.split_waves / (Tx / 512);
    const long long by_fill = cap_wg / (row_wgs > 1 ? row_wgs : 1);
    const long long m = by_fill < c.split_max ? by_fill : c.split_max;
    return (int)(m > 1 ? m : 1);
}
// orientations per row-pass launch: the batch's nb in slices of equal size (paired orientations: all of them, they
// go to the row pass as ONE orientation of nb templates)
inline int fft_route_row_slice(const FftChunkRoute& c, int nb, int G, bool pt, int nsplit_max) {
    if (nb <= 1 || fft_route_xp(c.col)) return nb;
    const int by_byte = SC_MAX_GROUP * nsplit_max * (pt ? 2 : 1);
    const int cap_t = nsplit_max > 1 ? (by_byte < 255 ? by_byte : 255) : SC_MAX_GROUP;
    const int per = cap_t / (G > 1 ? G : 1), cap = per > 1 ? per : 1, nsl = (nb + cap - 1) / cap;
    return (nb + nsl - 1) / nsl;
}
// shares of ONE row-pass launch of ngl transforms (the slice's orientations x fft_route_transforms): every share at
// least four transforms, at most SC_MAX_GROUP - its 64-bit mask
inline int fft_route_nsplit(const FftChunkRoute& c, int G, int nsplit_max, int ngl) {
    if (!fft_route_row_split(c, G)) return 1;
    int ns = nsplit_max < ngl / 4 ? nsplit_max : ngl / 4;
    if (ns < 1) ns = 1;
    const int by_mask = (ngl + SC_MAX_GROUP - 1) / SC_MAX_GROUP;
    return ns > by_mask ? ns : by_mask;
}
// ... and what the kernel cannot take: more than four shares, or a share of more than SC_MAX_GROUP transforms.
// (tests/match_plan_check.cpp: no chunk sc_match_plan produces comes here, on any route and any number of tile pairs -
//  a slice holds at most 255 templates)
inline bool fft_route_nsplit_refused(const FftChunkRoute& c, int G, int ngl, int nsplit) {
    return fft_route_row_split(c, G) && (nsplit > 4 || (ngl + nsplit - 1) / nsplit > SC_MAX_GROUP);
}
