// Invariants of the FFT path's route (scarplet_amd/csrc/sc_fft_route.h), enumerated on the host:
// g++ -std=c++17 -fsanitize=address,undefined, a program of its own (tests/test_fft_route_host.py builds and runs it).
// Nothing here restates the route's conditions: every check is a property of what the kernels are instantiated
// for (sc_fft.hip: the launchers' size lists), of what Matcher.can_flag_near_ties promises
// in Python, or of a shape DESIGN.md names.
#include "../scarplet_amd/csrc/sc_fft_route.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

static long long n_checked = 0, n_failed = 0;
static FftRouteIn cur;
static void fail(const char* what) {
    if (n_failed++ < 20)
        std::fprintf(stderr, "FAIL %s: Ty %d Tx %d tiles %d parity %d masks %d maps %d near %d nb %d n %d group %d kept %d variant %d\n",
                     what, cur.Ty, cur.Tx, cur.ntiles, cur.parity, cur.full_masks, cur.to_maps, cur.near, cur.nb, cur.n,
                     cur.group, cur.kept, cur.variant);
}
#define CHECK(cond) do { ++n_checked; if (!(cond)) fail(#cond); } while (0)

static bool in3(int T) { return T == 512 || T == 1024 || T == 2048; }
static bool paired_orient(FftColKernel k) { return k == FFT_COL_SYMX_XP || k == FFT_COL_H2_XP; }

// a kernel is named only at sizes, and in the chunk, it is instantiated for
static void check_chunk(const FftRouteIn& in, const FftRoute& r, const FftChunkRoute& c, bool pt) {
    const int Ty = in.Ty, Tx = in.Tx;
    switch (c.col) {
        case FFT_COL_W8: CHECK(Ty == 1024 || Ty == 2048); break;
        case FFT_COL_W4: CHECK(Ty == 2048 && pt); break;
        case FFT_COL_H2: CHECK(Ty == 512); break;
        case FFT_COL_H2_XP:
        case FFT_COL_SYMX_XP: CHECK(Ty == 512 && pt); break;
        case FFT_COL_SYMX: CHECK(in3(Ty)); break;
        case FFT_COL_SYM: CHECK(Ty <= 2048 && in.parity != 0); break;
        case FFT_COL_GENERIC: break;
    }
    if (in.parity == 0 || Ty == 4096) CHECK(c.col == FFT_COL_GENERIC);
    if (c.col != FFT_COL_GENERIC) CHECK(in.parity != 0);         // the real coefficients exist for symmetric templates only
    if (c.row == FFT_ROW_FAST || c.row == FFT_ROW_NEAR) CHECK(in3(Tx));
    if (c.row == FFT_ROW_SPLIT) {
        CHECK((Tx == 512 || Tx == 1024) && !in.full_masks && !in.to_maps);
        CHECK(c.split_max >= 1 && c.split_max <= 4 && c.split_min_g >= 1 && c.split_waves > 0);
    }
    if (pt) CHECK(c.row != FFT_ROW_GENERIC);
    // interleaved tile pairs are k_inv_cols_w8's, one orientation per launch
    CHECK(c.jil >= 1);
    if (c.jil > 1) CHECK(c.col == FFT_COL_W8 && in.nb == 1);
    // the kernels that transform the curvature columns themselves
    if (r.fwd) CHECK(c.col == FFT_COL_W8 || c.col == FFT_COL_W4);
    // near-tie flags (maps hold one template: there is no argmax to flag, and the route does not flag)
    if (in.near && !in.to_maps) CHECK(r.near && (c.row == FFT_ROW_NEAR || c.row == FFT_ROW_SPLIT));
    if (!in.near || in.to_maps) CHECK(!r.near && c.row != FFT_ROW_NEAR);
    if (in.to_maps || in.full_masks) CHECK(c.row == FFT_ROW_GENERIC || c.row == FFT_ROW_FAST);
    // the launch shapes, for any number of tile pairs in the hand-off: tile pairs per column launch, the most shares and
    // the slice of a row-pass launch, the shares of a launch of any number of transforms
    // (on the inputs that name a chunk's kernels: not over kept spectra, the fused forward and the group again)
    const int v = in.variant;
    if (in.kept || !in.fuse_fwd || in.group != 64 || !(v == 0 || v == 9 || v == 15 || v == 19 || v == 20)) return;
    for (int pc : {1, 2, 5}) {
        const FftColPairs cp = fft_route_col_pairs(c, Ty, Tx, in.nb, pc);
        CHECK(cp.pairs >= 1 && cp.pairs <= pc);
        if (cp.interleaved) CHECK(c.col == FFT_COL_W8 && cp.pairs <= c.jil);
        if (in.nb > 1) CHECK(cp.pairs == pc && !cp.interleaved);           // every job of the batch in one launch
        for (int G : {1, 3, 4, in.n}) for (int rp_n : {1, Ty / 2}) {
            const bool split = fft_route_row_split(c, G);
            if (split) CHECK(c.row == FFT_ROW_SPLIT);
            const int most = fft_route_nsplit_max(c, Tx, G, rp_n, pc);
            CHECK(most >= 1 && most <= (split ? c.split_max : 1));
            const int nbs = fft_route_row_slice(c, in.nb, G, pt, most);
            CHECK(nbs >= 1 && nbs <= in.nb);
            if (paired_orient(c.col)) CHECK(nbs == in.nb);                 // (to the row pass ONE orientation of nb templates)
            else if (in.nb > 1) CHECK(nbs == 1 || nbs * G <= (most > 1 ? 255 : SC_MAX_GROUP));
            for (int ngl : {1, 3, 4, 7, 8, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300}) {
                const int ns = fft_route_nsplit(c, G, most, ngl);
                CHECK(ns >= 1 && (split || ns == 1));
                if (ns > 1 && ns <= most) CHECK(ngl / ns >= 4);            // a share of fewer than four transforms: only the mask's doing
                CHECK(fft_route_nsplit_refused(c, G, ngl, ns) == (split && ngl > 4 * SC_MAX_GROUP));
                if (!fft_route_nsplit_refused(c, G, ngl, ns) && split) CHECK((ngl + ns - 1) / ns <= SC_MAX_GROUP && ns <= 4);
            }
        }
    }
}

static void check(const FftRouteIn& in) {
    cur = in;
    const FftRoute r = fft_route(in);
    const bool def = in.variant == 0;
    // refusals: the three of fft_inverse_fold, in its order; nothing else
    CHECK(r.err == SC_OK || r.msg == FFT_REFUSE_BATCH || r.msg == FFT_REFUSE_NEAR);       // (every size here is supported)
    CHECK((r.err == SC_OK) == (r.msg == nullptr));
    // batching: what fft_route_batch grants is not refused
    if (in.nb > 1 && fft_route_batch(in) >= in.nb) CHECK(r.msg != FFT_REFUSE_BATCH);
    // near-tie flags: refused exactly where Matcher.can_flag_near_ties says no (core.py)
    if (in.near && !in.to_maps && r.msg != FFT_REFUSE_BATCH) {
        const bool cannot = !in3(in.Tx) || in.variant == 9 || in.full_masks;
        CHECK((r.msg == FFT_REFUSE_NEAR) == cannot);
    } else {
        CHECK(r.msg != FFT_REFUSE_NEAR);
    }
    // the prepare-time question does not depend on the chunk
    FftRouteIn q = in;
    q.parity = 1; q.nb = q.n = q.group = 1; q.full_masks = q.to_maps = q.near = false;
    const FftRoute rq = fft_route(q);
    CHECK(rq.err == SC_OK && rq.fused == r.fused);
    if (in.kept || !in.fuse_fwd) CHECK(!r.fused);
    if (r.err) return;
    check_chunk(in, r, r.main, false);
    // the paired-template chunk: a non-zero parity, a fast row kernel, an odd tile count, variant != 5
    if (r.pt) CHECK(in.parity != 0 && r.main.row != FFT_ROW_GENERIC && (in.ntiles & 1) && in.variant != 5);
    if (r.pt) check_chunk(in, r, r.ptc, true);
    CHECK(!paired_orient(r.main.col));
    // the fused forward: every chunk transforms the parked rows itself or asks for k_fwd_cols first
    CHECK(!(r.fwd && r.cols_first));
    if (r.fused) CHECK(r.fwd || r.cols_first); else CHECK(!r.fwd && !r.cols_first);
    if (def && in.fuse_fwd && !in.kept && in.parity != 0 && !in.to_maps && (in.Ty == 1024 || in.Ty == 2048) && in.Tx % 128 == 0)
        CHECK(r.fused && r.fwd && !r.cols_first);                // k_fwd_cols is not in the step
    // the shapes DESIGN.md names, default options
    if (def && in.parity != 0) {
        if (in.Ty == 2048 && in.Tx == 2048) {
            CHECK(r.main.col == FFT_COL_W8 && r.main.row != FFT_ROW_GENERIC);
            CHECK(r.main.row == (in.near && !in.to_maps ? FFT_ROW_NEAR : FFT_ROW_FAST));
            if (in.ntiles & 1) CHECK(r.pt && r.ptc.col == FFT_COL_W4);
        }
        if (in.Ty == 1024 && r.pt) CHECK(r.ptc.col == FFT_COL_W8);
        if (in.Ty == 512 && in.Tx % 256 == 0) CHECK(r.main.col == FFT_COL_H2);
    }
    if (in.parity != 0 && in.Ty == 512 && in.n == 1 && in.nb >= 2 && r.pt && !in.to_maps && in.Tx % 256 == 0) {
        if (def) CHECK(r.ptc.col == FFT_COL_SYMX_XP);
        if (in.variant == 19) CHECK(r.ptc.col == FFT_COL_H2_XP);
    }
}

int main() {
    const int sizes[] = {64, 128, 256, 512, 1024, 2048, 4096};
    FftRouteIn in;
    std::memset(&in, 0, sizeof(in));
    in.i1_pairs = 2; in.split_i1 = 1;                            // the context's defaults (sc_internal.h)
    for (int Ty : sizes) for (int Tx : sizes) for (int parity = 0; parity <= 2; ++parity)
    for (int ntiles = 1; ntiles <= 3; ++ntiles) for (int masks = 0; masks <= 1; ++masks) for (int maps = 0; maps <= 1; ++maps)
    for (int near = 0; near <= 1; ++near) for (int nb : {1, 4}) for (int n : {1, 10}) for (int group : {8, 64})
    for (int kept = 0; kept <= 1; ++kept) for (int fuse = 0; fuse <= 1; ++fuse) for (int variant = 0; variant <= 20; ++variant) {
        in.Ty = Ty; in.Tx = Tx; in.parity = parity; in.ntiles = ntiles; in.full_masks = masks; in.to_maps = maps;
        in.near = near; in.nb = nb; in.n = n; in.group = group; in.kept = kept; in.fuse_fwd = fuse; in.variant = variant;
        check(in);
    }
    // unsupported sizes are refused as such, whatever else is asked
    in.variant = 0;
    for (int T : {0, 32, 96, 8192}) {
        in.Ty = T; in.Tx = 512; cur = in;
        CHECK(fft_route(in).err == SC_ERR_UNSUPPORTED && fft_route(in).msg == FFT_REFUSE_SIZE);
        in.Ty = 512; in.Tx = T; cur = in;
        CHECK(fft_route(in).err == SC_ERR_UNSUPPORTED && fft_route(in).msg == FFT_REFUSE_SIZE);
    }
    // parts of an under-filled column pass: 1 .. 8, every part at least four transforms; option off: 1
    for (long long wg = 1; wg <= 4096; wg += 37) for (int tr = 1; tr <= 70; ++tr) {
        const int nz = fft_route_parts(1, wg, 512, tr);
        CHECK(nz >= 1 && nz <= 8 && (nz == 1 || tr / nz >= 4));
        CHECK(fft_route_parts(0, wg, 512, tr) == 1);
    }
    std::printf("fft_route: %lld checks, %lld failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
