// Invariants of the real-space path's route (scarplet_amd/csrc/sc_direct_route.h), enumerated on the host:
// g++ -std=c++17 -fsanitize=address,undefined, a program of its own (tests/test_direct_route_host.py builds and runs it).
// Without arguments it sweeps core extents, window boxes, long_runs and the variants and checks properties of what the
// kernels are instantiated for and of what the LDS holds.  With the argument "cases" it answers queries on stdin
// (tests/direct_classes.py writes them):
//   L <a> <b> <uploaded> <c> <d> <cos> <sin> <dx>                         -> L <a> <b> <long_runs>
//   R <launch> <ch> <cw> <wh_max> <ww_max> <long_runs> <variant> <wh> <ww>
//       -> R <launch> <NB> <RW> <share> <w4> <lds_floats> <batch_want> <slab_rows> <slabs> <narrow>
// (slab rows and slabs: of a template of wh x ww in that launch; narrow: the DEM has fewer columns than the slab)
#include "../scarplet_amd/csrc/sc_direct_route.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

static long long n_checked = 0, n_failed = 0;
static int cur[6];
static void fail(const char* what) {
    if (n_failed++ < 20)
        std::fprintf(stderr, "FAIL %s: ch %d cw %d wh %d ww %d long_runs %d variant %d\n", what, cur[0], cur[1], cur[2], cur[3],
                     cur[4], cur[5]);
}
#define CHECK(cond) do { ++n_checked; if (!(cond)) fail(#cond); } while (0)

static void check(int ch, int cw, int wh, int ww, bool lr, int variant) {
    const int c[6] = {ch, cw, wh, ww, lr, variant};
    std::memcpy(cur, c, sizeof(c));
    const DirectRoute r = direct_route(ch, cw, wh, ww, lr, variant);
    const int P = direct_pad4(ww);
    // one of the eight instantiations
    CHECK((r.NB == 1 && (r.RW == 1 || r.RW == 2)) || (r.NB == 2 && r.RW == 2));
    if (r.w4) CHECK(r.NB == 1 && r.RW == 2);
    // the slab the launch asks for exists, and holds a template row for every output row of the patch
    CHECK(r.lds_floats >= 1 && r.lds_floats <= DR2_LDS_FLOATS);
    const long long lwp = 256 * r.NB + P, ty = DR2_WAVES * r.RW;
    const bool fits256 = (long long)(256 + P) * 16 <= DR2_LDS_FLOATS;         // (direct_window_fits: sc_match refuses the rest)
    if (fits256) CHECK(lwp * ty <= r.lds_floats);
    const int na = direct_slab_rows(r, P, wh);
    CHECK(na >= 1 && na <= wh);
    if (fits256) CHECK(lwp * (ty + na - 1) <= r.lds_floats);
    CHECK(direct_slabs(r, P, wh) >= 1 && (long long)direct_slabs(r, P, wh) * na >= wh && (long long)(direct_slabs(r, P, wh) - 1) * na < wh);
    // a narrower template of the same launch is staged in at most as many slabs
    if (ww > 4) CHECK(direct_slabs(r, direct_pad4(ww - 4), wh) <= direct_slabs(r, P, wh));
    // W4: the tallest template in ONE slab, of at most half the LDS (two workgroups per CU); never under variant 19
    if (r.w4) CHECK(na >= wh && direct_slabs(r, P, wh) == 1 && r.lds_floats <= DR2_LDS_FLOATS / 2 && variant != 19);
    if (!r.w4) CHECK(r.lds_floats == DR2_LDS_FLOATS);
    // the 512 patch only where its slab fits, and never under variant 16
    if (r.NB == 2) CHECK((long long)(512 + P) * 16 <= DR2_LDS_FLOATS && variant != 16);
    // the shared form: long runs, not variant 11
    CHECK(r.share == (lr && variant != 11));
    // the patch fills the chip: a two-row class has at least 256 workgroups of 256 x 16, the 512 patch 512 of its own
    if (r.RW == 2) CHECK(direct_wgs(ch, cw, 256, 16) >= 256);
    if (r.NB == 2) CHECK(direct_wgs(ch, cw, 512, 16) >= 512);
    if (direct_wgs(ch, cw, 256, 16) < 256) CHECK(r.NB == 1 && r.RW == 1 && !r.w4);
    // ... and such a DEM is never batched with 512 patches (a batch is for DEMs of at most 1024 patches of 256 x 8)
    const int want = direct_batch_want(ch, cw);
    CHECK(want == 1 || want == 32);
    if (r.NB == 2) CHECK(want == 1);
    if (r.RW == 1) CHECK(want == 32);
    // the class does not depend on long_runs or variant 11, nor the slab
    const DirectRoute q = direct_route(ch, cw, wh, ww, !lr, variant == 11 ? 0 : variant);
    CHECK(q.NB == r.NB && q.RW == r.RW && q.w4 == r.w4 && q.lds_floats == r.lds_floats);
}

static int cases() {
    char line[512];
    while (std::fgets(line, sizeof(line), stdin)) {
        int a, b, up, ch, cw, whm, wwm, lr, variant, wh, ww;
        double c, d, ca, sa, dx;
        if (std::sscanf(line, "L %d %d %d %lf %lf %lf %lf %lf", &a, &b, &up, &c, &d, &ca, &sa, &dx) == 8) {
            std::printf("L %d %d %d\n", a, b, (int)direct_long_runs(up != 0, c, d, ca, sa, dx));
        } else if (std::sscanf(line, "R %d %d %d %d %d %d %d %d %d", &a, &ch, &cw, &whm, &wwm, &lr, &variant, &wh, &ww) == 9) {
            if (variant == 10) { std::fprintf(stderr, "variant 10 is the box kernel's: no route\n"); return 2; }
            const DirectRoute r = direct_route(ch, cw, whm, wwm, lr != 0, variant);
            const int P = direct_pad4(ww);
            std::printf("R %d %d %d %d %d %d %d %d %d %d\n", a, r.NB, r.RW, (int)r.share, (int)r.w4, r.lds_floats,
                        direct_batch_want(ch, cw), direct_slab_rows(r, P, wh), direct_slabs(r, P, wh), (int)(cw < 256 * r.NB + P));
        } else {
            std::fprintf(stderr, "bad query: %s", line);
            return 2;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "cases")) return cases();
    if (argc > 1 && !std::strcmp(argv[1], "share_min")) { std::printf("%d\n", SC_DR_SHARE_MIN); return 0; }
    const int ext[] = {1, 7, 8, 9, 16, 131, 255, 256, 257, 512, 1030, 1501, 2061, 4091, 8201, 10000, 40000};
    const int box[] = {1, 3, 4, 5, 16, 41, 48, 49, 101, 189, 500, 1000, 2016, 2017, 2275};
    for (int ch : ext) for (int cw : ext) for (int wh : box) for (int ww : box) for (int lr = 0; lr <= 1; ++lr)
    for (int variant : {0, 11, 16, 19}) check(ch, cw, wh, ww, lr != 0, variant);
    // the long-run predicate: uploaded windows are long; a built-in rectangle by its shorter chord along x
    CHECK(direct_long_runs(true, 0, 0, 1, 0, 1));
    CHECK(direct_long_runs(false, 8.1, 100, 1, 0, 1) && !direct_long_runs(false, 7.9, 100, 1, 0, 1));
    CHECK(direct_long_runs(false, 100, 8.1, 0, 1, 1) && !direct_long_runs(false, 100, 7.9, 0, 1, 1));
    CHECK(!direct_long_runs(false, 8.1, 100, 1, 0, 2) && direct_long_runs(false, 8.1, 100, 1, 0, -0.5));       // (taps, not metres)
    std::printf("direct_route: %lld checks, %lld failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
