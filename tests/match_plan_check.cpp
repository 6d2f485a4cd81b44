// The search's launch plan (scarplet_amd/csrc/sc_match_plan.h) and the launch shapes of the FFT path's inverse passes
// (sc_fft_route.h) on the host: g++ -std=c++17 -fsanitize=address,undefined, a program of its own
// (tests/test_match_plan_host.py builds and runs it).
// match_plan_check print
//   stdout: the seeded random descriptor lists and their plans, for the restatement of tests/match_plan_reference.py.
//           Per case "case k", "in" with method, to_maps, ch, cw, oy, ox, dx, Ty, Tx, ntiles, group, batch_off, variant,
//           batch_templ, batch_fill, spectra and n, n lines "t" with kind, flags, pmin, pmax, qmin, qmax, masked, c, d,
//           cos_a, sin_a, cc, sc2, ss, then the plan: "runs" and "chunks" with a count and one line each (the fields in
//           the order of MatchRun and MatchChunk), the four per-template offsets, "max" with max_cells, max_dcells,
//           max_spans, nb_max, max_batch_templ, and "slots" with n_slots and slot_of.
// match_plan_check refusals
//   stdout: what sc_match_plan_check answers to six tile plans, one line each
// match_plan_check
//   properties of the plans of the same lists and of an exhaustive sweep of small regular searches (A orientations of
//   n templates each on every tile plan), none of which restates the rule; stdout: the counts, and how often a planned
//   chunk came to the row pass's refusal.
#include "../scarplet_amd/csrc/sc_match_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

static long long n_checked = 0, n_failed = 0, n_refused = 0, n_row_launches = 0;
static const char* where = "";
static long long where_k = 0;
static void fail(const char* what) {
    if (n_failed++ < 20) std::fprintf(stderr, "FAIL %s (%s %lld)\n", what, where, where_k);
}
#define CHECK(cond) do { ++n_checked; if (!(cond)) fail(#cond); } while (0)

struct Rng {
    unsigned long long s;
    unsigned long long next() {
        unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (unsigned long long)n); }
    template <class T> T pick(std::initializer_list<T> v) { return *(v.begin() + below((int)v.size())); }
};

struct Case {
    std::vector<sc_template> t;
    std::vector<unsigned char> masked;
    MatchPlanIn in;
};

static void set_plan_in(Case& c, int method, bool to_maps, int ch, int cw, int Ty, int Tx, int ntiles, int group) {
    std::memset(&c.in, 0, sizeof(c.in));
    c.in.method = method; c.in.to_maps = to_maps; c.in.ch = ch; c.in.cw = cw; c.in.dx = 1.0;
    c.in.route.Ty = Ty; c.in.route.Tx = Tx; c.in.route.ntiles = ntiles; c.in.route.parity = 1;
    c.in.route.nb = c.in.route.n = 1; c.in.route.group = group;
    c.in.route.i1_pairs = 2; c.in.route.split_i1 = 1; c.in.route.fuse_fwd = 1;      // the context's defaults
}
static void finish(Case& c) {
    c.in.t = c.t.data(); c.in.n = (int)c.t.size(); c.in.masked = c.masked.data();
}

// one template of orientation `o` (its id: equal ids are equal (cc, sc2, ss))
static sc_template templ(Rng& g, int o, int kind, int flags, bool symmetric, int oy, int ox) {
    sc_template s;
    std::memset(&s, 0, sizeof(s));
    s.kind = kind; s.flags = flags;
    s.cc = 0.25 * o; s.sc2 = 1.0 - 0.125 * o; s.ss = 1.0 - 0.25 * o;
    const int hy = 1 + g.below(40), hx = 1 + g.below(40);
    s.pmin = -hy; s.pmax = hy - (1 - oy); s.qmin = -hx; s.qmax = hx - (1 - ox);
    if (!symmetric) s.pmax += 1 + g.below(3);
    if (s.pmax < s.pmin) s.pmax = s.pmin;
    if (s.qmax < s.qmin) s.qmax = s.qmin;
    s.c = g.pick({0.5, 3.0, 8.0, 40.0}); s.d = g.pick({0.5, 3.0, 8.0, 40.0});
    const double ang[] = {0.0, 0.3, 0.7853981633974483, 1.2, 1.5707963267948966};
    const double a = ang[g.below(5)];
    s.cos_a = cos(a); s.sin_a = sin(a);
    s.window = kind == SC_KIND_WINDOW ? 0 : -1;
    return s;
}

static Case random_case(int k) {
    Rng g{0x5CA4B1E7ull * (unsigned long long)(k + 1)};
    Case c;
    const int sizes[] = {64, 128, 256, 512, 1024, 2048, 4096};
    const int method = k % 3 == 0 ? SC_METHOD_DIRECT : SC_METHOD_FFT;
    const bool to_maps = k % 17 == 5;
    const int ch = g.pick({80, 96, 300, 512, 1030, 2050, 5000}), cw = g.pick({80, 131, 512, 1031, 2061, 5000});
    set_plan_in(c, method, to_maps, ch, cw, sizes[2 + g.below(5)], g.below(4) ? sizes[3 + g.below(3)] : sizes[g.below(7)], 1 + g.below(9),
                g.pick({1, 8, 35, 64, 64, 64}));
    c.in.oy = g.below(2); c.in.ox = g.below(2);
    c.in.dx = g.pick({0.5, 1.0, 1.0, 2.0});
    c.in.route.batch_off = g.below(5) == 0;
    c.in.route.variant = g.below(3) ? 0 : g.pick({9, 10, 15, 17, 20});
    c.in.route.batch_templ = g.pick({0, 0, 0, 64, 100});
    c.in.route.batch_fill = g.pick({0, 0, 0, 512, 100000});
    c.in.spectra = g.below(3) == 0;
    if (to_maps) {
        c.t.push_back(templ(g, 0, g.below(3), 0, g.below(2), c.in.oy, c.in.ox));
        c.masked.push_back(c.t[0].kind == SC_KIND_WINDOW && g.below(2));
        finish(c);
        return c;
    }
    // orientations in sections: within a section one family and one run length, or - "mixed" - neither
    const int target = g.pick({1, 5, 20, 70, 70, 200, 200, SC_MAX_BATCH, 2 * SC_MAX_BATCH + 7, 3 * SC_MAX_BATCH + 1});
    int o = 0;
    while ((int)c.t.size() < target) {
        const int n_or = 1 + g.below(g.pick({2, 8, 40, 95}));
        const int n_per = g.pick({1, 1, 2, 3, 5, 10, 21, 22, 35, SC_MAX_GROUP, SC_MAX_GROUP + 1, 2 * SC_MAX_GROUP + 3});
        const bool mixed = g.below(5) == 0, sym = g.below(4) != 0;
        const int kind = g.below(3), flags = g.below(6) == 0 ? (g.below(2) ? SC_FLAG_ERR_XR_LE0 : SC_FLAG_ERR_XR_GE0) : 0;
        const bool masks = kind == SC_KIND_WINDOW && g.below(3) == 0;
        for (int a = 0; a < n_or; ++a, ++o) {
            const int n_here = mixed ? 1 + g.below(n_per) : n_per;
            // (an orientation now and then repeats the one before it, or an earlier one)
            const int oid = a > 0 && g.below(12) == 0 ? o - 1 : g.below(40) == 0 ? g.below(o + 1) : o;
            for (int j = 0; j < n_here; ++j) {
                const int kj = mixed && g.below(4) == 0 ? g.below(3) : kind;
                c.t.push_back(templ(g, oid, kj, mixed && g.below(8) == 0 ? SC_FLAG_ERR_XR_LE0 : flags, sym || (mixed && g.below(2)), c.in.oy, c.in.ox));
                c.masked.push_back(kj == SC_KIND_WINDOW && (masks || (mixed && g.below(6) == 0)));
            }
        }
    }
    finish(c);
    return c;
}

template <class T>
static void print(const char* name, const std::vector<T>& v) {
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

static void print_case(int k, const Case& c, const MatchPlan& p) {
    const MatchPlanIn& in = c.in;
    std::printf("case %d\nin %d %d %d %d %d %d %.17g %d %d %d %d %d %d %d %d %d %d\n", k, in.method, (int)in.to_maps, in.ch, in.cw, in.oy,
                in.ox, in.dx, in.route.Ty, in.route.Tx, in.route.ntiles, in.route.group, in.route.batch_off, in.route.variant,
                in.route.batch_templ, in.route.batch_fill, (int)in.spectra, in.n);
    for (int j = 0; j < in.n; ++j) {
        const sc_template& s = in.t[j];
        std::printf("t %d %d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", s.kind, s.flags, s.pmin, s.pmax, s.qmin, s.qmax,
                    (int)in.masked[j], s.c, s.d, s.cos_a, s.sin_a, s.cc, s.sc2, s.ss);
    }
    std::printf("runs %zu\n", p.runs.size());
    for (const MatchRun& r : p.runs) std::printf("%d %d %d %d %d\n", r.first, r.n, r.parity, (int)r.full, (int)r.long_runs);
    std::printf("chunks %zu\n", p.chunks.size());
    for (const MatchChunk& q : p.chunks)
        std::printf("%d %d %d %d %d %d %d %d %zu %d\n", q.first, q.n, q.nb, q.wh, q.ww, q.parity, (int)q.full, (int)q.long_runs, q.cells, q.run0);
    print("win_off", p.win_off);
    print("dwin_off", p.dwin_off);
    print("dpitch", p.dpitch);
    print("span_off", p.span_off);
    std::printf("max %zu %zu %zu %d %d\n", p.max_cells, p.max_dcells, p.max_spans, p.nb_max, p.max_batch_templ);
    std::printf("slots %d", p.n_slots);
    for (int s : p.slot_of) std::printf(" %d", s);
    std::printf("\n");
}

// the inverse passes of one planned chunk on one route: what fft_inverse_fold's loops come to
static void check_launch_shapes(const MatchPlanIn& in, const MatchChunk& q, FftRouteIn rin) {
    rin.parity = q.parity; rin.full_masks = q.full; rin.to_maps = in.to_maps; rin.nb = q.nb; rin.n = q.n;
    const FftRoute r = fft_route(rin);
    CHECK(r.msg != FFT_REFUSE_BATCH);
    if (r.err) return;
    const int np = (rin.ntiles + 1) / 2, np_main = r.pt ? np - 1 : np;
    for (int pt = 0; pt <= (r.pt ? 1 : 0); ++pt) {
        const FftChunkRoute& c = pt ? r.ptc : r.main;
        for (int pc = 1; pc <= (pt ? 1 : np_main); ++pc)
            for (int g0 = 0; g0 < q.n; g0 += rin.group) {
                const int G = std::min(rin.group, q.n - g0), ng = fft_route_transforms(G, pt != 0);
                const FftColPairs cp = fft_route_col_pairs(c, rin.Ty, rin.Tx, q.nb, pc);
                CHECK(cp.pairs >= 1 && cp.pairs <= pc);
                if (q.nb > 1) CHECK(cp.pairs == pc && !cp.interleaved);     // job ob * pc + q: the numbering the row kernel expects
                if (cp.interleaved) CHECK(c.col == FFT_COL_W8);
                for (int rp_n : {1, rin.Ty / 8, rin.Ty / 2}) {
                    const int nsplit_max = fft_route_nsplit_max(c, rin.Tx, G, rp_n, pc);
                    const int nbs = fft_route_row_slice(c, q.nb, G, pt != 0, nsplit_max);
                    CHECK(nsplit_max >= 1 && nsplit_max <= 4 && nbs >= 1 && nbs <= q.nb);
                    // (not held: slices that differ by at most one orientation.  ceil(nb / ceil(nb / cap)) leaves a short
                    //  last slice where the batch is a little over two slices: 7 orientations of 33 templates, two shares
                    //  allowed - 3 to a slice - go 3 + 3 + 1, not 3 + 2 + 2.  Same results; docs/history.md)
                    int sum = 0;
                    for (int b0 = 0; b0 < q.nb; b0 += nbs) {
                        const int nbc = std::min(nbs, q.nb - b0), ngl = nbc * ng;
                        sum += nbc;
                        CHECK(nbc * G <= 255);                              // the winner's byte
                        const int nsplit = fft_route_nsplit(c, G, nsplit_max, ngl);
                        ++n_row_launches;
                        if (fft_route_nsplit_refused(c, G, ngl, nsplit)) ++n_refused;
                        CHECK(nsplit >= 1 && nsplit <= 4 && (ngl + nsplit - 1) / nsplit <= SC_MAX_GROUP);
                        if (c.row != FFT_ROW_SPLIT) CHECK(nsplit == 1);
                    }
                    CHECK(sum == q.nb);
                }
            }
    }
}

static void check_plan(const Case& c, const MatchPlan& p, bool every_variant) {
    const MatchPlanIn& in = c.in;
    const bool fft = in.method == SC_METHOD_FFT;
    const int n = in.n;
    // the runs partition [0, n) in order: one orientation each, at most SC_MAX_GROUP templates
    int at = 0;
    for (const MatchRun& r : p.runs) {
        CHECK(r.first == at && r.n >= 1 && r.n <= SC_MAX_GROUP);
        for (int j = r.first; j < r.first + r.n && j < n; ++j) CHECK(sc_match_same_orientation(in.t[j], in.t[r.first]));
        at += r.n;
    }
    CHECK(at == n);
    // the chunks partition [0, n) in order, each nb consecutive runs of equal n, parity and mask kind
    at = 0;
    size_t run = 0, max_cells = 0, max_dcells = 0, max_spans = 0;
    int nb_max = 1, max_templ = 1;
    for (const MatchChunk& q : p.chunks) {
        CHECK(q.first == at && q.nb >= 1 && (size_t)q.run0 == run && run + q.nb <= p.runs.size());
        if (run + q.nb > p.runs.size()) return;
        for (int b = 0; b < q.nb; ++b) {
            const MatchRun& r = p.runs[run + b];
            CHECK(r.first == q.first + b * q.n && r.n == q.n && r.parity == q.parity && r.full == q.full);
            if (!fft) CHECK(r.long_runs == q.long_runs);
        }
        if (in.to_maps || (!fft && (in.route.batch_off || in.route.variant == 10))) CHECK(q.nb == 1);
        if (fft) CHECK(q.nb <= std::min(SC_MAX_ORIENT, SC_MAX_BATCH / q.n)); else CHECK(q.nb <= 32);
        // the windows of the chunk: offsets 4-aligned and disjoint, in each of the three buffers
        long long end = 0, dend = 0;
        int send = 0, wh = 0, ww = 0;
        for (int j = q.first; j < q.first + q.nb * q.n; ++j) {
            const int h = in.t[j].pmax - in.t[j].pmin + 1, w = in.t[j].qmax - in.t[j].qmin + 1;
            CHECK(p.win_off[j] % 4 == 0 && p.win_off[j] >= end);
            CHECK(p.dwin_off[j] % 4 == 0 && p.dwin_off[j] >= dend && p.dpitch[j] % 4 == 0 && p.dpitch[j] >= w && p.dpitch[j] < w + 4);
            CHECK(p.span_off[j] >= send);
            end = p.win_off[j] + (long long)h * w; dend = p.dwin_off[j] + (long long)h * p.dpitch[j]; send = p.span_off[j] + h;
            wh = std::max(wh, h); ww = std::max(ww, w);
        }
        CHECK(p.win_off[q.first] == 0 && p.dwin_off[q.first] == 0 && p.span_off[q.first] == 0);
        CHECK(q.wh == wh && q.ww == ww && (long long)q.cells >= end && (long long)q.cells < end + 4);
        max_cells = std::max(max_cells, q.cells); max_dcells = std::max(max_dcells, (size_t)dend);
        max_spans = std::max(max_spans, (size_t)send);
        nb_max = std::max(nb_max, q.nb); max_templ = std::max(max_templ, q.nb * q.n);
        at += q.nb * q.n; run += q.nb;
    }
    CHECK(at == n && run == p.runs.size());
    CHECK(p.max_cells == max_cells && p.max_dcells == max_dcells && p.max_spans == max_spans);
    CHECK(p.nb_max == nb_max && p.max_batch_templ == max_templ);
    if (fft) CHECK(p.max_batch_templ <= SC_MAX_BATCH);
    // kept spectra: a slot per distinct consecutive orientation, a batch in consecutive slots - or nothing is kept
    CHECK(p.slot_of.size() == p.runs.size());
    if (!(fft && !in.to_maps && in.spectra)) CHECK(p.n_slots == 0);
    if (p.n_slots > 0) {
        for (const MatchChunk& q : p.chunks)
            for (int b = 1; b < q.nb; ++b) CHECK(p.slot_of[q.run0 + b] == p.slot_of[q.run0] + b);
        CHECK(p.slot_of[0] == 0 && p.slot_of.back() == p.n_slots - 1);
        for (size_t r = 1; r < p.runs.size(); ++r) {
            const bool same = sc_match_same_orientation(in.t[p.runs[r].first], in.t[p.runs[r - 1].first]);
            CHECK(p.slot_of[r] == p.slot_of[r - 1] + (same ? 0 : 1));
        }
    }
    if (!fft) return;
    // every shape of chunk on every route: the options of the plan, and those the plan does not depend on
    // (variant 9 - the generic row kernel everywhere - changes what the plan batches: only as the plan's own)
    std::vector<int> variants(1, in.route.variant);
    if (every_variant) variants.insert(variants.end(), {0, 1, 2, 5, 6, 12, 15, 18, 19, 20});
    std::vector<const MatchChunk*> seen;
    for (const MatchChunk& q : p.chunks) {
        bool dup = false;
        for (const MatchChunk* s : seen) dup = dup || (s->nb == q.nb && s->n == q.n && s->parity == q.parity && s->full == q.full);
        if (dup) continue;
        seen.push_back(&q);
        for (int near = 0; near <= 1; ++near) for (int variant : variants) for (long long fill : {0LL, 64LL, 1000000LL})
        for (int sib = 0; sib <= (every_variant ? 1 : 0); ++sib) {
            FftRouteIn rin = in.route;
            rin.near = near; rin.variant = variant; rin.split_fill = fill; rin.sib = sib; rin.kept = p.n_slots > 0;
            check_launch_shapes(in, q, rin);
        }
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "refusals")) {
        // sc_match_plan_check: a 512 x 512 tile with 400 x 400 valid outputs over a 400 x 400 core, and what is wrong with it
        sc_plan p;
        std::memset(&p, 0, sizeof(p));
        p.method = SC_METHOD_FFT; p.Ty = p.Tx = 512; p.Vy = p.Vx = 400; p.nty = p.ntx = 1;
        auto say = [](const sc_plan& q, int ny, int nx, bool wrap, int ch, int cw) {
            const MatchPlanRefusal r = sc_match_plan_check(q, ny, nx, wrap, ch, cw);
            std::printf("%s\n", r.err ? r.msg : "ok");
        };
        say(p, 400, 400, true, 400, 400);
        sc_plan q = p; q.Vy = 0; q.circ_y = 1;                   // (the first refusal is the one answered)
        say(q, 400, 400, true, 400, 400);
        q = p; q.circ_y = 1;                                     // T != n
        say(q, 400, 400, true, 400, 400);
        q = p; q.circ_x = 1;                                     // T == n, but a block of a larger DEM
        say(q, 400, 512, false, 400, 400);
        say(p, 400, 400, true, 401, 400);
        q = p; q.method = SC_METHOD_DIRECT; q.Vy = 0;            // the real-space path has no tile plan
        say(q, 400, 400, true, 400, 400);
        return 0;
    }
    const bool printing = argc > 1 && !std::strcmp(argv[1], "print");
    const int n_random = 300;
    for (int k = 0; k < n_random; ++k) {
        const Case c = random_case(k);
        const MatchPlan p = sc_match_plan(c.in);
        where = "random case"; where_k = k;
        if (printing) print_case(k, c, p); else check_plan(c, p, true);
    }
    if (printing) return 0;
    // the sweep: A orientations of n templates each, on every tile plan of the fast row kernel and one of the generic
    Rng g{7};
    long long k = 0;
    for (int n_per : {1, 2, 3, 4, 5, 7, 10, 16, 21, 22, 25, 32, 33, 35, 64, 65}) for (int A = 1; A <= 70; ++A) {
        Case c;
        for (int a = 0; a < A; ++a)
            for (int j = 0; j < n_per; ++j) {
                c.t.push_back(templ(g, a, SC_KIND_SCARP, 0, true, 0, 0));
                c.masked.push_back(0);
            }
        for (int method : {SC_METHOD_FFT, SC_METHOD_DIRECT}) for (int Ty : {512, 2048}) for (int Tx : {256, 512, 1024, 2048})
        for (int ntiles : {1, 2, 3, 7}) for (int batch_templ : {0, 100}) {
            if (method == SC_METHOD_DIRECT && (Ty != 512 || Tx != 512 || ntiles > 2 || batch_templ)) continue;
            set_plan_in(c, method, false, method == SC_METHOD_DIRECT && ntiles == 2 ? 3000 : 500, 500, Ty, Tx, ntiles, std::min(n_per, SC_MAX_GROUP));
            c.in.route.batch_templ = batch_templ;
            c.in.spectra = A % 2;
            finish(c);
            where = "sweep"; where_k = k++;
            check_plan(c, sc_match_plan(c.in), false);
        }
    }
    std::printf("match_plan: %lld checks, %lld failed; %lld row-pass launches, %lld refused\n", n_checked, n_failed, n_row_launches, n_refused);
    return n_failed ? 1 : 0;
}
