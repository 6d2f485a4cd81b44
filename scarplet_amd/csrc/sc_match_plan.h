// The search's launch plan: how a list of templates becomes launches, decided in ONE place.
//
// sc_match_plan() is a pure function of the descriptors, the core, the tile plan and the options - nothing of HIP, so
// that a host compiler can build it alone (tests/match_plan_check.cpp prints it and enumerates its properties under
// AddressSanitizer / UBSan).  match_impl (sc_api.hip) validates, asks it, copies the offsets into the device's template
// table and loops over the chunks: it decides no run, batch, offset or slot for itself.
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/scarplet_hip.h"      // sc_template, sc_plan
#include "sc_fft_route.h"
#include "sc_direct_route.h"

struct MatchPlanIn {
    const sc_template* t;        // the descriptors, orientation-major
    int n;
    const unsigned char* masked; // per template: its window slot carries per-cell masks (nullptr: none does)
    int method;                  // SC_METHOD_DIRECT / SC_METHOD_FFT
    bool to_maps;                // sc_match_template: one template, its maps
    int ch, cw;                  // the core's extent
    int oy, ox;                  // ny % 2, nx % 2
    double dx;
    FftRouteIn route;            // the tile plan (Ty, Tx, ntiles), `group`, and the options that bear on the plan:
                                 // batch_off, variant, batch_templ, batch_fill (nb, n, parity: not read)
    bool spectra;                // option "spectra_mb" > 0: curvature spectra are kept across searches
};

// An orientation run: consecutive templates with equal (cc, sc2, ss) share one curvature plane, at most SC_MAX_GROUP
// of them per run.
struct MatchRun {
    int first, n;
    int parity;                  // flip symmetry of the run's built-in templates (k_split_templ_sym): 0 none, 1 odd, 2 even
    bool full;                   // some template has an error half-plane or per-cell masks: every cell is written
    bool long_runs;              // real-space path: some template has window rows of SC_DR_SHARE_MIN taps or more
};
// A chunk: one run, or nb consecutive runs of equal length, parity and mask kind (real space: and equal long_runs)
// sent through every launch together (sc_fft.hip, "Orientation batching"; launch_direct)
struct MatchChunk {
    int first, n, nb;            // templates [first, first + nb * n)
    int wh, ww;                  // the largest window box
    int parity;
    bool full, long_runs;
    size_t cells;                // of win_w / win_m the chunk's windows take
    int run0;                    // its first run
};
struct MatchPlan {
    std::vector<MatchRun> runs;
    std::vector<MatchChunk> chunks;
    // per template, offsets into the per-chunk window buffers (TemplDev): the window in win_w / win_m; real-space
    // path: the reversed rows padded to groups of four taps in dwin (k_direct_prep), their pitch, the first entry of
    // the row-span table
    std::vector<long long> win_off, dwin_off;
    std::vector<int> dpitch, span_off;
    size_t max_cells, max_dcells, max_spans;     // the most a chunk needs of win_w / win_m, of dwin, of spans
    int nb_max, max_batch_templ;                 // the most orientations, and templates, a chunk holds
    // Spectra kept across searches: slot of run r = its orientation's index among the search's distinct consecutive
    // orientations; n_slots 0: nothing kept
    std::vector<int> slot_of;
    int n_slots;
};

// The tile plan of an FFT search against the DEM (ny x nx, `wrap`: the block is the whole periodic DEM) and the core
struct MatchPlanRefusal { int err; const char* msg; };
inline MatchPlanRefusal sc_match_plan_check(const sc_plan& p, int ny, int nx, bool wrap, int ch, int cw) {
    if (p.method != SC_METHOD_FFT) return {SC_OK, nullptr};
    if (p.nty < 1 || p.ntx < 1 || p.Vy < 1 || p.Vx < 1) return {SC_ERR_INVALID, "bad tile plan"};
    if ((p.circ_y && (p.Ty != ny || !wrap || p.nty != 1)) || (p.circ_x && (p.Tx != nx || !wrap || p.ntx != 1)))
        return {SC_ERR_INVALID, "circular axis needs T == n and the whole DEM"};
    if ((long long)p.nty * p.Vy < ch || (long long)p.ntx * p.Vx < cw) return {SC_ERR_INVALID, "tiles do not cover the core"};
    return {SC_OK, nullptr};
}

inline bool sc_match_same_orientation(const sc_template& a, const sc_template& b) {
    return a.cc == b.cc && a.sc2 == b.sc2 && a.ss == b.ss;
}

inline MatchPlan sc_match_plan(const MatchPlanIn& in) {
    MatchPlan p{};
    const sc_template* t = in.t;
    const int n = in.n;
    const bool fft = in.method == SC_METHOD_FFT;
    for (int i = 0; i < n;) {
        int j = i, parity = -1;
        bool full = false, long_runs = false;
        for (; j < n && j - i < SC_MAX_GROUP && sc_match_same_orientation(t[j], t[i]); ++j) {
            const sc_template& s = t[j];
            // the same parity for the whole run, and support boxes that map onto themselves
            int pj = s.kind == SC_KIND_SCARP ? 1 : (s.kind == SC_KIND_RICKER ? 2 : 0);
            if (s.pmin + s.pmax != -(1 - in.oy) || s.qmin + s.qmax != -(1 - in.ox)) pj = 0;
            parity = (parity == -1 || parity == pj) ? pj : 0;
            full |= (s.flags & (SC_FLAG_ERR_XR_LE0 | SC_FLAG_ERR_XR_GE0)) != 0 || (in.masked && in.masked[j]);
            // (direct_long_runs, sc_direct_route.h: decides the kernel form of the run's launch - per RUN, so that a
            //  template's sums do not depend on what it is batched with)
            long_runs = long_runs || direct_long_runs(s.kind == SC_KIND_WINDOW, s.c, s.d, s.cos_a, s.sin_a, in.dx);
        }
        p.runs.push_back({i, j - i, parity < 0 ? 0 : parity, full, long_runs});
        i = j;
    }
    p.win_off.assign(n, 0); p.dwin_off.assign(n, 0); p.dpitch.assign(n, 0); p.span_off.assign(n, 0);
    p.nb_max = p.max_batch_templ = 1;
    const std::vector<MatchRun>& runs = p.runs;
    for (size_t r = 0; r < runs.size();) {
        const MatchRun& r0 = runs[r];
        int nb = 1;
        if ((fft || (!in.route.batch_off && in.route.variant != 10)) && !in.to_maps) {
            // `want` fills the chip: fft_route_batch; real space: small DEMs fold up to 32 orientations per launch
            FftRouteIn q = in.route;
            q.n = r0.n;
            const int want = fft ? fft_route_batch(q) : direct_batch_want(in.ch, in.cw);
            // what one launch sequence can hold: SC_MAX_BATCH templates, SC_MAX_ORIENT curvature planes - the row pass
            // takes them in slices of whole orientations (fft_route_row_slice)
            const int by_templ = SC_MAX_BATCH / (r0.n > 1 ? r0.n : 1);
            const int hard = fft ? (by_templ < SC_MAX_ORIENT ? by_templ : SC_MAX_ORIENT) : 32;
            // compatible runs ahead - counted beyond what one launch can hold, up to two full batches: whether a
            // remainder rides along or the rest is split evenly is decided on what is really left (capped at `hard`, 91
            // orientations of ten templates went six at a time as 3 + 3 instead of 4 + 4 + ...)
            const int look = hard > 2 * want + 1 ? hard : 2 * want + 1;
            int avail = 1;
            while (avail < look && r + avail < runs.size() && runs[r + avail].n == r0.n &&
                   runs[r + avail].parity == r0.parity && runs[r + avail].full == r0.full &&
                   (fft || runs[r + avail].long_runs == r0.long_runs))
                ++avail;
            // a tail of a few orientations costs a whole launch sequence of its own (C1: 35 orientations were 32 + 3),
            // so a remainder up to a quarter of `want` rides along and a larger one is split evenly
            if (want <= 1) nb = 1;
            else if (avail <= want + want / 4) nb = avail;
            else if (avail < 2 * want) nb = (avail + 1) / 2;
            else nb = want;
            if (nb > hard) nb = hard;
        }
        size_t off = 0, doff = 0;
        int wh = 0, ww = 0, soff = 0;
        for (int j = r0.first; j < r0.first + nb * r0.n; ++j) {
            const int h = t[j].pmax - t[j].pmin + 1, w = t[j].qmax - t[j].qmin + 1;
            p.win_off[j] = (long long)off;
            off = (off + (size_t)h * w + 3) & ~(size_t)3;
            if (h > wh) wh = h;
            if (w > ww) ww = w;
            p.dpitch[j] = direct_pad4(w);
            p.dwin_off[j] = (long long)doff;
            p.span_off[j] = soff;
            doff += (size_t)h * p.dpitch[j];
            soff += h;
        }
        p.chunks.push_back({r0.first, r0.n, nb, wh, ww, r0.parity, r0.full, r0.long_runs, off, (int)r});
        if (off > p.max_cells) p.max_cells = off;
        if (doff > p.max_dcells) p.max_dcells = doff;
        if ((size_t)soff > p.max_spans) p.max_spans = (size_t)soff;
        if (nb > p.nb_max) p.nb_max = nb;
        if (nb * r0.n > p.max_batch_templ) p.max_batch_templ = nb * r0.n;
        r += nb;
    }
    p.slot_of.assign(runs.size(), 0);
    if (fft && !in.to_maps && in.spectra) {
        for (size_t r = 0; r < runs.size(); ++r) {
            const bool same = r > 0 && sc_match_same_orientation(t[runs[r].first], t[runs[r - 1].first]);
            p.slot_of[r] = same ? p.slot_of[r - 1] : p.n_slots++;
        }
        // a batch must sit in consecutive slots (an orientation twice in a batch: nothing is kept)
        for (const MatchChunk& c : p.chunks)
            for (int b = 1; b < c.nb; ++b)
                if (p.slot_of[c.run0 + b] != p.slot_of[c.run0] + b) p.n_slots = 0;
    }
    return p;
}
