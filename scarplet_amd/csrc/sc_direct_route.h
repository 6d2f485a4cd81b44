// The real-space path's route: which instantiation of k_direct2 a launch takes, how many orientations ride in it and in
// how many slabs a template is staged, decided in ONE place.
//
// Pure functions of the core's extent, the launch's window box and the options - nothing of HIP, so that a host compiler
// can build them alone (tests/direct_route_check.cpp enumerates them under AddressSanitizer / UBSan).  launch_direct
// (sc_kernels.hip) and sc_match_plan (sc_match_plan.h: the batch and the long-run predicate) ask them and decide no
// patch, no slab and no batch for themselves.
#pragma once
#include <math.h>

#define DR2_LDS_FLOATS (39 * 1024 + 512)        // 158 KB
#define DR2_WAVES 8
#ifndef SC_DR_SHARE_MIN
#define SC_DR_SHARE_MIN 16    // shortest hole-free run (taps) whose T3 takes the shared form (8, the least the end-cell pieces allow, is slower:
                              // 0.26 against 0.19 ms at 46 taps, 0.56 against 0.50 at 294 - profiles/r06_crossover.txt)
#endif

// k_direct2<NB, RW, share, w4>: a patch of 256 NB columns x DR2_WAVES RW rows per workgroup
struct DirectRoute {
    int NB, RW;
    bool share;                  // the shared form of T3 on hole-free runs of SC_DR_SHARE_MIN taps or more
    bool w4;                     // built for four waves per SIMD: a slab of the launch's own size, two workgroups per CU
    int lds_floats;              // the slab the launch is given
};

inline int direct_pad4(int ww) { return (ww + 3) & ~3; }
// workgroups of a txw x ty patch over a core of ch x cw cells
inline long long direct_wgs(int ch, int cw, int txw, int ty) {
    return (long long)((cw + txw - 1) / txw) * ((ch + ty - 1) / ty);
}
// (the 512-wide patch needs a slab of 512 + the padded window width cells x 16 rows)
inline bool direct_fits512(int ww_max) { return (long long)(512 + direct_pad4(ww_max)) * 16 <= DR2_LDS_FLOATS; }

// patch: 512 x 16 cells where that still gives every CU a workgroup, else 256 x 16, else 256 x 8.
// The slab: all of the LDS (one workgroup per CU) unless the patch selection gives the launch a smaller one.  Its size
// decides only how many template rows are staged at a time, not the order of any sum
// (tests/test_gpu_direct_classes.py: the records of two classes are the same bits).
// ch x cw: the core; wh_max x ww_max: the launch's largest window box; `variant`: the option (10, the box kernel, is
// launch_direct_box's and never comes here).
inline DirectRoute direct_route(int ch, int cw, int wh_max, int ww_max, bool long_runs, int variant) {
    DirectRoute r;
    // (variant 11: T3 in the weighted form on every row; long_runs: some template of the launch has
    //  rows of 16 taps or more - the shared form's kernel carries more registers, thin windows are
    //  10 % faster on the plain one)
    r.share = variant != 11 && long_runs;
    r.w4 = false;
    r.lds_floats = DR2_LDS_FLOATS;
    // (round 6) windows whose 256 x 16 slab fits half the LDS in one piece - up to about a thousand taps - take that patch
    // with a slab of their own size: 128 registers and half the LDS are two workgroups per CU, four waves per SIMD, and the
    // kernel is bound by instruction issue there (-4 .. -25 % against the 512 x 16 patch at two waves per SIMD,
    // profiles/r06_crossover.txt; option "variant" 19: the whole LDS as before)
    const long long need256 = (long long)(256 + direct_pad4(ww_max)) * (16 + wh_max - 1);
    const bool two_wg = need256 <= DR2_LDS_FLOATS / 2 - 256 && direct_wgs(ch, cw, 256, 16) >= 256 && variant != 19;
    if (two_wg) { r.NB = 1; r.RW = 2; r.w4 = true; r.lds_floats = (int)need256; }
    else if (direct_fits512(ww_max) && direct_wgs(ch, cw, 512, 16) >= 512 && variant != 16) { r.NB = 2; r.RW = 2; }
    else if (direct_wgs(ch, cw, 256, 16) >= 256) { r.NB = 1; r.RW = 2; }
    else { r.NB = 1; r.RW = 1; }
    return r;
}

// orientations one launch is asked to fold: small DEMs fold up to 32, in order, inside the workgroup that owns a patch
// - a 512 x 512 search is 905 launches of a few microseconds otherwise; DEMs of a thousand workgroups per orientation
// gain nothing
inline int direct_batch_want(int ch, int cw) {
    const long long wg1 = (long long)((cw + 255) / 256) * ((ch + 7) / 8);
    return wg1 <= 1024 ? 32 : 1;
}

// does a built-in template have window rows of SC_DR_SHARE_MIN taps or more along x: about min(2c / |cos a|,
// 2d / |sin a|) cells for its c x d rectangle (a window uploaded by the host: unknown, taken as long)
inline bool direct_long_runs(bool uploaded, double c, double d, double cos_a, double sin_a, double dx) {
    if (uploaded) return true;
    const double ca = fabs(cos_a) + 1e-9, sa = fabs(sin_a) + 1e-9;
    const double by_c = 2.0 * c / ca, by_d = 2.0 * d / sa;
    return (by_c < by_d ? by_c : by_d) / fabs(dx) >= (double)SC_DR_SHARE_MIN;
}

// template rows per slab, as k_direct2 computes them for a template of wh rows and a padded pitch of P taps:
// the slab holds rows of 256 NB + P cells, a template row for every output row of the patch
inline int direct_slab_rows(const DirectRoute& r, int P, int wh) {
    const int lwp = 256 * r.NB + P, ty = DR2_WAVES * r.RW;
    int na = r.lds_floats / lwp - (ty - 1);
    if (na > wh) na = wh;
    return na < 1 ? 1 : na;
}
inline int direct_slabs(const DirectRoute& r, int P, int wh) {
    const int na = direct_slab_rows(r, P, wh);
    return (wh + na - 1) / na;
}
