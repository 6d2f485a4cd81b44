// What sc_channel_profiles* (sc_channel.hip) and sc_channel_segments* (sc_channel_segment.hip) share (docs/channels.md):
// the column of a (shift, frequency) pair, the Sep sweep of a complete profile, the two searches over the pairs, and the
// launch of the call's tables.  The pieces underneath are those of sc_fit.h.
#pragma once
#include "sc_fit.h"

// The tables of a channel call, both launches in one SC_K_PROFILE bracket: G over x = -(h + D)..(h + D) into d_tab
// ((2 (h + D) + 1) F doubles on the device) from d_freqs, and - option "channel_terms" - what a pair's column leaves
// against (1, s) on a profile without a missing point, into the context's buffer: *d_terms, or null with the option off
int sc_ch_tables(sc_ctx* ctx, const double* d_freqs, int F, int h, int D, double de, double* d_tab, const double** d_terms);
// the checks a channel call adds to those of its frame: the frequencies ahead of them, pi f de <= SC_CHANNEL_MAX_ARG behind
int sc_ch_check_freqs(sc_ctx* ctx, const char* who, const double* freqs, int F);
int sc_ch_check_arg(sc_ctx* ctx, const char* who, const double* freqs, int F, double de);
// every refusal of sc_channel_segments (sc_channel_segment.hip), for the calls that share its arguments (sc_channel_bootstrap.hip,
// sc_channel_strike.hip): the frequencies, the mode, D, sc_sg_check's with the park's cap, then pi f de
int sc_cs_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                const double* freqs, int F, int h, int w, int D, int mode, double de, double delta, int min_samples,
                int min_profiles, const void* out_rows);
// the degrees of freedom of a reach - or of a window of one - of m usable profiles and n pooled points
__device__ __forceinline__ int cs_dof(int mode, int m, int n, int D) {
    return mode == SC_CHANNEL_DEPTH_PROFILE ? n - (3 + (D > 0 ? 1 : 0)) * m : sg_dof(m, n, D);
}
// Stage one of sc_channel_segments on a chunk of whole reaches (sc_channel_segment.hip), shared with sc_channel_bootstrap.hip
// and sc_channel_strike.hip:
// the dynamic-LDS limit of k_cs_stage and where G sits, once a call; then k_cs_stage - none for a chunk without cells -
// and k_sg_rank inside the chunk's timing bracket, the number of launches returned.  d_tab is G, d_terms what sc_ch_tables
// left; park_prof: the profiles go to st.prof for k_sg_resid
struct cs_stage_plan { bool tab_lds; size_t lds; };
int sc_cs_stage_attr(sc_ctx* ctx, int F, int h, int D, cs_stage_plan* plan);
int sc_cs_stage_launch(sc_ctx* ctx, const cs_stage_plan& plan, const double* z, int ny, int nx, int F, int h, int w, int D,
                       double de, int min_samples, int mode, const double* d_tab, const double* d_terms, bool park_prof,
                       const sg_stage& st);

// pair q = r F + i (rank r of the shift, frequency i): the column of shift d is row j - d of the table
__device__ __forceinline__ pf_tab_col ch_col(const double* tab, int F, int D, int r, int i) {
    return pf_at(tab + (size_t)(D - sh_shift_of(r)) * F + i, F);
}

// the Sep of pf_rest alone, t.ebar and t.gamma given: its loop, its e2 * p2 sum, in its order
template <class E>
__device__ __forceinline__ double ch_sep(const double* prof, int np, int h, double de, const pf_lin& L, const E& e,
                                         const pf_col& t) {
    double Sep = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double sc = (double)(jj - h) * de - L.sbar;
        const double e2 = (e(jj) - t.ebar) - t.gamma * sc;
        const double p2 = (p - L.pbar) - L.beta * sc;
        Sep += e2 * p2;
    }
    return Sep;
}

// one pair's fit on either route: terms (or null) are k_ch_terms' planes of P pairs, for a profile without a missing point
template <class E>
__device__ __forceinline__ double ch_pair(const double* prof, const double* __restrict__ terms, int P, int q, int np, int h,
                                          double de, const pf_lin& L, const E& e, pf_col& t, double& a, double& b, double& c0) {
    if (terms) {
        t.ebar = terms[q];
        t.gamma = terms[(size_t)P + q];
        t.See = terms[2 * (size_t)P + q];
        t.Sep = ch_sep(prof, np, h, de, L, e, t);
        a = t.Sep / t.See;
        pf_slope(L.sbar, L.pbar, L.beta, t.ebar, t.gamma, a, b, c0);
        return pf_sse(prof, np, h, de, e, a, b, c0);
    }
    return pf_candidate(prof, np, h, de, L, e, t, a, b, c0);
}

// sh_search for the channel: the shift d_i with the smallest sse among d = -D..D in the order 0, -1, +1, ... for every
// frequency i.  A pair whose See is not > 0 - a Gaussian whose every entry on the profile's points is 0 - or whose sse
// is NaN is dead: its key is +inf and it never wins against a live one.  terms (or null): k_ch_terms' planes, for a
// profile without a missing point (uniform per wave).  slot: key, sse (NaN where no pair of the frequency is alive), a, b,
// c0; the rank
__device__ __forceinline__ void ch_search(const double* prof, const double* tab, const double* __restrict__ terms, int np,
                                          int h, int F, int D, double de, int lane, const pf_lin& L, double* slot) {
    int* srank = (int*)(slot + (size_t)SH_TERMS * F);
    const int P = F * (2 * D + 1);
    for (int q0 = 0; q0 < P; q0 += 64) {
        const bool on = q0 + lane < P;
        const int q = on ? q0 + lane : P - 1;            // lanes beyond the pairs repeat the last one and are ignored
        const int r = q / F, i = q - r * F;
        const pf_tab_col e = ch_col(tab, F, D, r, i);
        pf_col t;
        double a, b, c0, sse;
        if (terms) {
            t.ebar = terms[q];
            t.gamma = terms[(size_t)P + q];
            t.See = terms[2 * (size_t)P + q];
            t.Sep = ch_sep(prof, np, h, de, L, e, t);
            a = t.Sep / t.See;
            pf_slope(L.sbar, L.pbar, L.beta, t.ebar, t.gamma, a, b, c0);
            sse = pf_sse(prof, np, h, de, e, a, b, c0);
        } else {
            sse = pf_candidate(prof, np, h, de, L, e, t, a, b, c0);
        }
        const bool alive = on && t.See > 0.0 && sse == sse;
        const double key = alive ? sse : INFINITY;
        // the round's winner of every frequency: argmin over the lanes F apart
        const int win = pair_winner(key, on ? r : INT_MAX, F, lane);
        if (on && r == win) {                            // (one lane per frequency)
            if (q0 == 0 || key < slot[i]) {              // (every frequency meets its rank 0 in the first round: F <= 64)
                slot[i] = key;
                slot[F + i] = alive ? sse : __builtin_nan("");
                slot[2 * F + i] = a;
                slot[3 * F + i] = b;
                slot[4 * F + i] = c0;
                srank[i] = r;
            }
        }
        wave_sync();                                     // (the next round's winners, and the caller, read the slot)
    }
}

// ch_search keeping what the joint fit sums: the same pairs on the same routes, the same dead-pair rule and the same
// winner, and in the slot the winner's sse (NaN where no pair of the frequency is alive: its key is then +inf), See, Sep,
// ebar, gamma - sh_search's layout - and the rank.  a = Sep / See and pf_slope on these give ch_search's a, b and c0 bit
// for bit: they are the operations that formed them
__device__ __forceinline__ void ch_search_terms(const double* prof, const double* tab, const double* __restrict__ terms, int np,
                                                int h, int F, int D, double de, int lane, const pf_lin& L, double* slot) {
    int* srank = (int*)(slot + (size_t)SH_TERMS * F);
    const int P = F * (2 * D + 1);
    for (int q0 = 0; q0 < P; q0 += 64) {
        const bool on = q0 + lane < P;
        const int q = on ? q0 + lane : P - 1;            // lanes beyond the pairs repeat the last one and are ignored
        const int r = q / F, i = q - r * F;
        pf_col t;
        double a, b, c0;
        const double sse = ch_pair(prof, terms, P, q, np, h, de, L, ch_col(tab, F, D, r, i), t, a, b, c0);
        const bool alive = on && t.See > 0.0 && sse == sse;
        const double key = alive ? sse : INFINITY;
        // the round's winner of every frequency: argmin over the lanes F apart
        const int win = pair_winner(key, on ? r : INT_MAX, F, lane);
        if (on && r == win) {                            // (one lane per frequency)
            const double cur = slot[i];
            if (q0 == 0 || key < ((cur == cur) ? cur : INFINITY)) {       // (every frequency meets its rank 0 in the first round)
                slot[i] = alive ? sse : __builtin_nan("");
                slot[F + i] = t.See;
                slot[2 * F + i] = t.Sep;
                slot[3 * F + i] = t.ebar;
                slot[4 * F + i] = t.gamma;
                srank[i] = r;
            }
        }
        wave_sync();                                     // (the next round's winners, and the caller, read the slot)
    }
}
