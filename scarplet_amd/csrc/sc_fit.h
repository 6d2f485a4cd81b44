// The fit of sc_fit_profiles* and sc_fit_segments* (docs/profiles.md, docs/segments.md), each piece of it written once:
// the arithmetic AND the frame around it.  Included by sc_profile.hip and sc_segment.hip - by sc_bootstrap.hip and
// sc_strike.hip for stage one -, by sc_robust.hip, whose weighted sweeps (at the end) are these with a weight on every
// term, by sc_segment_robust.hip, the joint fit on those sweeps, by sc_ramp.hip and sc_segment_ramp.hip, the initial slope
// of the two, by sc_refine.hip and sc_segment_refine.hip, the ages off the grid of the two (rf_col), and by sc_lateral.hip for
// the sampler and the host frame; by sc_channel.hip and sc_channel_segment.hip through sc_channel.h.  Who owns what:
//   host    sc_profile.hip defines the frame of every per-cell call: the DEM's source (sc_pf_dem), the erf table
//           (sc_pf_table) and the chunked driver (sc_pf_chunks), to which a call hands its one launch line.
//           sc_segment.hip defines the frame of every segment call: the argument checks with the one cap refusal
//           (sc_sg_check, sc_sg_check_cap), the chunked driver (sc_sg_chunks), to which a call hands the shape of its
//           park, its outputs and its launches, stage one and the segmented sum (sc_sg_sum_launch).  What the host
//           computes of a chunk - where it ends, its CSR arrays, the cap - is sc_fit_chunk.h's
//   device  pf_stage and pf_each_cell are the frame of a kernel with one wave per cell, pf_fetch brings a parked profile
//           back (k_sg_resid, k_sq_step, k_sq_loss); pf_column, pf_rest and pf_sse take
//           their column through an accessor (pf_at: a table's column, rp_col: the ramp's); pf_candidate, pair_winner
//           and wave_sync are what sh_search and rp_search share
// The library is built with -ffp-contract=off and every helper here is inlined, so a helper does the operations of its
// text in the order of its text wherever it is called: the calls return the same bits in every field they share because
// they call the same helpers.
#pragma once
#include "sc_fit_chunk.h"
#include "sc_internal.h"
#include <math.h>
#include <functional>
#include <vector>

#define PF_WAVES 4                       // cells in flight per workgroup: one wave per cell
#define PF_THREADS (64 * PF_WAVES)
#define PF_TAB_LDS 65536                 // the erf table goes to LDS up to this many bytes
#define PF_MAX_GRID 2048
#ifndef PF_CHUNK
#define PF_CHUNK (1ll << 19)             // cells per launch of a per-cell call: bounds its buffers (rows, 8 A B a curve)
#endif

// ---- sc_profile.hip, shared with sc_segment.hip (`who` names the call in the messages) ----------------------------------
// the argument checks of a profile call
int sc_pf_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const double* ages, int A, int h, int w, double de, double delta,
                int min_samples, const void* out_rows);
// the rules of the shift range D of sc_fit_profiles_shift / sc_fit_segments_shift
int sc_pf_check_shift(sc_ctx* ctx, const char* who, int h, int D, int min_samples);
// the calls on the context's DEM: it must be set and be the whole grid
int sc_pf_whole_grid(sc_ctx* ctx, const char* who);
// the _dem calls: z (ny x nx float64 on the host) into the call's own buffer
int sc_pf_upload(sc_ctx* ctx, DevBuf& buf, const double* z, int ny, int nx);
// the DEM a call works on: z uploaded into buf, or - z null - the context's own (the device is set either way)
int sc_pf_dem(sc_ctx* ctx, DevBuf& buf, const double* z, int ny, int nx, const double** z_dev);
// the launch of the erf table over j = -h..h (d_ages on the device; timed as SC_K_PROFILE)
int sc_pf_table(sc_ctx* ctx, const double* d_ages, int A, int h, double de, double* d_tab);
// The chunked driver of the per-cell calls (K >= 1 cells, at most `chunk` a launch, in the pf_ buffers of the context).  Per
// chunk: cells and (sa, ca) go up, the rows are cleared, `launch` issues the call's ONE kernel launch on the chunk's m
// cells inside the SC_K_PROFILE bracket, the rows and the planes that were asked for come back, and the stream is
// synchronised.  A plane is an optional per-cell output: the float64 curve or the int8 shifts / widths (host null: none,
// and its device pointer is null)
struct pf_plane { void* host; DevBuf* buf; size_t cell_bytes; };
struct pf_chunk { long long* cells; double* dir; void* rows; void* plane[2]; };
typedef std::function<void(const pf_chunk&, long long m)> pf_launch;
int sc_pf_chunks(sc_ctx* ctx, const long long* cells, const double* sa, const double* ca, long long K, long long chunk,
                 size_t row_bytes, void* out_rows, const pf_plane& p0, const pf_plane& p1, const pf_launch& launch);
// the grids of a kernel with one wave per cell over m cells, and of one with a workgroup per item (segment, block) over n
static inline unsigned pf_grid(long long m) {
    const long long g = (m + PF_WAVES - 1) / PF_WAVES;
    return (unsigned)(g < 1 ? 1 : g > PF_MAX_GRID ? PF_MAX_GRID : g);
}
static inline unsigned sg_grid(long long n) { return (unsigned)(n < 1 ? 1 : n > 65536 ? 65536 : n); }

// ---- sc_ramp.hip, shared with sc_segment_ramp.hip ---------------------------------------------------------------------------
// the rules of the width range M, the mode and the slope of sc_fit_profiles_ramp / sc_fit_segments_ramp
int sc_rp_check(sc_ctx* ctx, const char* who, int h, int M, int mode, double slope, int min_samples);
// the launch of the table of F over x = -ht..ht (d_ages on the device; timed as SC_K_PROFILE)
int sc_rp_table(sc_ctx* ctx, const double* d_ages, int A, int ht, double de, double* d_ftab);

// ---- sc_segment.hip, shared with every segment call ---------------------------------------------------------------------------
// The park of a cell: `prof` doubles of the profile (2h + 1; twice that with a weight plane behind the profiles), `planes`
// per-cell-and-column planes (4; SC_SEGMENT_ROBUST_PLANES) of C columns (A ages; the A (M + 1) pairs of the initial slope),
// and - shift - d_ci, one byte a column.  The cells of one segment that it holds: sc_fit_park_cap of SC_SEGMENT_MAX_PARK
struct sg_park { int prof, planes, C; bool shift; };
static inline sg_park sg_park_plain(int A, int h, bool shift) { return {2 * h + 1, 4, A, shift}; }
long long sc_sg_cap_cells(const sg_park& park);
// the argument checks of a segment call (D < 0: the call without a shift), the last of them sc_sg_check_cap on the plain
// park ("... at this h and A")
int sc_sg_check(sc_ctx* ctx, const char* who, long long ny, long long nx, const long long* cells, const double* sa,
                const double* ca, long long K, const long long* seg_start, const int32_t* seg_label, long long S,
                const double* ages, int A, int h, int w, int D, double de, double delta, int min_samples, int min_profiles,
                const void* out_rows);
// SC_ERR_UNSUPPORTED for the first segment of more than `cap` cells: "<who>: a segment of N cells, more than <cap> <tail>"
int sc_sg_check_cap(sc_ctx* ctx, const char* who, const long long* seg_start, long long S, long long cap, const char* tail);
// Stage one of a chunk of whole segments: the host arrays that go up (kept until the stream is synchronised) and, on the
// device, the chunk's cells, (sa, ca), CSR array over cells and labels, what the parking kernel leaves (profiles, n
// and used, sbar / pbar / beta, the park's planes - k_sg_partial / k_sg_shift: ebar, gamma, See, Sep, at d_ci with a shift -
// and d_ci) and what k_sg_rank leaves (the usable cells of each segment in order; n_profiles and the pooled n per segment)
struct sg_stage {
    std::vector<double> dir;
    std::vector<int> start;
    long long Sc = 0, m = 0;
    long long* cells = nullptr;
    double *dirs = nullptr, *prof = nullptr, *scal = nullptr, *planes = nullptr;
    int *seg = nullptr, *label = nullptr, *cn = nullptr, *used = nullptr, *list = nullptr, *cnt = nullptr;
    signed char* shift = nullptr;
};
// the dynamic-LDS limit of k_sg_partial / k_sg_shift, and their launch and k_sg_rank's inside the chunk's timing bracket:
// returns the number of launches (the parking kernel - none for a chunk without cells - and k_sg_rank)
int sc_sg_stage_attr(sc_ctx* ctx, int A, int h, int D);
int sc_sg_stage_launch(sc_ctx* ctx, const double* z, int ny, int nx, int A, int h, int w, int D, double de, int min_samples,
                       const double* d_tab, const sg_stage& st);

// The chunked driver of the segment calls (S >= 1 segments, in the sg_ buffers of the context).  Once: the ages and the erf
// table over j = -ht..ht go up and `tables` (if any) adds the call's further tables.  Per chunk of whole segments s0..s1 -
// sc_fit_chunk_end under max_segs, the park's cap lowered by option "fit_chunk", and the second CSR array `aux` under max_aux -
// stage one is sized by the park and its host arrays go up; a call that sums in blocks (`sums` > 0) gets cseg and blk on the
// device and the buffers of sc_sg_sum_launch (part; tot, two planes of C columns a segment; tsum, `sums` planes: what
// the second sum of the call leaves); the outputs are sized and those marked are cleared; `prepare` (if any) sizes and uploads what is private to the call; `launch` issues the call's
// launches inside the SC_K_PROFILE bracket and returns their number, or an error; the outputs that were asked for come
// back to their place, and the stream is synchronised.
// An output: `item` bytes for each of the chunk's segments, cells or items of `aux`.  Its device copy is null where the
// host pointer is - unless the kernels need it whether or not it is asked for (always)
enum sg_axis { SG_SEGS, SG_CELLS, SG_AUX };
struct sg_out { void* host; DevBuf* buf; size_t item; sg_axis axis; bool clear = false, always = false; };
struct sg_chunk {
    const sg_stage& st;                  // st.Sc segments, st.m cells
    long long s0, s1, k0, G;             // the first and the end segment, the first cell; the blocks (0 without `sums`)
    const int *cseg, *blk;               // the segment of every cell and the CSR array of blocks over segments, or null
    double *part, *tot, *tsum;           // the partial sums of the blocks and the two totals of the segments, or null
    const std::vector<void*>& out;       // the device copies of the outputs, in the order of the call's list
    const double *ages, *tab;
};
struct sg_call {
    const long long* cells; const double *sa, *ca; const long long* seg_start; const int32_t* seg_label; long long S;
    const double* ages; int A, ht; double de;
    sg_park park;
    long long max_segs; const long long* aux; long long max_aux;
    int sums;
    std::vector<sg_out> out;
    std::function<int(const double* d_ages)> tables;
    std::function<int(const sg_chunk&)> prepare, launch;
};
int sc_sg_chunks(sc_ctx* ctx, const sg_call& call);
// The grid fit of the chunk after stage one (D < 0: the call without a shift): the two segmented sums, k_sg_resid between them (none of the five
// for a chunk without cells) and k_sg_choose into rows, cells (or null; sc_segment_shift_cell with a shift) and curve (or null).  `fine`
// (D < 0): the rows and the cells are sc_segment_fine_fit and sc_segment_fine_cell, whose shared fields the same kernel writes.  Returns the
// number of launches.  The LDS limit of k_sg_resid is raised by sc_sg_grid_attr before the first chunk
int sc_sg_grid_attr(sc_ctx* ctx, int A, int h, int D);
int sc_sg_grid_launch(sc_ctx* ctx, const sg_chunk& k, int A, int h, int D, double de, double delta, int min_profiles, bool fine,
                      void* rows, void* cells, double* curve);
// k_sg_resid alone, after the sum of (See, Sep) into k.tot, on whatever table k.tab is - rows j = -(h + D)..(h + D) of A
// columns, the cell's column at column i its row j - d_ci (sc_channel_segment.hip: the Gaussian table); D < 0: no shift
void sc_sg_resid_launch(sc_ctx* ctx, const sg_chunk& k, int A, int h, int D, double de, int min_profiles);
// k_sg_rank alone, on what another parking kernel left in st.cn and st.used (sc_segment_ramp.hip)
void sc_sg_rank_launch(sc_ctx* ctx, const sg_stage& st);

// k_sg_sum1<P> and k_sg_sum2<P> on P (1 or 2) neighbouring per-cell-and-column planes (src, src + m C) of the stage's chunk:
// the blocked sum of docs/segments.md into tot (Sc x P x C); blk: the CSR array of blocks over the chunk's segments, G its
// blocks.  C = A columns, or the A (M + 1) pairs of sc_segment_ramp.hip
void sc_sg_sum_launch(sc_ctx* ctx, const double* src, const sg_stage& st, const int* blk, long long G, int C, int P,
                      double* part, double* tot);

// ---- sc_robust.hip, shared with sc_segment_robust.hip -----------------------------------------------------------------------
// the rules of the loss, the tuning constant, the iterations and the scale of sc_fit_profiles_robust / sc_fit_segments_robust
int sc_rb_check(sc_ctx* ctx, const char* who, int loss, double tuning, int iterations, double scale);

// the degrees of freedom of a segment - or of a window of one, sc_strike.hip - of m usable profiles and n pooled points
// (D = 0 in the call without a shift), and whether it is fitted
__device__ __forceinline__ int sg_dof(int m, int n, int D) { return n - 2 * m - 1 - (D > 0 ? m : 0); }
__device__ __forceinline__ bool sg_fitted(int m, int dof, int min_profiles) { return m >= min_profiles && dof >= 1; }

// ---- the centre shift (docs/profiles.md, "The centre shift") --------------------------------------------------------------
// candidates in the order 0, -1, +1, -2, +2, ...: rank r -> shift d
__host__ __device__ __forceinline__ int sh_shift_of(int r) { return (r & 1) ? -((r + 1) >> 1) : (r >> 1); }

#define SH_TERMS 5             // what a wave keeps per age of the best shift: sse, See, Sep, ebar, gamma
__host__ __device__ __forceinline__ size_t sh_slot_doubles(int A) { return (size_t)SH_TERMS * A + (size_t)((A + 1) / 2); }

// ---- dynamic LDS of a kernel with one wave per cell ------------------------------------------------------------------------
// PF_WAVES profiles of np points, then PF_WAVES slots of the shift search where the kernel searches, then the erf table
// (nt rows of A) where it is staged.  The host sizes the launch by the same two functions.
__host__ __device__ __forceinline__ size_t pf_lds_head(int np, int A, bool slots) {
    return (size_t)PF_WAVES * ((size_t)np + (slots ? sh_slot_doubles(A) : 0));
}
__host__ __device__ __forceinline__ size_t pf_lds_bytes(int np, int nt, int A, bool slots, bool tab_lds) {
    return sizeof(double) * (pf_lds_head(np, A, slots) + (tab_lds ? (size_t)nt * A : 0));
}

struct pf_lds {
    double* prof;              // this wave's profile
    double* slot;              // this wave's slot of the search (SLOTS)
    const double* tab;         // the table: in LDS (TAB_LDS) or where it was
};

// carves the workgroup's LDS and stages the table; ends in a barrier
template <bool TAB_LDS, bool SLOTS>
__device__ __forceinline__ pf_lds pf_stage(const double* __restrict__ tab_g, int np, int nt, int A) {
    extern __shared__ double pf_lds_mem[];
    const int wave = threadIdx.x >> 6;
    pf_lds L;
    L.prof = pf_lds_mem + (size_t)wave * np;
    L.slot = SLOTS ? pf_lds_mem + (size_t)PF_WAVES * np + (size_t)wave * sh_slot_doubles(A) : nullptr;
    L.tab = tab_g;
    if (TAB_LDS) {
        double* t = pf_lds_mem + pf_lds_head(np, A, SLOTS);
        for (int idx = threadIdx.x; idx < nt * A; idx += PF_THREADS) t[idx] = tab_g[idx];
        L.tab = t;
    }
    __syncthreads();
    return L;
}

// The loop of such a kernel, written once: workgroups stride over rounds of PF_WAVES cells, so that the cells in flight are
// neighbours of the input order.  Wave w of round g takes input cell kc = g PF_WAVES + w: cut(kc, cell) puts its profile
// into the wave's LDS, fit(kc, cell) does the rest.  The loop's bound is uniform per workgroup, so every wave meets both
// barriers of every round - a wave past the end with nothing to do
template <class CUT, class FIT>
__device__ __forceinline__ void pf_each_cell(const long long* __restrict__ cells, long long K, CUT cut, FIT fit) {
    const int wave = threadIdx.x >> 6;
    const long long rounds = (K + PF_WAVES - 1) / PF_WAVES;
    for (long long g = blockIdx.x; g < rounds; g += gridDim.x) {      // (uniform per workgroup: the barriers below)
        const long long kc = g * PF_WAVES + wave;
        const bool act = kc < K;
        long long cell = 0;
        if (act) {
            cell = cells[kc];
            cut(kc, cell);
        }
        __syncthreads();
        if (act) fit(kc, cell);
        __syncthreads();
    }
}

// what a cell without a fit leaves in the optional planes: NaN in its curve, 0 in its shifts / widths
__device__ __forceinline__ void pf_unfit_planes(long long kc, int lane, int A, double* __restrict__ curve,
                                                signed char* __restrict__ plane) {
    if (curve && lane < A) curve[kc * A + lane] = __builtin_nan("");
    if (plane && lane < A) plane[kc * A + lane] = 0;
}

// (one wave: the lanes read what the others wrote, and what they read is overwritten afterwards)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- sampling (docs/profiles.md, "Samples") ----------------------------------------------------------------------------------
// one bilinear sample; false where it is outside the grid or not finite
__device__ __forceinline__ bool pf_sample(const double* __restrict__ z, int ny, int nx, double rr, double cc, double& v) {
    if (!(rr >= 0.0 && rr <= (double)(ny - 1) && cc >= 0.0 && cc <= (double)(nx - 1))) return false;
    const int r0 = min((int)floor(rr), ny - 2), c0 = min((int)floor(cc), nx - 2);
    const double fr = rr - (double)r0, fc = cc - (double)c0;
    const double* q = z + (size_t)r0 * nx + c0;
    const double z00 = q[0], z01 = q[1], z10 = q[nx], z11 = q[nx + 1];
    v = (z00 * (1.0 - fc) + z01 * fc) * (1.0 - fr) + (z10 * (1.0 - fc) + z11 * fc) * fr;
    return isfinite(v);
}

// one point of a profile: the mean of the valid samples across the swath in ascending k, NaN where none is valid
__device__ __forceinline__ double pf_point(const double* __restrict__ z, int ny, int nx, double r, double c, double sa,
                                           double ca, int jj, int h, int w) {
    const double j = (double)(jj - h);
    const double jsa = j * sa, jca = j * ca;
    double acc = 0.0;
    int cnt = 0;
    for (int kk = -w; kk <= w; ++kk) {
        const double k = (double)kk;
        const double rr = r + (k * ca - jsa), cc = c + (jca + k * sa);
        double v;
        if (pf_sample(z, ny, nx, rr, cc, v)) {
            acc += v;
            ++cnt;
        }
    }
    return cnt ? acc / (double)cnt : __builtin_nan("");
}

// the profile of input cell kc, lanes over its points: into the wave's LDS and, where park is given, global memory
__device__ __forceinline__ void pf_cut(const double* __restrict__ z, int ny, int nx, long long cell,
                                       const double* __restrict__ dir, long long kc, int h, int w, int lane, double* prof,
                                       double* __restrict__ park) {
    const int np = 2 * h + 1;
    const double sa = dir[2 * kc], ca = dir[2 * kc + 1];
    const double r = (double)(cell / nx), c = (double)(cell % nx);
    for (int jj = lane; jj < np; jj += 64) {
        const double p = pf_point(z, ny, nx, r, c, sa, ca, jj, h, w);
        prof[jj] = p;
        if (park) park[(size_t)kc * np + jj] = p;
    }
}

// ---- the fit of one erf column to one profile ----------------------------------------------------------------------------------
// The profile is in LDS, NaN marking a missing point; point jj has s = (jj - h) de and the column's e is col[jj * A].
// Every sum is a plain loop over ascending jj in one lane.  The lanes-over-ages kernels (k_pf_fit, k_sg_partial) take
// the column's sums in the sweeps that form the profile's own (COL); the kernels of the shift form the profile's once
// (no COL) and each (shift, age) pair's by pf_column.  An in-order sum is the same bits in a sweep of its own.
struct pf_mom { int n, n_neg, n_pos; double Ss, Sp, Se; };      // pass 0: counts (all, j < 0, j > 0) and plain sums
struct pf_lin { double dn, sbar, pbar, Sss, beta; };            // the profile against (1, s)
struct pf_col { double ebar, gamma, See, Sep; };                // the column against (1, s), and what is left of both

template <bool COL>
__device__ __forceinline__ pf_mom pf_moments(const double* prof, int np, int h, double de, const double* col, int A) {
    pf_mom m = {0, 0, 0, 0.0, 0.0, 0.0};
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        ++m.n;
        m.n_neg += jj < h ? 1 : 0;
        m.n_pos += jj > h ? 1 : 0;
        m.Ss += (double)(jj - h) * de;
        m.Sp += p;
        if (COL) m.Se += col[(size_t)jj * A];
    }
    return m;
}

// pass 1: the centred s against itself and p - and against e (COL: t.ebar and t.gamma)
template <bool COL>
__device__ __forceinline__ pf_lin pf_line(const double* prof, int np, int h, double de, const pf_mom& m, const double* col,
                                          int A, pf_col& t) {
    pf_lin L;
    L.dn = (double)m.n;
    L.sbar = m.Ss / L.dn;
    L.pbar = m.Sp / L.dn;
    if (COL) t.ebar = m.Se / L.dn;
    double Sss = 0.0, Sps = 0.0, Ses = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double sc = (double)(jj - h) * de - L.sbar;
        Sss += sc * sc;
        Sps += sc * (p - L.pbar);
        if (COL) Ses += sc * (col[(size_t)jj * A] - t.ebar);
    }
    L.Sss = Sss;
    L.beta = Sps / Sss;
    if (COL) t.gamma = Ses / Sss;
    return L;
}

// From here on a sweep takes its column through an accessor E: e(jj) is the column's entry at point jj.  pf_at is a
// column of a table - the entry of one age in A doubles a row, col[jj * A] -, rp_col (below) the diffused ramp's.
struct pf_tab_col {
    const double* col;
    int A;
    __device__ __forceinline__ double operator()(int jj) const { return col[(size_t)jj * A]; }
};
__device__ __forceinline__ pf_tab_col pf_at(const double* col, int A) { return pf_tab_col{col, A}; }

// pass 2: what is left of e after 1 and s, against what is left of p (t.ebar and t.gamma in, t.See and t.Sep out)
template <class E>
__device__ __forceinline__ void pf_rest(const double* prof, int np, int h, double de, const pf_lin& L, const E& e, pf_col& t) {
    double See = 0.0, Sep = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double sc = (double)(jj - h) * de - L.sbar;
        const double e2 = (e(jj) - t.ebar) - t.gamma * sc;
        const double p2 = (p - L.pbar) - L.beta * sc;
        See += e2 * e2;
        Sep += e2 * p2;
    }
    t.See = See;
    t.Sep = Sep;
}

// passes 0 to 2 of a column alone, the profile's own terms given
template <class E>
__device__ __forceinline__ pf_col pf_column(const double* prof, int np, int h, double de, const pf_lin& L, const E& e) {
    pf_col t;
    double Se = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        Se += e(jj);
    }
    t.ebar = Se / L.dn;
    double Ses = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double sc = (double)(jj - h) * de - L.sbar;
        Ses += sc * (e(jj) - t.ebar);
    }
    t.gamma = Ses / L.Sss;
    pf_rest(prof, np, h, de, L, e, t);
    return t;
}

// slope and intercept of a profile once the amplitude a is known (its own Sep / See, or the segment's)
__device__ __forceinline__ void pf_slope(double sbar, double pbar, double beta, double ebar, double gamma, double a,
                                         double& b, double& c0) {
    b = beta - a * gamma;
    c0 = (pbar - a * ebar) - b * sbar;
}

// pass 3: the explicit residuals
template <class E>
__device__ __forceinline__ double pf_sse(const double* prof, int np, int h, double de, const E& e, double a, double b,
                                         double c0) {
    double sse = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double s = (double)(jj - h) * de;
        const double res = p - ((c0 + b * s) + a * e(jj));
        sse += res * res;
    }
    return sse;
}

// passes 0 to 3 of one candidate column, the profile's own terms given: its terms t, its own a = Sep / See with (b, c0),
// and the sse of that fit
template <class E>
__device__ __forceinline__ double pf_candidate(const double* prof, int np, int h, double de, const pf_lin& L, const E& e,
                                               pf_col& t, double& a, double& b, double& c0) {
    t = pf_column(prof, np, h, de, L, e);
    a = t.Sep / t.See;
    pf_slope(L.sbar, L.pbar, L.beta, t.ebar, t.gamma, a, b, c0);
    return pf_sse(prof, np, h, de, e, a, b, c0);
}

// ---- the column of an age off the grid (docs/profiles.md, "Continuous ages") ------------------------------------------------------
// Shared by sc_refine.hip and sc_segment_refine.hip.
// the column of a candidate age x that no table holds: den = 2.0 * sqrt(x), and e(jj) is k_pf_table's expression.  Beyond
// |argument| = RF_SAT the erf is +-1 in float64 (1 - erf(6) = 2.2e-17, under half a unit in the last place of 1), so the
// tails of a profile - most of its points at a young age - cost a comparison where the whole wave is there
#define RF_SAT 6.0
struct rf_col {
    double den, de;
    int h;
    __device__ __forceinline__ double operator()(int jj) const {
        const double x = ((double)(jj - h) * de) / den;
        if (fabs(x) >= RF_SAT) return copysign(1.0, x);
        return erf(x);
    }
};

// candidate l of the bracket [p, q]
__device__ __forceinline__ double rf_x(double p, double q, int l) { return l == 63 ? q : p + (q - p) * ((double)l / 63.0); }

// ---- the choice over the ages ---------------------------------------------------------------------------------------------------
// One wave, lane i holding sse_i (lanes >= A are ignored): argmin with ties to the smaller index (a NaN never wins), thr =
// sse_min (1 + delta / dof), and the interval walked from the best age while sse <= thr.  The same in every lane.
struct pf_pick { int best, lo, hi; double sse_min; };

// the parked profile of cell kc - and, WT, its weights - back into the wave's LDS, lanes over the points
template <bool WT>
__device__ __forceinline__ void pf_fetch(const double* __restrict__ prof_g, const double* __restrict__ u_g, long long kc, int np,
                                         int lane, double* prof, double* u) {
    for (int jj = lane; jj < np; jj += 64) {
        prof[jj] = prof_g[(size_t)kc * np + jj];
        if (WT) u[jj] = u_g[(size_t)kc * np + jj];
    }
}

// the walk alone, from a best age found elsewhere (sc_strike.hip: the argmax of Q_i) with sse_best its sse
__device__ __forceinline__ pf_pick pf_walk(double sse, int lane, int A, int best, double sse_best, double delta, int dof) {
    pf_pick k;
    k.sse_min = sse_best;
    k.best = best;
    const double thr = sse_best * (1.0 + delta / (double)dof);
    const unsigned long long ok = __ballot(lane < A && sse <= thr);
    k.lo = k.hi = k.best;
    while (k.lo > 0 && ((ok >> (k.lo - 1)) & 1ull)) --k.lo;
    while (k.hi < A - 1 && ((ok >> (k.hi + 1)) & 1ull)) ++k.hi;
    return k;
}

__device__ __forceinline__ pf_pick pf_choose(double sse, int lane, int A, double delta, int dof) {
    double m = lane < A ? sse : INFINITY;
    if (m != m) m = INFINITY;
    int mi = lane;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (om < m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    return pf_walk(sse, lane, A, min(mi, A - 1), m, delta, dof);
}

// status bits 2 and 4: the interval is open below, above
__device__ __forceinline__ int pf_open(const pf_pick& k, int A) { return (k.lo == 0 ? 2 : 0) + (k.hi == A - 1 ? 4 : 0); }

// ---- the rows ----------------------------------------------------------------------------------------------------------------
// the fields sc_profile_fit, sc_profile_shift_fit and sc_profile_robust_fit share, of a cell that is not fitted and of one that is (the rows
// were cleared: their padding is part of what the caller compares)
template <class ROW>
__device__ __forceinline__ void pf_row_unfit(ROW* out, long long cell, int n) {
    const double nan = __builtin_nan("");
    out->cell = cell;
    out->n = n;
    out->kt_index = -1;
    out->lo_index = -1;
    out->hi_index = -1;
    out->status = 1;
    out->kt = nan; out->kt_lo = nan; out->kt_hi = nan;
    out->a = nan; out->b = nan; out->c0 = nan;
    out->sse = nan; out->rmse = nan;
}

template <class ROW>
__device__ __forceinline__ void pf_row_fit(ROW* out, long long cell, int n, const pf_pick& k, int status,
                                           const double* __restrict__ ages, double a, double b, double c0, double sse,
                                           int dof) {
    out->cell = cell;
    out->n = n;
    out->kt_index = k.best;
    out->lo_index = k.lo;
    out->hi_index = k.hi;
    out->status = status;
    out->kt = ages[k.best]; out->kt_lo = ages[k.lo]; out->kt_hi = ages[k.hi];
    out->a = a; out->b = b; out->c0 = c0;
    out->sse = sse; out->rmse = sqrt(sse / (double)dof);
}

// ---- the search over (candidate, age) pairs ----------------------------------------------------------------------------------------
// One wave, one profile, and for every age i the best of a list of candidates - the shifts of sh_search, the half-widths
// of rp_search.  The LANES RUN OVER THE (candidate rank, age) PAIRS, age-minor, 64 pairs a round; each lane runs
// pf_candidate for its pair.  The lanes of a round that share an age sit A lanes apart: an argmin over them by shuffles
// (offsets A, 2 A, 4 A, ...) on the key (key, rank) - a pair that cannot win counts as +inf, the smaller rank wins a tie,
// so the order of the combination does not matter - leaves the round's winner of every age known to its lowest lane;
// the winning lane merges its terms into the wave's slot, where a later round wins only when strictly smaller (ranks
// ascend from round to round).  The first smallest in the order of the ranks wins, whatever the round it fell into.
// slot: SH_TERMS x A doubles of the winner, then A ints (its rank, or its m).  No atomics, no float sum across lanes.
// the rank that wins this lane's age in the round: argmin over the lanes A apart (a lane past the end hands back its own
// value; a lane that is not `on` enters with rank INT_MAX), read from the age's lowest lane.  (By reference: by value
// k_pf_ramp takes four more VGPRs than with the loop written out, and crosses 96)
__device__ __forceinline__ int pair_winner(const double& key, const int& rank, int A, int lane) {
    double m = key;
    int mr = rank;
    for (int off = A; off < 64; off <<= 1) {
        const double om = __shfl_down(m, off, 64);
        const int orr = __shfl_down(mr, off, 64);
        if (om < m || (om == m && orr < mr)) { m = om; mr = orr; }
    }
    return __shfl(mr, lane % A, 64);
}

// the shift d_i with the smallest sse among d = -D..D, in the order 0, -1, +1, ...: e_ij is taken from row j - d of the
// table (rows -(h + D)..(h + D), A doubles each); a NaN sse counts as +inf.  slot: sse, See, Sep, ebar, gamma; the rank
__device__ __forceinline__ void sh_search(const double* prof, const double* tab, int np, int h, int A, int D, double de,
                                          int lane, const pf_lin& L, double* slot) {
    int* srank = (int*)(slot + (size_t)SH_TERMS * A);
    const int P = A * (2 * D + 1);
    for (int q0 = 0; q0 < P; q0 += 64) {
        const bool on = q0 + lane < P;
        const int q = on ? q0 + lane : P - 1;            // lanes beyond the pairs repeat the last one and are ignored
        const int r = q / A, i = q - r * A;
        pf_col t;
        double a, b, c0;
        const double sse = pf_candidate(prof, np, h, de, L, pf_at(tab + (size_t)(D - sh_shift_of(r)) * A + i, A), t, a, b, c0);
        // the round's winner of every age: argmin over the lanes A apart (a lane past the end hands back its own value)
        const double key = (on && sse == sse) ? sse : INFINITY;
        const int win = pair_winner(key, on ? r : INT_MAX, A, lane);
        if (on && r == win) {                            // (one lane per age)
            const double cur = slot[i];
            if (q0 == 0 || key < ((cur == cur) ? cur : INFINITY)) {       // (every age meets its rank 0 in the first round)
                slot[i] = sse;
                slot[A + i] = t.See;
                slot[2 * A + i] = t.Sep;
                slot[3 * A + i] = t.ebar;
                slot[4 * A + i] = t.gamma;
                srank[i] = r;
            }
        }
        wave_sync();                                     // (the next round's winners, and the caller, read the slot)
    }
}

// ---- the initial slope (docs/profiles.md, "The initial slope") -----------------------------------------------------------------
// The column of a diffused ramp of half-width m >= 1 cells is a difference of two rows of ONE table per age, F over
// x = -(h + M)..(h + M): e_ij = (F[j + m][i] - F[j - m][i]) / (2 m de), formed in that order.  rp_col holds the two
// rows' first entries of the lane's age (point jj reads hi[jj * A] and lo[jj * A]) and the divisor: the accessor with
// which pf_column and pf_sse fit a ramp.
struct rp_col {
    const double *hi, *lo;
    double den;
    int A;
    __device__ __forceinline__ double operator()(int jj) const { return (hi[(size_t)jj * A] - lo[(size_t)jj * A]) / den; }
};

__device__ __forceinline__ rp_col rp_col_of(const double* ftab, int A, int M, int m, int i, double de) {
    rp_col c;
    c.hi = ftab + (size_t)(M + m) * A + i;               // (row x = j + m sits at jj + M + m, jj = j + h)
    c.lo = ftab + (size_t)(M - m) * A + i;
    c.den = (double)(2 * m) * de;
    c.A = A;
    return c;
}

// the signed initial slope of a pair with m >= 1
__device__ __forceinline__ double rp_slope_of(double a, double b, int m, double de) { return b + a / ((double)m * de); }

// the half-width m_i among m = m0..M (m0 = 0 with the width free, 1 with the slope given) with the smallest key - sse_im,
// or the distance | |b + a / (m de)| - slope |; the smaller m wins a tie.  The m = 0 pairs (all in the first round:
// A <= 64) read the erf table `etab` (rows -h..h, in global memory), the plain call's arithmetic; the others read `ftab`.
// slot: key, sse, a, b, c0 (sse NaN where no pair of the age can win); m
__device__ __forceinline__ void rp_search(const double* prof, const double* __restrict__ etab, const double* ftab, int np, int h,
                                          int A, int M, bool given, double slope, double de, int lane, const pf_lin& L,
                                          double* slot) {
    int* sm = (int*)(slot + (size_t)SH_TERMS * A);
    const int m0 = given ? 1 : 0;
    const int P = A * (M + 1 - m0);
    for (int q0 = 0; q0 < P; q0 += 64) {
        const bool on = q0 + lane < P;
        const int q = on ? q0 + lane : P - 1;            // lanes beyond the pairs repeat the last one and are ignored
        const int r = q / A, i = q - r * A, m = m0 + r;
        pf_col t;
        double a, b, c0, sse;
        if (m == 0)
            sse = pf_candidate(prof, np, h, de, L, pf_at(etab + i, A), t, a, b, c0);
        else
            sse = pf_candidate(prof, np, h, de, L, rp_col_of(ftab, A, M, m, i, de), t, a, b, c0);
        const bool alive = on && t.See > 0.0 && sse == sse;
        double key = given ? fabs(fabs(rp_slope_of(a, b, m, de)) - slope) : sse;
        if (!(alive && key == key)) key = INFINITY;
        // the round's winner of every age: argmin over the lanes A apart (a lane past the end hands back its own value)
        const int win = pair_winner(key, on ? m : INT_MAX, A, lane);
        if (on && m == win) {                            // (one lane per age)
            if (q0 == 0 || key < slot[i]) {              // (every age meets its first candidate in the first round)
                slot[i] = key;
                slot[A + i] = alive ? sse : __builtin_nan("");
                slot[2 * A + i] = a;
                slot[3 * A + i] = b;
                slot[4 * A + i] = c0;
                sm[i] = m;
            }
        }
        wave_sync();                                     // (the next round's winners, and the caller, read the slot)
    }
}

// ---- the weighted fit (docs/profiles.md, "Weights and robust fits") ---------------------------------------------------------------
// The sweeps above with every sum weighted, in the same order.  Point j's weight is q_j = u_j f(|r_j|): u_j the profile's
// own weight (WT: from the wave's LDS beside the profile; else 1) and f the robust factor of the residual r_j of the
// age's PREVIOUS iterate (c0, b, a), which the lane holds in registers - q is recomputed in every sweep and stored
// nowhere.  LOSS 0: q = u (iterate 0, the weighted least squares fit); 1: Huber; 2: Tukey; c = k sigma.  A product by 1
// is exact, so with u = 1 and f = 1 every sum here has the bits of its unweighted twin above.
struct rb_prev { double c0, b, a, c; };

template <int LOSS>
__device__ __forceinline__ double rb_factor(double r, double c) {
    const double x = fabs(r);
    if (LOSS == 1) return x <= c ? 1.0 : c / x;
    if (LOSS == 2) {
        if (!(x < c)) return 0.0;
        const double t = x / c, g = 1.0 - t * t;
        return g * g;
    }
    return 1.0;
}

// rho(r): r^2 capped (Huber: linear beyond c; Tukey: constant c^2 / 3 beyond c)
template <int LOSS>
__device__ __forceinline__ double rb_rho(double r, double c) {
    const double x = fabs(r);
    if (LOSS == 1) return x <= c ? r * r : 2.0 * c * x - c * c;
    if (LOSS == 2) {
        if (!(x < c)) return c * c / 3.0;
        const double t = r / c, g = 1.0 - t * t;
        return (c * c / 3.0) * (1.0 - g * g * g);
    }
    return r * r;
}

__device__ __forceinline__ double rb_resid(double p, double s, double e, const rb_prev& v) {
    return p - ((v.c0 + v.b * s) + v.a * e);
}

template <int LOSS, bool WT>
__device__ __forceinline__ double rb_q(const double* u, int jj, double p, double s, double e, const rb_prev& v) {
    if (!LOSS) return WT ? u[jj] : 1.0;
    const double f = rb_factor<LOSS>(rb_resid(p, s, e, v), v.c);
    return WT ? u[jj] * f : f;
}

// one point of a profile and of the weight plane under it: the means over the samples valid in BOTH, in ascending k
__device__ __forceinline__ void rb_point(const double* __restrict__ z, const double* __restrict__ wt, int ny, int nx, double r,
                                         double c, double sa, double ca, int jj, int h, int w, double& p, double& u) {
    const double j = (double)(jj - h);
    const double jsa = j * sa, jca = j * ca;
    double accp = 0.0, accu = 0.0;
    int cnt = 0;
    for (int kk = -w; kk <= w; ++kk) {
        const double k = (double)kk;
        const double rr = r + (k * ca - jsa), cc = c + (jca + k * sa);
        double v, g;
        if (pf_sample(z, ny, nx, rr, cc, v) && pf_sample(wt, ny, nx, rr, cc, g) && g >= 0.0) {
            accp += v;
            accu += g;
            ++cnt;
        }
    }
    p = u = __builtin_nan("");
    if (cnt) {
        const double um = accu / (double)cnt;
        if (um > 0.0) {
            p = accp / (double)cnt;
            u = um;
        }
    }
}

// the profile and its weights of input cell kc, lanes over the points: into the wave's LDS and, where park is given, global
// memory (the profiles first, then the weights, K cells each)
__device__ __forceinline__ void rb_cut(const double* __restrict__ z, const double* __restrict__ wt, int ny, int nx,
                                       long long cell, const double* __restrict__ dir, long long kc, int h, int w, int lane,
                                       double* prof, double* u, double* __restrict__ park_p = nullptr,
                                       double* __restrict__ park_u = nullptr) {
    const int np = 2 * h + 1;
    const double sa = dir[2 * kc], ca = dir[2 * kc + 1];
    const double r = (double)(cell / nx), c = (double)(cell % nx);
    for (int jj = lane; jj < np; jj += 64) {
        rb_point(z, wt, ny, nx, r, c, sa, ca, jj, h, w, prof[jj], u[jj]);
        if (park_p) {
            park_p[(size_t)kc * np + jj] = prof[jj];
            park_u[(size_t)kc * np + jj] = u[jj];
        }
    }
}

// pass 0: n counts the profile's points, n_neg and n_pos those with q > 0 on either side
struct rb_mom { int n, n_neg, n_pos; double W, Ss, Sp, Se; };

template <int LOSS, bool WT>
__device__ __forceinline__ rb_mom rb_moments(const double* prof, const double* u, int np, int h, double de, const double* col,
                                             int A, const rb_prev& v) {
    rb_mom m = {0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double s = (double)(jj - h) * de, e = col[(size_t)jj * A];
        const double q = rb_q<LOSS, WT>(u, jj, p, s, e, v);
        ++m.n;
        m.n_neg += (jj < h && q > 0.0) ? 1 : 0;
        m.n_pos += (jj > h && q > 0.0) ? 1 : 0;
        m.W += q;
        m.Ss += q * s;
        m.Sp += q * p;
        m.Se += q * e;
    }
    return m;
}

// passes 1 and 2: the weighted terms of a profile at one age, without the division by its own See - what the joint fit
// sums over a segment's profiles (sc_segment_robust.hip) and what rb_solve divides
struct rb_par { double sbar, pbar, beta, ebar, gamma, See, Sep; };

template <int LOSS, bool WT>
__device__ __forceinline__ rb_par rb_terms(const double* prof, const double* u, int np, int h, double de, const double* col,
                                           int A, const rb_prev& v, const rb_mom& m) {
    rb_par t;
    const double sbar = m.Ss / m.W, pbar = m.Sp / m.W, ebar = m.Se / m.W;
    double Sss = 0.0, Sps = 0.0, Ses = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double s = (double)(jj - h) * de, e = col[(size_t)jj * A];
        const double q = rb_q<LOSS, WT>(u, jj, p, s, e, v);
        const double sc = s - sbar;
        Sss += q * (sc * sc);
        Sps += q * (sc * (p - pbar));
        Ses += q * (sc * (e - ebar));
    }
    const double beta = Sps / Sss, gamma = Ses / Sss;
    double See = 0.0, Sep = 0.0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double s = (double)(jj - h) * de, e = col[(size_t)jj * A];
        const double q = rb_q<LOSS, WT>(u, jj, p, s, e, v);
        const double sc = s - sbar;
        const double e2 = (e - ebar) - gamma * sc;
        const double p2 = (p - pbar) - beta * sc;
        See += q * (e2 * e2);
        Sep += q * (e2 * p2);
    }
    t.sbar = sbar; t.pbar = pbar; t.beta = beta; t.ebar = ebar; t.gamma = gamma;
    t.See = See; t.Sep = Sep;
    return t;
}

// ... then the coefficients: (c0, b, a) of the refit into `next`; false where See is not > 0
template <int LOSS, bool WT>
__device__ __forceinline__ bool rb_solve(const double* prof, const double* u, int np, int h, double de, const double* col,
                                         int A, const rb_prev& v, const rb_mom& m, rb_prev& next) {
    const rb_par t = rb_terms<LOSS, WT>(prof, u, np, h, de, col, A, v, m);
    next.a = t.Sep / t.See;
    next.c = v.c;
    pf_slope(t.sbar, t.pbar, t.beta, t.ebar, t.gamma, next.a, next.b, next.c0);
    return t.See > 0.0;
}

// the last pass over the residuals of (c0, b, a): sum u r^2, sum u rho(r) and the points whose factor is < 1
template <int LOSS, bool WT>
__device__ __forceinline__ void rb_loss(const double* prof, const double* u, int np, int h, double de, const double* col, int A,
                                        const rb_prev& v, double& sse, double& loss, int& n_down) {
    sse = 0.0;
    loss = 0.0;
    n_down = 0;
    for (int jj = 0; jj < np; ++jj) {
        const double p = prof[jj];
        if (p != p) continue;
        const double s = (double)(jj - h) * de;
        const double res = rb_resid(p, s, col[(size_t)jj * A], v);
        const double uj = WT ? u[jj] : 1.0;
        sse += uj * (res * res);
        if (LOSS) {
            loss += uj * rb_rho<LOSS>(res, v.c);
            n_down += rb_factor<LOSS>(res, v.c) < 1.0 ? 1 : 0;
        }
    }
    if (!LOSS) loss = sse;
}

// The element of rank `rank` (0-based, ascending) of |r_j| over the profile's points, r the residuals of (c0, b, a) at
// column col: the lanes run over the points, and the answer is built bit by bit from the top on the bit patterns of the
// non-negative doubles (which order as the values do) - cand is kept where at most `rank` values lie below it.  The
// residuals are recomputed in every round; the counts are integers: exact, and the same in every lane.
__device__ __forceinline__ double rb_select(const double* prof, int np, int h, double de, const double* col, int A,
                                            const rb_prev& v, int lane, int rank) {
    unsigned long long best = 0;
    for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long cand = best | (1ull << bit);
        int below = 0;
        for (int j0 = 0; j0 < np; j0 += 64) {
            const int jj = j0 + lane;
            bool lt = false;
            if (jj < np) {
                const double p = prof[jj];
                if (p == p) {
                    const double x = fabs(rb_resid(p, (double)(jj - h) * de, col[(size_t)jj * A], v));
                    lt = (unsigned long long)__double_as_longlong(x) < cand;
                }
            }
            below += __popcll(__ballot(lt));
        }
        if (below <= rank) best = cand;
    }
    return __longlong_as_double((long long)best);
}
