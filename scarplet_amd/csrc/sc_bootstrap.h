// What sc_bootstrap_segments* (sc_bootstrap.hip) and sc_channel_bootstrap* (sc_channel_bootstrap.hip) share
// (docs/bootstrap.md; docs/channels.md, "Intervals per reach"): the shape of the launches, the generator of the draws, the
// sums of a replicate in draw order, the checks of the block arrays and the launch of k_bs_terms.
#pragma once
#include "sc_fit.h"

#define BS_RUN 64                        // usable profiles per run of a block's sum: sc_fit_segments' SG_BLOCK
#define BS_WAVES 4
#define BS_THREADS (64 * BS_WAVES)
#define BS_TILE 16                       // replicates a wave takes of one work item: 64 per workgroup
#define BS_LDS_MAX 65536                 // a segment's block terms go to LDS up to this many bytes
#define BS_MAX_GRID 8192
#define BS_MAX_OUT (1ll << 26)           // (segment, replicate) pairs of a chunk: 0.6 GB of indices and amplitudes
#define BS_MAX_SEGS (1ll << 20)

// the splitmix64 finaliser
__host__ __device__ __forceinline__ unsigned long long bs_mix(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the key of a segment's draws
__device__ __forceinline__ unsigned long long bs_key(unsigned long long seed, int label) {
    return bs_mix(seed ^ ((unsigned long long)(unsigned)label * 0x9E3779B97F4A7C15ull));
}

// whether a segment of nb blocks and m usable profiles is bootstrapped
__device__ __forceinline__ bool bs_boot(int nb, int m, int min_blocks, int min_profiles) {
    return nb >= min_blocks && m >= min_profiles;
}

// The sums of one replicate over its drawn blocks, in draw order; T: the segment's block terms, nb rows of A.  The ONE place
// where the draws are formed: both bootstraps call it.  COUNT (sc_channel_bootstrap.hip, profile mode): M is the sum of
// cnt[block] - the usable profiles of the segment's blocks - over the same draws; else cnt is not read and M stays 0
template <bool COUNT>
__device__ __forceinline__ void bs_sums_counted(const double2* T, const int* __restrict__ cnt, int nb, int A, int ia, int lane,
                                                int r, unsigned long long key, double& S, double& P, int& M) {
    S = 0.0;
    P = 0.0;
    M = 0;
    if (r == 0) {                                        // the anchor: every block once
        for (int k = 0; k < nb; ++k) {
            const double2 v = T[(size_t)k * A + ia];
            S += v.x;
            P += v.y;
            if (COUNT) M += cnt[k];
        }
        return;
    }
    for (int k0 = 0; k0 < nb; k0 += 64) {
        // 64 draws at once, one per lane (a lane past the end forms a draw nobody reads)
        const unsigned long long u = bs_mix(key + (((unsigned long long)(unsigned)r << 32) | (unsigned)(k0 + lane)));
        const int b = (int)(((u >> 32) * (unsigned long long)(unsigned)nb) >> 32);
        const int nk = min(64, nb - k0);
        for (int j = 0; j < nk; ++j) {
            const int bj = __builtin_amdgcn_readlane(b, j);          // (< nb: the product's high word)
            const double2 v = T[(size_t)bj * A + ia];
            S += v.x;
            P += v.y;
            if (COUNT) M += cnt[bj];
        }
    }
}

__device__ __forceinline__ void bs_sums(const double2* T, int nb, int A, int ia, int lane, int r, unsigned long long key,
                                        double& S, double& P) {
    int M;
    bs_sums_counted<false>(T, nullptr, nb, A, ia, lane, r, key, S, P, M);
}

// ---- sc_bootstrap.hip, shared with sc_channel_bootstrap.hip ---------------------------------------------------------------------
static inline unsigned bs_grid(long long n) { return (unsigned)(n < 1 ? 1 : n > BS_MAX_GRID ? BS_MAX_GRID : n); }
// the rules of R, level and min_blocks and of the CSR arrays of blocks over segments and of cells over blocks
int sc_bs_check(sc_ctx* ctx, const char* who, long long K, const long long* seg_start, long long S,
                const long long* seg_blk_start, const long long* blk_start, long long NB, int min_blocks, int R, double level);
// k_bs_terms on two neighbouring planes of the chunk's park (NB >= 1 blocks, blk their CSR array over the chunk's cells):
// (sum x_ci, sum y_ci) per block and column into terms
void sc_bs_terms_launch(sc_ctx* ctx, const int* used, const double* x, const double* y, const int* blk, long long NB, int A,
                        double2* terms);
