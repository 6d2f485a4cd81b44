// The segment-chunk rule of the fit drivers and the host arrays of a chunk (scarplet_amd/csrc/sc_fit_chunk.h) on the
// host: g++ -std=c++17 -fsanitize=address,undefined, a program of its own (tests/test_fit_chunks_host.py builds it, feeds
// it and checks what it prints against a restatement in Python).
// fit_chunk_check [arrays]
//   stdin:  cases, each "n S max_segs max_cells has_aux max_aux" (n: option "fit_chunk", the cells are bounded by
//           sc_fit_chunk_bound(max_cells, n)), then the S + 1 entries of seg_start and - has_aux - the S + 1 entries of
//           the second CSR array
//   stdout: per case one line, the chunk boundaries 0 = s_0 < s_1 < ... = S; with `arrays`, after it "totals" with the
//           CSR array of the block totals over the case's segments (sc_fit_block_totals), and then five lines per chunk:
//           "G" and the number of blocks, "start", "blk", "cseg" and "dir" with the entries of the chunk's CSR array over
//           its cells, of the CSR array of blocks over its segments, of the segment of every cell and of the interleaved
//           (sa, ca), where cell k of the case has sa = k and ca = -(k + 1)
// fit_chunk_check cap
//   stdin:  lines "max_park prof planes C shift";  stdout: per line sc_fit_park_cap of it
#include "../scarplet_amd/csrc/sc_fit_chunk.h"
#include <cstdio>
#include <cstring>
#include <vector>

template <class T>
static void print(const char* name, const std::vector<T>& v) {
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "cap")) {
        long long max_park, prof, planes, C;
        int shift;
        while (std::scanf("%lld %lld %lld %lld %d", &max_park, &prof, &planes, &C, &shift) == 5)
            std::printf("%lld\n", sc_fit_park_cap(max_park, prof, planes, C, shift != 0));
        return 0;
    }
    const bool arrays = argc > 1 && !std::strcmp(argv[1], "arrays");
    long long S, max_segs, max_cells, max_aux, n;
    int has_aux;
    while (std::scanf("%lld %lld %lld %lld %d %lld", &n, &S, &max_segs, &max_cells, &has_aux, &max_aux) == 6) {
        std::vector<long long> seg((size_t)S + 1), aux((size_t)S + 1), cuts(1, 0);
        for (auto& v : seg)
            if (std::scanf("%lld", &v) != 1) return 2;
        if (has_aux)
            for (auto& v : aux)
                if (std::scanf("%lld", &v) != 1) return 2;
        std::printf("0");
        for (long long s0 = 0; s0 < S;) {
            s0 = sc_fit_chunk_end(seg.data(), s0, S, max_segs, sc_fit_chunk_bound(max_cells, n), has_aux ? aux.data() : nullptr,
                                  max_aux);
            std::printf(" %lld", s0);
            cuts.push_back(s0);
        }
        std::printf("\n");
        if (!arrays) continue;
        std::vector<double> sa((size_t)seg[S]), ca((size_t)seg[S]), dir;
        for (long long k = 0; k < seg[S]; ++k) {
            sa[k] = (double)k;
            ca[k] = (double)(-(k + 1));
        }
        std::vector<int> start, cseg, blk;
        std::vector<long long> totals;
        sc_fit_block_totals(seg.data(), S, totals);
        print("totals", totals);
        for (size_t c = 0; c + 1 < cuts.size(); ++c) {
            const long long s0 = cuts[c], s1 = cuts[c + 1];
            sc_fit_chunk_start(seg.data(), s0, s1, start);
            sc_fit_chunk_dir(sa.data(), ca.data(), seg[s0], seg[s1] - seg[s0], dir);
            std::printf("G %lld\n", sc_fit_chunk_blocks(seg.data(), s0, s1, cseg, blk));
            print("start", start);
            print("blk", blk);
            print("cseg", cseg);
            print("dir", dir);
        }
    }
    return 0;
}
