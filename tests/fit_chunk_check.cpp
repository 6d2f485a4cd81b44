// The segment-chunk rule of the fit drivers (scarplet_amd/csrc/sc_fit_chunk.h) on the host: g++ -std=c++17
// -fsanitize=address,undefined, a program of its own (tests/test_fit_chunks_host.py builds it, feeds it and checks
// what it prints against a restatement of the rule in Python).
// stdin:  cases, each "n S max_segs max_cells has_aux max_aux" (n: option "fit_chunk", the cells are bounded by
//         sc_fit_chunk_bound(max_cells, n)), then the S + 1 entries of seg_start and - has_aux - the S + 1 entries of
//         the second CSR array
// stdout: per case one line, the chunk boundaries 0 = s_0 < s_1 < ... = S
#include "../scarplet_amd/csrc/sc_fit_chunk.h"
#include <cstdio>
#include <vector>

int main() {
    long long S, max_segs, max_cells, max_aux, n;
    int has_aux;
    while (std::scanf("%lld %lld %lld %lld %d %lld", &n, &S, &max_segs, &max_cells, &has_aux, &max_aux) == 6) {
        std::vector<long long> seg((size_t)S + 1), aux((size_t)S + 1);
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
        }
        std::printf("\n");
    }
    return 0;
}
