// Dumps csrc/score_tiles.h for tests/test_score_tiles.py (host compiler only).  One request per line of standard input:
//   rc <tiles_m> <tiles_n>               -> rc <tiles_m> <tiles_n> r0 c0 r1 c1 ...       tile_rc of t = 0 .. tiles_m tiles_n - 1
//   sym <T>                              -> sym <T> r0 c0 r1 c1 ...                      tile_rc_sym of t = 0 .. T (T + 1) / 2 - 1
//   rule <M> <N> <K> <sym> <pre> <cus>   -> rule <tile edge>                             gemm_tile_size
#include <cstdio>
#include <cstring>

#include "score_tiles.h"

int main() {
    using namespace xvec::score_tiles;
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "rc")) {
            int tm, tn;
            if (std::scanf("%d %d", &tm, &tn) != 2) return 2;
            std::printf("rc %d %d", tm, tn);
            for (int t = 0; t < tm * tn; ++t) {
                int r = -1, c = -1;
                tile_rc(t, tm, tn, r, c);
                std::printf(" %d %d", r, c);
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "sym")) {
            int T;
            if (std::scanf("%d", &T) != 1) return 2;
            std::printf("sym %d", T);
            for (int t = 0; t < T * (T + 1) / 2; ++t) {
                int r = -1, c = -1;
                tile_rc_sym(t, T, r, c);
                std::printf(" %d %d", r, c);
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "rule")) {
            long long M, N;
            int K, sym, pre, cus;
            if (std::scanf("%lld %lld %d %d %d %d", &M, &N, &K, &sym, &pre, &cus) != 6) return 2;
            std::printf("rule %d\n", gemm_tile_size(M, N, K, sym != 0, pre != 0, cus));
        } else {
            return 2;
        }
    }
    return 0;
}
