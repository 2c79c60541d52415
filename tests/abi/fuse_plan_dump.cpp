// Dumps csrc/fuse_plan.h for tests/test_fuse.py (host compiler only).  One request per line of standard input:
//   const                                   -> const <max terms> <threads> <items> <max blocks> <state bytes> <gather counts>
//                                                    <matrix> <row> <col> <converged> <max iter> <one class> <inf score>
//   words <k>                               -> words <pass words> <gather words> <partial stride> <term ulps>
//   hess <k>                                -> hess <word of (0,0)> <word of (1,0)> <word of (1,1)> ... <word of (k,k)>
//   blocks <n>                              -> blocks <pass blocks> <sum depth>
//   layout <n> <k>                          -> layout <state> <partials> <planes> <fit_bits> <total>            (all 0: refused)
//   terms <k> <cols> <kind> <ld> <data 0|1> -> ok | refused <message>     check_terms; the LAST of the k terms is <kind> <ld>
//                                              <data>, the ones before it MATRIX terms of row stride <cols>
//   trials <k> <rows> <cols> <idx 0|1> <n>  -> ok | refused <message> | toolarge <message>          check_fit_trials
//   pairs <k> <rows> <cols>                 -> ok | refused <message> | toolarge <message>          check_fit_all_pairs
//   fit <p_target> <max_iter>               -> ok | refused <message>
//   ridge <l2>                              -> ok | refused <message>
//   apply <k> <rows> <cols> <ld_out> <out: -1 its own | t the data of term t> <kind of term 0> <ld of term 0>
//                                           -> ok | refused <message> | toolarge <message>          check_fuse_apply
#include <iostream>

#include "fuse_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::fuse_plan;
    std::string line;
    char cells[16];
    auto ptr = [&](int k) { return reinterpret_cast<const double*>(cells + k); };      // distinct, never followed
    void* const P = cells + 12;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        bool too_large = false;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why, too_large); };
        xvec_fuse_term t[kMaxTerms + 2];
        auto fill = [&](long long k, long long cols) {
            for (int i = 0; i < kMaxTerms + 2; ++i) t[i] = xvec_fuse_term{ptr(i), cols, XVEC_FUSE_MATRIX};
            return (int32_t)k;
        };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %d %d %d %d %d %d %d %d\n", kMaxTerms, kThreads, kItems, kMaxBlocks, kStateBytes,
                        kGatherCounts, XVEC_FUSE_MATRIX, XVEC_FUSE_ROW, XVEC_FUSE_COL, XVEC_FUSE_CONVERGED, XVEC_FUSE_MAX_ITER,
                        XVEC_FUSE_ONE_CLASS, XVEC_FUSE_INF_SCORE);
        } else if (q.what == "words" && q.a.size() == 1) {
            const int k = (int)q.I(0);
            std::printf("words %d %d %d %d\n", pass_words(k), gather_words(k), partial_stride(k), term_ulps(k));
        } else if (q.what == "hess" && q.a.size() == 1) {
            const int k = (int)q.I(0);
            std::printf("hess");
            for (int i = 0; i <= k; ++i)
                for (int j = 0; j <= i; ++j) std::printf(" %d", hess_word(k, i, j));
            std::printf("\n");
        } else if (q.what == "blocks" && q.a.size() == 1) {
            std::printf("blocks %lld %lld\n", (long long)pass_blocks(q.I(0)), (long long)sum_depth(q.I(0)));
        } else if (q.what == "layout" && q.a.size() == 2) {
            const Layout l = make_layout(q.I(0), q.I(1));
            std::printf("layout %zu %zu %zu %zu %zu\n", l.state, l.partials, l.planes, l.fit_bits, l.total);
        } else if (q.what == "terms" && q.a.size() == 5) {
            const int32_t k = fill(q.I(0), q.I(1));
            if (k >= 1 && k <= kMaxTerms + 2) t[k - 1] = xvec_fuse_term{q.I(4) ? ptr(k - 1) : nullptr, q.I(3), (int32_t)q.I(2)};
            verdict(check_terms(t, k, q.I(1), why));
        } else if (q.what == "trials" && q.a.size() == 5) {
            const int32_t k = fill(q.I(0), q.I(2));
            verdict(check_fit_trials(t, k, q.I(1), q.I(2), q.I(3) ? P : nullptr, q.I(3) ? P : nullptr, P, q.I(4), why, &too_large));
        } else if (q.what == "pairs" && q.a.size() == 3) {
            const int32_t k = fill(q.I(0), q.I(2));
            verdict(check_fit_all_pairs(t, k, q.I(1), q.I(2), P, P, why, &too_large));
        } else if (q.what == "fit" && q.a.size() == 2) {
            verdict(check_fit(q.D(0), (int32_t)q.I(1), why));
        } else if (q.what == "ridge" && q.a.size() == 1) {
            verdict(check_ridge(q.D(0), why));
        } else if (q.what == "apply" && q.a.size() == 7) {
            const int32_t k = fill(q.I(0), q.I(2));
            t[0].kind = (int32_t)q.I(5);
            t[0].ld = q.I(6);
            const void* out = q.I(4) < 0 ? P : static_cast<const void*>(t[q.I(4)].data);
            verdict(check_fuse_apply(t, k, q.I(1), q.I(2), P, out, q.I(3), why, &too_large));
        } else {
            return 2;
        }
    }
    return 0;
}
