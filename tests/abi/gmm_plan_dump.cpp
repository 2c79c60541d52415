// Dumps csrc/gmm_plan.h for tests/test_gmm.py (host compiler only).  One request per line of standard input:
//   const                                          -> const <threads> <frame tile> <comp tile> <col tile> <k chunk> <lds stride>
//                                                           <max C> <max D> <max utts> <max slices> <max iter> <target blocks>
//                                                           <min slice frames> <em state bytes>
//   plan <n_total> <U> <C> <D> <per_utt> <n_slices> -> plan <comp tiles> <col tiles> <slices> <slice frames> <k pad> <k chunks>
//                                                           <slab doubles>
//   loglik <U> <C> <D>                             -> loglik <first> <off> <P> <g> <total>
//   acc <n_total> <U> <C> <D> <per_utt> <n_slices> -> acc <first> <off> <P> <g> <lse> <slab> <total> <slices>
//   em <n_total> <U> <C> <D> <n_slices>            -> em <n> <f> <s> <sums> <state> <total>
//   score <M> <U> <C> <D>                          -> score <model> <test> <total>
//   model <C> <D>                                  -> ok | refused <message>
//   frames <given> <x> <x_type> <reserved> <rows> <ldx> <D> <arrays 0|1> <first count>...   -> ok <n_total> | refused <message>
//   slices <per_utt> <n_slices>                    -> ok | refused <message>
//   options <given> <reg_covar> <var_floor> <min_count>   -> ok | refused <message>
//   iter <max_iter> <tol>                          -> ok | refused <message>
//   map <M> <relevance>                            -> ok | refused <message>
//   scores <M> <U> <ld_s>                          -> ok | refused <message>
//   query <n_total> <U> <C> <D> <per_utt> <n_slices> <out 0|1>   -> ok | refused <message>
#include <iostream>

#include "gmm_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::gmm_plan;
    std::string line;
    char cells[16];
    void* const P = cells;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why); };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %d %d %d %lld %d %d %d %d %d\n", kThreads, kFT, kCT, kYT, kKC, kLD, kMaxC, kMaxD,
                        (long long)kMaxUtts, kMaxSlices, kMaxIter, kTargetBlocks, kMinSliceFrames, kEmStateBytes);
        } else if (q.what == "plan" && q.a.size() == 6) {
            const int32_t C = (int32_t)q.I(2), D = (int32_t)q.I(3);
            const bool per = q.I(4) != 0;
            const int32_t sl = per ? 0 : slices_of(q.I(0), C, D, (int32_t)q.I(5));
            std::printf("plan %d %d %d %lld %d %d %zu\n", comp_tiles(C), y_tiles(D, per), sl, (long long)(per ? 0 : slice_frames(q.I(0), sl)),
                        k_pad(D), k_chunks(D), per ? (size_t)0 : slab_doubles(C, D, sl));
        } else if (q.what == "loglik" && q.a.size() == 3) {
            const Layout l = loglik_layout(q.I(0), (int32_t)q.I(1), (int32_t)q.I(2));
            std::printf("loglik %zu %zu %zu %zu %zu\n", l.first, l.off, l.P, l.g, l.total);
        } else if (q.what == "acc" && q.a.size() == 6) {
            const Layout l = accumulate_layout(q.I(0), q.I(1), (int32_t)q.I(2), (int32_t)q.I(3), (int32_t)q.I(4), (int32_t)q.I(5));
            std::printf("acc %zu %zu %zu %zu %zu %zu %zu %d\n", l.first, l.off, l.P, l.g, l.lse, l.slab, l.total, l.slices);
        } else if (q.what == "em" && q.a.size() == 5) {
            const Layout l = em_layout(q.I(0), q.I(1), (int32_t)q.I(2), (int32_t)q.I(3), (int32_t)q.I(4));
            std::printf("em %zu %zu %zu %zu %zu %zu\n", l.n, l.f, l.s, l.sums, l.state, l.total);
        } else if (q.what == "score" && q.a.size() == 4) {
            const ScoreLayout l = score_layout(q.I(0), q.I(1), (int32_t)q.I(2), (int32_t)q.I(3));
            std::printf("score %zu %zu %zu\n", l.model, l.test, l.total);
        } else if (q.what == "model" && q.a.size() == 2) {
            verdict(check_model((int32_t)q.I(0), (int32_t)q.I(1), why));
        } else if (q.what == "frames" && q.a.size() >= 8 && q.a.size() % 2 == 0) {
            std::vector<int64_t> first, count;
            for (size_t k = 8; k < q.a.size(); k += 2) {
                first.push_back(q.I(k));
                count.push_back(q.I(k + 1));
            }
            xvec_gmm_frames f{};
            f.x = q.I(1) ? P : nullptr;
            f.x_type = (int32_t)q.I(2);
            f.reserved = (int32_t)q.I(3);
            f.rows = q.I(4);
            f.ldx = q.I(5);
            f.utt_first = q.I(7) ? first.data() : nullptr;
            f.utt_count = q.I(7) ? count.data() : nullptr;
            f.n_utts = (int64_t)first.size();
            int64_t total = -1;
            const int bad = check_frames(q.I(0) ? &f : nullptr, (int32_t)q.I(6), &total, why);
            if (bad) verdict(bad);
            else std::printf("ok %lld\n", (long long)total);
        } else if (q.what == "slices" && q.a.size() == 2) {
            verdict(check_slices((int32_t)q.I(0), (int32_t)q.I(1), why));
        } else if (q.what == "options" && q.a.size() == 4) {
            xvec_gmm_mstep_options o{q.D(1), q.D(2), q.D(3)};
            verdict(check_options(q.I(0) ? &o : nullptr, why));
        } else if (q.what == "iter" && q.a.size() == 2) {
            verdict(check_em((int32_t)q.I(0), q.D(1), why));
        } else if (q.what == "map" && q.a.size() == 2) {
            verdict(check_map(q.I(0), q.D(1), why));
        } else if (q.what == "scores" && q.a.size() == 3) {
            verdict(check_scores(q.I(0), q.I(1), q.I(2), why));
        } else if (q.what == "query" && q.a.size() == 7) {
            verdict(check_plan_query(q.I(0), q.I(1), (int32_t)q.I(2), (int32_t)q.I(3), (int32_t)q.I(4), (int32_t)q.I(5), q.I(6) ? P : nullptr, why));
        } else {
            return 2;
        }
    }
    return 0;
}
