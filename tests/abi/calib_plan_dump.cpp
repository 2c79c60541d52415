// Dumps csrc/calib_plan.h for tests/test_calibrate.py (host compiler only).  One request per line of standard input:
//   const                                  -> const <threads> <items> <max blocks> <chunk> <final> <hull tile> <partial words>
//   blocks <n>                             -> blocks <pass blocks> <sum depth>
//   hull <n>                               -> hull <levels> <groups 1> <span 1> ... <groups L> <span L> | refused
//   layout <n> <eval bytes>                -> layout <state> <partials> <fit_scores> <fit_bits> <eval> <keys> <bits> <points>
//                                                    <block_counts> <group_counts> <total> <hull blocks>   (all 0: refused)
//   trials <ld> <rows> <cols> <idx 0|1> <n> -> ok | refused <message> | toolarge <message>          check_trials
//   pairs <ld> <rows> <cols>               -> ok | refused <message> | toolarge <message>          check_all_pairs
//   fit <p_target> <max_iter>              -> ok | refused <message>
//   costs <c_miss> <c_fa> <p_target>       -> ok | refused <message>
//   apply <ld> <rows> <cols> <ld_out> <in place 0|1> -> ok | refused <message> | toolarge <message>
//   segments <capacity> <arrays 0|1>       -> ok | refused <message>
#include <iostream>

#include "calib_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::calib_plan;
    std::string line;
    void* const P = reinterpret_cast<void*>(0x1000);      // never followed
    void* const Q = reinterpret_cast<void*>(0x2000);
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        bool too_large = false;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why, too_large); };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %d %d\n", kThreads, kItems, kMaxBlocks, kChunk, kFinal, kHullTile, kPartialWords);
        } else if (q.what == "blocks" && q.a.size() == 1) {
            std::printf("blocks %lld %lld\n", (long long)pass_blocks(q.I(0)), (long long)sum_depth(q.I(0)));
        } else if (q.what == "hull" && q.a.size() == 1) {
            HullPlan h;
            if (plan_hull(q.I(0), &h)) {
                std::printf("refused\n");
            } else {
                std::printf("hull %d", h.levels);
                for (int l = 1; l <= h.levels; ++l) std::printf(" %lld %lld", (long long)h.groups[l], (long long)h.span[l]);
                std::printf("\n");
            }
        } else if (q.what == "layout" && q.a.size() == 2) {
            const Layout l = make_layout(q.I(0), (size_t)q.I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", l.state, l.partials, l.fit_scores, l.fit_bits,
                        l.eval, l.keys, l.bits, l.points, l.block_counts, l.group_counts, l.total, (long long)l.hull_blocks);
        } else if (q.what == "trials" && q.a.size() == 5) {
            verdict(check_trials(P, q.I(0), q.I(1), q.I(2), q.I(3) ? P : nullptr, q.I(3) ? P : nullptr, P, q.I(4), why, &too_large));
        } else if (q.what == "pairs" && q.a.size() == 3) {
            verdict(check_all_pairs(P, q.I(0), q.I(1), q.I(2), P, P, why, &too_large));
        } else if (q.what == "fit" && q.a.size() == 2) {
            verdict(check_fit(q.D(0), (int32_t)q.I(1), why));
        } else if (q.what == "costs" && q.a.size() == 3) {
            verdict(check_costs(q.D(0), q.D(1), q.D(2), why));
        } else if (q.what == "apply" && q.a.size() == 5) {
            verdict(check_apply(P, q.I(0), q.I(1), q.I(2), P, q.I(4) ? P : Q, q.I(3), why, &too_large));
        } else if (q.what == "segments" && q.a.size() == 2) {
            void* arr = q.I(1) ? P : nullptr;
            verdict(check_segments(arr, arr, arr, arr, q.I(0), why));
        } else {
            return 2;
        }
    }
    return 0;
}
