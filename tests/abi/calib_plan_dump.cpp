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
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "calib_plan.h"

int main() {
    using namespace xvec::calib_plan;
    std::string line;
    void* const P = reinterpret_cast<void*>(0x1000);      // never followed
    void* const Q = reinterpret_cast<void*>(0x2000);
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        std::vector<std::string> a;
        for (std::string x; in >> x;) a.push_back(x);
        auto I = [&](size_t k) { return std::strtoll(a.at(k).c_str(), nullptr, 10); };
        auto D = [&](size_t k) { return std::strtod(a.at(k).c_str(), nullptr); };
        xvec::Refusal why;
        bool too_large = false;
        auto verdict = [&](int bad) {
            if (bad) std::printf("%s %s\n", too_large ? "toolarge" : "refused", why.text); else std::printf("ok\n");
        };
        if (what == "const" && a.empty()) {
            std::printf("const %d %d %d %d %d %d %d\n", kThreads, kItems, kMaxBlocks, kChunk, kFinal, kHullTile, kPartialWords);
        } else if (what == "blocks" && a.size() == 1) {
            std::printf("blocks %lld %lld\n", (long long)pass_blocks(I(0)), (long long)sum_depth(I(0)));
        } else if (what == "hull" && a.size() == 1) {
            HullPlan h;
            if (plan_hull(I(0), &h)) {
                std::printf("refused\n");
            } else {
                std::printf("hull %d", h.levels);
                for (int l = 1; l <= h.levels; ++l) std::printf(" %lld %lld", (long long)h.groups[l], (long long)h.span[l]);
                std::printf("\n");
            }
        } else if (what == "layout" && a.size() == 2) {
            const Layout l = make_layout(I(0), (size_t)I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", l.state, l.partials, l.fit_scores, l.fit_bits,
                        l.eval, l.keys, l.bits, l.points, l.block_counts, l.group_counts, l.total, (long long)l.hull_blocks);
        } else if (what == "trials" && a.size() == 5) {
            verdict(check_trials(P, I(0), I(1), I(2), I(3) ? P : nullptr, I(3) ? P : nullptr, P, I(4), why, &too_large));
        } else if (what == "pairs" && a.size() == 3) {
            verdict(check_all_pairs(P, I(0), I(1), I(2), P, P, why, &too_large));
        } else if (what == "fit" && a.size() == 2) {
            verdict(check_fit(D(0), (int32_t)I(1), why));
        } else if (what == "costs" && a.size() == 3) {
            verdict(check_costs(D(0), D(1), D(2), why));
        } else if (what == "apply" && a.size() == 5) {
            verdict(check_apply(P, I(0), I(1), I(2), P, I(4) ? P : Q, I(3), why, &too_large));
        } else if (what == "segments" && a.size() == 2) {
            void* arr = I(1) ? P : nullptr;
            verdict(check_segments(arr, arr, arr, arr, I(0), why));
        } else {
            return 2;
        }
    }
    return 0;
}
