// Dumps csrc/tsne_plan.h for tests/test_tsne.py (host compiler only).  One request per line of standard input:
//   plan <n> <cus>            -> plan <rows> <slices> <slice_cols> <groups>                                      make_plan
//   layout <n> <d>            -> layout <x64> <sqnorm> <row_sum> <scalars> <partials> <kl_part> <norm_part> <total>
//                                <max_slices> <update_blocks>                                                    byte offsets
//   points <n>                -> ok | refused <message>                                                          check_points
//   perplexity <value> <n>    -> ok | refused <message>                                                          check_perplexity
//   steps <components> <steps> <exaggeration> <momentum> <learning rate> <min gain>  -> ok | refused <message>   check_steps
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tsne_plan.h"

int main() {
    using namespace xvec::tsne_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        std::vector<std::string> a;
        for (std::string x; in >> x;) a.push_back(x);
        auto I = [&](size_t k) { return (int32_t)std::strtoll(a.at(k).c_str(), nullptr, 10); };
        auto D = [&](size_t k) { return std::strtod(a.at(k).c_str(), nullptr); };      // (reads "nan" and "inf" too)
        xvec::Refusal why;
        auto verdict = [&](int bad) {
            if (bad) std::printf("refused %s\n", why.text); else std::printf("ok\n");
        };
        if (what == "plan" && a.size() == 2) {
            const Plan p = make_plan(I(0), I(1));
            std::printf("plan %d %d %d %d\n", p.rows, p.slices, p.slice_cols, p.groups);
        } else if (what == "layout" && a.size() == 2) {
            const Layout l = make_layout(I(0), I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", l.x64, l.sqnorm, l.row_sum, l.scalars, l.partials, l.kl_part,
                        l.norm_part, l.total, max_slices(I(0)), update_blocks(I(0)));
        } else if (what == "points" && a.size() == 1) {
            verdict(check_points(I(0), why));
        } else if (what == "perplexity" && a.size() == 2) {
            verdict(check_perplexity(D(0), I(1), why));
        } else if (what == "steps" && a.size() == 6) {
            verdict(check_steps(I(0), I(1), D(2), D(3), D(4), D(5), why));
        } else {
            return 2;
        }
    }
    return 0;
}
