// Dumps csrc/tsne_plan.h for tests/test_tsne.py (host compiler only).  One request per line of standard input:
//   plan <n> <cus>            -> plan <rows> <slices> <slice_cols> <groups>                                      make_plan
//   layout <n> <d>            -> layout <x64> <sqnorm> <row_sum> <scalars> <partials> <kl_part> <norm_part> <total>
//                                <max_slices> <update_blocks>                                                    byte offsets
//   points <n>                -> ok | refused <message>                                                          check_points
//   perplexity <value> <n>    -> ok | refused <message>                                                          check_perplexity
//   steps <components> <steps> <exaggeration> <momentum> <learning rate> <min gain>  -> ok | refused <message>   check_steps
#include <iostream>

#include "plan_dump.h"
#include "tsne_plan.h"

int main() {
    using namespace xvec::tsne_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why); };
        if (q.what == "plan" && q.a.size() == 2) {
            const Plan p = make_plan(q.I(0), q.I(1));
            std::printf("plan %d %d %d %d\n", p.rows, p.slices, p.slice_cols, p.groups);
        } else if (q.what == "layout" && q.a.size() == 2) {
            const Layout l = make_layout(q.I(0), q.I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", l.x64, l.sqnorm, l.row_sum, l.scalars, l.partials, l.kl_part,
                        l.norm_part, l.total, max_slices(q.I(0)), update_blocks(q.I(0)));
        } else if (q.what == "points" && q.a.size() == 1) {
            verdict(check_points(q.I(0), why));
        } else if (q.what == "perplexity" && q.a.size() == 2) {
            verdict(check_perplexity(q.D(0), q.I(1), why));
        } else if (q.what == "steps" && q.a.size() == 6) {
            verdict(check_steps(q.I(0), q.I(1), q.D(2), q.D(3), q.D(4), q.D(5), why));
        } else {
            return 2;
        }
    }
    return 0;
}
