// Dumps csrc/diar_plan.h for tests/test_diarize.py (host compiler only).  One request per line of standard input; the numbers
// after the keyword are the recordings' segment counts n_0 n_1 ... (rec_start is their running sum), but for `start`, whose
// numbers are rec_start itself, and `want`, whose numbers are want:
//   layout <n_0> ...    -> layout <rec_start> <want> <mat_off> <best_v> <best_i> <mats> <total> <matrix 0> <matrix 1> ...   byte offsets
//   check <n_0> ...     -> ok | refused <message>                                       check_rec_start
//   start <s_0> ...     -> ok | refused <message>                                       check_rec_start of n_rec = count - 1 offsets
//   nullstart <n_rec>   -> ok | refused <message>                                       check_rec_start of a null pointer
//   want <w_0> ...      -> ok | refused <message>                                       check_want
//   groups <n_0> ...    -> groups <first> <count> <threads> ...                         plan_groups
//   threads <n>         -> threads <block size>                                         block_threads
#include <iostream>

#include "diar_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::diar_plan;
    using plan_dump::answer;
    std::string line;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        const std::string& what = q.what;
        xvec::Refusal why;
        if (what == "start" || what == "check" || what == "layout" || what == "groups") {
            const std::vector<int64_t> rs = q.rec_start();
            const int32_t n_rec = (int32_t)rs.size() - 1;
            const int bad = check_rec_start(rs.data(), n_rec, why);
            if (what == "start" || what == "check") {
                answer(bad, why);
            } else if (bad) {
                return 3;
            } else if (what == "layout") {
                const Layout l = make_layout(rs.data(), n_rec);
                std::printf("layout %zu %zu %zu %zu %zu %zu %zu", l.rec_start, l.want, l.mat_off, l.best_v, l.best_i, l.mats, l.total);
                for (int32_t r = 0; r < n_rec; ++r) std::printf(" %zu", matrix_offset(l, rs.data(), r));
                std::printf("\n");
            } else {
                Group g[2];
                const int n = plan_groups(rs.data(), n_rec, g);
                std::printf("groups");
                for (int k = 0; k < n; ++k) std::printf(" %d %d %d", g[k].first, g[k].count, g[k].threads);
                std::printf("\n");
            }
        } else if (what == "nullstart") {
            if (q.a.size() != 1) return 2;
            answer(check_rec_start(nullptr, (int32_t)q.I(0), why), why);
        } else if (what == "want") {
            std::vector<int32_t> w;
            for (size_t k = 0; k < q.a.size(); ++k) w.push_back((int32_t)q.I(k));
            answer(check_want(w.data(), (int32_t)w.size(), why), why);
        } else if (what == "threads") {
            if (q.a.size() != 1) return 2;
            std::printf("threads %d\n", block_threads(q.I(0)));
        } else {
            return 2;
        }
    }
    return 0;
}
