// Dumps csrc/diar_plan.h for tests/test_diarize.py (host compiler only).  One request per line of standard input; the numbers
// after the keyword are the recordings' segment counts n_0 n_1 ... (rec_start is their running sum), but for `start`, whose
// numbers are rec_start itself, and `want`, whose numbers are want:
//   layout <n_0> ...    -> layout <rec_start> <want> <mat_off> <best_v> <best_i> <mats> <total> <matrix 0> <matrix 1> ...   byte offsets
//   check <n_0> ...     -> ok | refused <message>                                       check_rec_start
//   start <s_0> ...     -> ok | refused <message>                                       check_rec_start of n_rec = count - 1 offsets
//   want <w_0> ...      -> ok | refused <message>                                       check_want
//   groups <n_0> ...    -> groups <first> <count> <threads> ...                         plan_groups
//   threads <n>         -> threads <block size>                                         block_threads
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include <iostream>

#include "diar_plan.h"

int main() {
    using namespace xvec::diar_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        std::vector<long long> v;
        for (long long x; in >> x;) v.push_back(x);
        xvec::Refusal why;
        if (what == "start" || what == "check" || what == "layout" || what == "groups") {
            std::vector<int64_t> rs;
            if (what == "start") {
                rs.assign(v.begin(), v.end());
            } else {
                rs.push_back(0);
                for (long long n : v) rs.push_back(rs.back() + n);
            }
            const int32_t n_rec = (int32_t)rs.size() - 1;
            const int bad = check_rec_start(rs.data(), n_rec, why);
            if (what == "start" || what == "check") {
                if (bad) std::printf("refused %s\n", why.text); else std::printf("ok\n");
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
                for (int q = 0; q < n; ++q) std::printf(" %d %d %d", g[q].first, g[q].count, g[q].threads);
                std::printf("\n");
            }
        } else if (what == "want") {
            std::vector<int32_t> w(v.begin(), v.end());
            if (check_want(w.data(), (int32_t)w.size(), why)) std::printf("refused %s\n", why.text); else std::printf("ok\n");
        } else if (what == "threads") {
            if (v.size() != 1) return 2;
            std::printf("threads %d\n", block_threads(v[0]));
        } else {
            return 2;
        }
    }
    return 0;
}
