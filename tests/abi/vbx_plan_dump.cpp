// Dumps csrc/vbx_plan.h for tests/test_vbx.py (host compiler only).  One request per line of standard input:
//   layout <dim> <n_spk> <n_0> ...  -> layout <rec_start> <rho> <g> <em> <fw> <c> <mx> <raw> <model> <total>     byte offsets
//   check <n_0> <n_1> ...           -> ok | refused <message>       check_rec_start of the recordings' frame counts
//   start <s_0> <s_1> ...           -> ok | refused <message>       check_rec_start of n_rec = count - 1 offsets
//   nullstart <n_rec>               -> ok | refused <message>       check_rec_start of a null pointer
//   shape <dim> <n_spk>             -> ok | refused <message>       check_shape
//   options <loop_prob> <Fa> <Fb> <epsilon> <max_iter>              -> ok | refused <message>       check_options
//   launch <n_frames> <n_rec>       -> launch <run blocks> <run threads> <init blocks> <init threads>
#include <iostream>

#include "plan_dump.h"
#include "vbx_plan.h"

int main() {
    using namespace xvec::vbx_plan;
    using plan_dump::answer;
    std::string line;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        const std::string& what = q.what;
        xvec::Refusal why;
        if (what == "options") {
            if (q.a.size() != 5) return 2;
            xvec_vbx_options o{q.D(0), q.D(1), q.D(2), q.D(3), (int32_t)q.I(4), 0};
            answer(check_options(&o, why), why);
        } else if (what == "shape") {
            if (q.a.size() != 2) return 2;
            answer(check_shape((int32_t)q.I(0), (int32_t)q.I(1), why), why);
        } else if (what == "nullstart") {
            if (q.a.size() != 1) return 2;
            answer(check_rec_start(nullptr, (int32_t)q.I(0), why), why);
        } else if (what == "launch") {
            if (q.a.size() != 2) return 2;
            const Launch run = run_launch((int32_t)q.I(1)), init = init_launch(q.I(0), (int32_t)q.I(1));
            std::printf("launch %lld %d %lld %d\n", (long long)run.blocks, run.threads, (long long)init.blocks, init.threads);
        } else if (what == "start" || what == "check" || what == "layout") {
            const size_t lead = what == "layout" ? 2 : 0;
            if (q.a.size() < lead) return 2;
            const std::vector<int64_t> rs = q.rec_start(lead);
            const int32_t n_rec = (int32_t)rs.size() - 1;
            const int bad = check_rec_start(rs.data(), n_rec, why);
            if (what != "layout") {
                answer(bad, why);
            } else if (bad || check_shape((int32_t)q.I(0), (int32_t)q.I(1), why)) {
                return 3;
            } else {
                const Layout l = make_layout(rs.data(), n_rec, (int32_t)q.I(0), (int32_t)q.I(1));
                std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.rec_start, l.rho, l.g, l.em, l.fw, l.c, l.mx, l.raw,
                            l.model, l.total);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
