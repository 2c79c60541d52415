// Dumps csrc/vbx_plan.h for tests/test_vbx.py (host compiler only).  One request per line of standard input:
//   layout <dim> <n_spk> <n_0> ...  -> layout <rec_start> <rho> <g> <em> <fw> <c> <mx> <raw> <model> <total>     byte offsets
//   check <n_0> <n_1> ...           -> ok | refused <message>       check_rec_start of the recordings' frame counts
//   start <s_0> <s_1> ...           -> ok | refused <message>       check_rec_start of n_rec = count - 1 offsets
//   shape <dim> <n_spk>             -> ok | refused <message>       check_shape
//   options <loop_prob> <Fa> <Fb> <epsilon> <max_iter>              -> ok | refused <message>       check_options
//   launch <n_frames> <n_rec>       -> launch <run blocks> <run threads> <init blocks> <init threads>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vbx_plan.h"

int main() {
    using namespace xvec::vbx_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        xvec::Refusal why;
        if (what == "options") {
            std::string lp, fa, fb, eps;
            int max_iter;
            if (!(in >> lp >> fa >> fb >> eps >> max_iter)) return 2;
            xvec_vbx_options o{std::strtod(lp.c_str(), nullptr), std::strtod(fa.c_str(), nullptr), std::strtod(fb.c_str(), nullptr),
                               std::strtod(eps.c_str(), nullptr), max_iter, 0};
            if (check_options(&o, why)) std::printf("refused %s\n", why.text); else std::printf("ok\n");
            continue;
        }
        std::vector<long long> v;
        for (long long x; in >> x;) v.push_back(x);
        if (what == "shape") {
            if (v.size() != 2) return 2;
            if (check_shape((int32_t)v[0], (int32_t)v[1], why)) std::printf("refused %s\n", why.text); else std::printf("ok\n");
        } else if (what == "launch") {
            if (v.size() != 2) return 2;
            const Launch run = run_launch((int32_t)v[1]), init = init_launch(v[0], (int32_t)v[1]);
            std::printf("launch %lld %d %lld %d\n", (long long)run.blocks, run.threads, (long long)init.blocks, init.threads);
        } else if (what == "start" || what == "check" || what == "layout") {
            const size_t skip = what == "layout" ? 2 : 0;
            if (v.size() < skip) return 2;
            std::vector<int64_t> rs;
            if (what == "start") {
                rs.assign(v.begin(), v.end());
            } else {
                rs.push_back(0);
                for (size_t i = skip; i < v.size(); ++i) rs.push_back(rs.back() + v[i]);
            }
            const int32_t n_rec = (int32_t)rs.size() - 1;
            const int bad = check_rec_start(rs.data(), n_rec, why);
            if (what != "layout") {
                if (bad) std::printf("refused %s\n", why.text); else std::printf("ok\n");
            } else if (bad || check_shape((int32_t)v[0], (int32_t)v[1], why)) {
                return 3;
            } else {
                const Layout l = make_layout(rs.data(), n_rec, (int32_t)v[0], (int32_t)v[1]);
                std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.rec_start, l.rho, l.g, l.em, l.fw, l.c, l.mx, l.raw,
                            l.model, l.total);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
