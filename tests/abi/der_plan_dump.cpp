// Dumps csrc/der_plan.h for tests/test_der.py (host compiler only).  One request per line of standard input:
//   layout <n_0> <n_1> ...          -> layout <rec_start> <blk_start> <ref_mask> <hyp_mask> <noscore> <acc> <ignored> <cooc> <zero_from> <total>
//   check <n_0> <n_1> ...           -> ok | refused <message>       check_rec_start of the recordings' tick counts
//   start <s_0> <s_1> ...           -> ok | refused <message>       check_rec_start of n_rec = count - 1 offsets
//   nullstart <n_rec>               -> ok | refused <message>       check_rec_start of a null pointer
//   counts <m_ref> <m_hyp>          -> ok | refused <message>       check_turn_counts
//   collar <collar>                 -> ok | refused <message>       check_collar
//   turns <0 | 1> <m> <ref | hyp>   -> ok | refused <message>       check_turns of a null (0) or a given (1) pointer
//   blocks <n_0> <n_1> ...          -> blocks <pass blocks> then per block " <rec>:<chunk>:<first tick>:<ticks>"
//   launch <m_ref> <m_hyp> <n_0> .. -> launch <raster blocks> <threads> <pass blocks> <threads> <assign blocks> <threads> <pool blocks> <threads>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "der_plan.h"

int main() {
    using namespace xvec::der_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        xvec::Refusal why;
        auto answer = [&](int bad) { if (bad) std::printf("refused %s\n", why.text); else std::printf("ok\n"); };
        if (what == "turns") {
            int given;
            long long m;
            std::string side;
            if (!(in >> given >> m >> side)) return 2;
            static const int32_t row[4] = {0, 0, 1, 0};
            answer(check_turns(given ? row : nullptr, m, side.c_str(), why));
            continue;
        }
        std::vector<long long> v;
        for (long long x; in >> x;) v.push_back(x);
        if (what == "nullstart") {
            if (v.size() != 1) return 2;
            answer(check_rec_start(nullptr, (int32_t)v[0], why));
        } else if (what == "counts") {
            if (v.size() != 2) return 2;
            answer(check_turn_counts(v[0], v[1], why));
        } else if (what == "collar") {
            if (v.size() != 1) return 2;
            answer(check_collar((int32_t)v[0], why));
        } else if (what == "start" || what == "check" || what == "layout" || what == "blocks" || what == "launch") {
            const size_t skip = what == "launch" ? 2 : 0;
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
            if (what == "start" || what == "check") {
                answer(bad);
            } else if (bad) {
                return 3;
            } else if (what == "layout") {
                const Layout l = make_layout(rs.data(), n_rec);
                std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.rec_start, l.blk_start, l.ref_mask, l.hyp_mask, l.noscore,
                            l.acc, l.ignored, l.cooc, l.zero_from, l.total);
            } else if (what == "blocks") {
                const int64_t n = pass_blocks(rs.data(), n_rec);
                std::printf("blocks %lld", (long long)n);
                for (int64_t b = 0; b < n; ++b) {
                    const Chunk c = block_chunk(rs.data(), n_rec, b);
                    std::printf(" %d:%d:%lld:%d", c.rec, c.chunk, (long long)c.first_tick, c.ticks);
                }
                std::printf("\n");
            } else {
                const Launch r = raster_launch(v[0], v[1]), p = pass_launch(rs.data(), n_rec), a = assign_launch(n_rec), q = pool_launch();
                std::printf("launch %lld %d %lld %d %lld %d %lld %d\n", (long long)r.blocks, r.threads, (long long)p.blocks, p.threads,
                            (long long)a.blocks, a.threads, (long long)q.blocks, q.threads);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
