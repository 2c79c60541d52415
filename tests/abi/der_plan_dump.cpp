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
#include <iostream>

#include "der_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::der_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        const std::string& what = q.what;
        xvec::Refusal why;
        auto answer = [&](int bad) { plan_dump::answer(bad, why); };
        if (what == "turns") {
            if (q.a.size() != 3) return 2;
            static const int32_t row[4] = {0, 0, 1, 0};
            answer(check_turns(q.I(0) ? row : nullptr, q.I(1), q.a[2].c_str(), why));
        } else if (what == "nullstart") {
            if (q.a.size() != 1) return 2;
            answer(check_rec_start(nullptr, (int32_t)q.I(0), why));
        } else if (what == "counts") {
            if (q.a.size() != 2) return 2;
            answer(check_turn_counts(q.I(0), q.I(1), why));
        } else if (what == "collar") {
            if (q.a.size() != 1) return 2;
            answer(check_collar((int32_t)q.I(0), why));
        } else if (what == "start" || what == "check" || what == "layout" || what == "blocks" || what == "launch") {
            const size_t lead = what == "launch" ? 2 : 0;
            if (q.a.size() < lead) return 2;
            const std::vector<int64_t> rs = q.rec_start(lead);
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
                const Launch r = raster_launch(q.I(0), q.I(1)), p = pass_launch(rs.data(), n_rec), a = assign_launch(n_rec), q = pool_launch();
                std::printf("launch %lld %d %lld %d %lld %d %lld %d\n", (long long)r.blocks, r.threads, (long long)p.blocks, p.threads,
                            (long long)a.blocks, a.threads, (long long)q.blocks, q.threads);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
