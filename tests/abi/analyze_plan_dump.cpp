// Dumps csrc/analyze_plan.h for tests/test_analyze.py (host compiler only).  One request per line of standard input:
//   const                                   -> const <threads> <items> <tile> <max blocks> <max bins> <max k> <max cand>
//                                                    <default cand> <hist words> <max copies> <radix> <passes> <part1 bytes>
//                                                    <part2 bytes> <state bytes> <record bytes> <second tile from>
//   grid <n>                                -> grid <tiles> <blocks> <most tiles> <depth>
//   range <b> <tiles> <G>                   -> range <first tile> <end tile>
//   slot <s> <width> <first> <n_bins> <rounding>   -> slot <slot>          (s and width as C reads them: hex floats, inf)
//   copies <n_bins> <asked>                 -> copies <max> <used> <slots> <stride>
//   cap <k> <asked>                         -> cap <cand_cap>
//   shift <p>                               -> shift <bits>
//   summary <n> <n_bins>                    -> summary <part1> <part2> <total> <tiles> <blocks>
//   hardest <n> <k> <cand_cap>              -> hardest <hist> <state> <counts> <offsets> <cand0> <cand1> <total> <tiles> <blocks> <cap>
//   bins <given 0|1> <n_bins> <width> <first> <rounding> <copies> <reserved> <counts 0|1>  -> ok | refused <message>
//   stats <out 0|1>                         -> ok | refused <message>
//   select <given 0|1> <k> <cand_cap>       -> ok | refused <message>
//   lists <nontarget 0|1> <target 0|1> <counts 0|1>  -> ok | refused <message>
//   query <n> <n_bins> <out 0|1>            -> ok | refused <message>
#include <iostream>

#include "analyze_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::analyze_plan;
    std::string line;
    char cells[16];
    void* const P = cells;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why); };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld\n", kThreads, kItems, kTile, kMaxBlocks, kMaxBins,
                        kMaxK, kMaxCand, kDefaultCand, kHistWords, kMaxCopies, kRadix, kPasses, kPart1Bytes, kPart2Bytes, kStateBytes,
                        kRecordBytes, (long long)kSecondTileFrom);
        } else if (q.what == "grid" && q.a.size() == 1) {
            std::printf("grid %lld %lld %lld %lld\n", (long long)tiles_of(q.I(0)), (long long)blocks_of(q.I(0)),
                        (long long)most_tiles(q.I(0)), (long long)sum_depth(q.I(0)));
        } else if (q.what == "range" && q.a.size() == 3) {
            std::printf("range %lld %lld\n", (long long)first_tile(q.I(0), q.I(1), q.I(2)), (long long)first_tile(q.I(0) + 1, q.I(1), q.I(2)));
        } else if (q.what == "slot" && q.a.size() == 5) {
            std::printf("slot %d\n", slot_of(q.D(0), q.D(1), q.I(2), (int32_t)q.I(3), (int32_t)q.I(4)));
        } else if (q.what == "copies" && q.a.size() == 2) {
            const int32_t nb = (int32_t)q.I(0);
            std::printf("copies %d %d %d %d\n", max_copies(nb), copies_of(nb, (int32_t)q.I(1)), slots_of(nb), copy_stride(slots_of(nb)));
        } else if (q.what == "cap" && q.a.size() == 2) {
            std::printf("cap %d\n", cand_cap_of((int32_t)q.I(0), (int32_t)q.I(1)));
        } else if (q.what == "shift" && q.a.size() == 1) {
            std::printf("shift %d\n", shift_after((int)q.I(0)));
        } else if (q.what == "summary" && q.a.size() == 2) {
            const SummaryLayout l = summary_layout(q.I(0), (int32_t)q.I(1));
            std::printf("summary %zu %zu %zu %lld %lld\n", l.part1, l.part2, l.total, (long long)l.tiles, (long long)l.blocks);
        } else if (q.what == "hardest" && q.a.size() == 3) {
            const HardestLayout l = hardest_layout(q.I(0), (int32_t)q.I(1), (int32_t)q.I(2));
            std::printf("hardest %zu %zu %zu %zu %zu %zu %zu %lld %lld %d\n", l.hist, l.state, l.counts, l.offsets, l.cand[0], l.cand[1],
                        l.total, (long long)l.tiles, (long long)l.blocks, l.cap);
        } else if (q.what == "bins" && q.a.size() == 8) {
            xvec_analyze_bins b{};
            b.n_bins = (int32_t)q.I(1);
            b.width = q.D(2);
            b.first = q.I(3);
            b.rounding = (int32_t)q.I(4);
            b.hist_copies = (int32_t)q.I(5);
            b.reserved = (int32_t)q.I(6);
            verdict(check_bins(q.I(0) ? &b : nullptr, q.I(7) ? P : nullptr, why));
        } else if (q.what == "stats" && q.a.size() == 1) {
            verdict(check_stats(q.I(0) ? P : nullptr, why));
        } else if (q.what == "select" && q.a.size() == 3) {
            xvec_analyze_select s{};
            s.k = (int32_t)q.I(1);
            s.cand_cap = (int32_t)q.I(2);
            verdict(check_select(q.I(0) ? &s : nullptr, why));
        } else if (q.what == "lists" && q.a.size() == 3) {
            verdict(check_lists(q.I(0) ? P : nullptr, q.I(1) ? P : nullptr, q.I(2) ? P : nullptr, why));
        } else if (q.what == "query" && q.a.size() == 3) {
            verdict(check_plan_query(q.I(0), (int32_t)q.I(1), q.I(2) ? P : nullptr, why));
        } else {
            return 2;
        }
    }
    return 0;
}
