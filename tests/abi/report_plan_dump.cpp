// Dumps csrc/report_plan.h for tests/test_report.py (host compiler only).  One request per line of standard input:
//   const                                   -> const <threads> <tile> <range blocks> <range tile> <det items> <det tile> <gap> <chunk> <max planes>
//   tiles <rows> <cols>                     -> tiles <tile rows> <tile cols> <row tiles> <col tiles> <image tiles>
//   wide <cols> <w>                         -> wide <panel> <cell> <first wide column of the panel>
//   piece <a> <b>                           -> piece <body> <tail>
//   step <count> <total> <grid>             -> step <floor(count grid / total)>
//   keep <tp> <nn> <tp_prev> <nn_prev> <P> <N> <grid> <first 0|1> <last 0|1> -> keep <0|1>
//   range <rows> <cols>                     -> range <col tiles> <blocks> <workspace bytes>
//   layout <n> <eval bytes>                 -> layout <state> <eval> <keys> <bits> <row> <col> <tgt> <sums> <keep_sums> <pt_thr>
//                                                     <pt_tp> <pt_nn> <total> <blocks>   (all 0: refused)
//   tmap <n> <arrays 0|1> <rows> <cols> <ld_map> <map offset>  -> ok | refused <message> | toolarge <message>   check_trial_map
//   images <ld> <rows> <cols> <ld_map> <which> <dtype> <null image, -1 none> <image offset> -> ok | refused .. | toolarge ..
//   curve <grid> <header 0|1> <capacity> <arrays 0|1>          -> ok | refused <message>
//   trials <ld> <rows> <cols> <idx 0|1> <n> -> ok | refused <message> | toolarge <message>          check_trials
//   pairs <ld> <rows> <cols>                -> ok | refused <message> | toolarge <message>          check_all_pairs
#include <iostream>

#include "plan_dump.h"
#include "report_plan.h"

int main() {
    using namespace xvec::report_plan;
    std::string line;
    char* const P = reinterpret_cast<char*>(0x1000);      // never followed
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        bool too_large = false;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why, too_large); };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %d %d %d %d\n", kThreads, kTile, kRangeBlocks, kRangeTile, kDetItems, kDetTile, kGap, kChunk,
                        kMaxPlanes);
        } else if (q.what == "tiles" && q.a.size() == 2) {
            std::printf("tiles %lld %lld %lld %lld %lld\n", (long long)tile_rows(q.I(1)), (long long)tile_cols(q.I(1)),
                        (long long)row_tiles(q.I(0), q.I(1)), (long long)col_tiles(q.I(1)), (long long)image_tiles(q.I(0), q.I(1)));
        } else if (q.what == "wide" && q.a.size() == 2) {
            int64_t cell = -1;
            const int panel = wide_panel(q.I(1), q.I(0), &cell);
            std::printf("wide %d %lld %lld\n", panel, (long long)cell, (long long)panel_first(panel, q.I(0)));
        } else if (q.what == "piece" && q.a.size() == 2) {
            const Piece p = split_piece((uint64_t)q.I(0), (uint64_t)q.I(1));
            std::printf("piece %llu %llu\n", (unsigned long long)p.body, (unsigned long long)p.tail);
        } else if (q.what == "step" && q.a.size() == 3) {
            std::printf("step %lld\n", (long long)det_step(q.I(0), q.I(1), q.I(2)));
        } else if (q.what == "keep" && q.a.size() == 9) {
            std::printf("keep %d\n", det_keep(q.I(0), q.I(1), q.I(2), q.I(3), q.I(4), q.I(5), q.I(6), q.I(7) != 0, q.I(8) != 0) ? 1 : 0);
        } else if (q.what == "range" && q.a.size() == 2) {
            std::printf("range %lld %lld %zu\n", (long long)range_col_tiles(q.I(1)), (long long)range_blocks(q.I(0), q.I(1)), range_bytes());
        } else if (q.what == "layout" && q.a.size() == 2) {
            const Layout l = make_layout(q.I(0), (size_t)q.I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", l.state, l.eval, l.keys, l.bits, l.row,
                        l.col, l.tgt, l.sums, l.keep_sums, l.pt_thr, l.pt_tp, l.pt_nn, l.total, (long long)l.blocks);
        } else if (q.what == "tmap" && q.a.size() == 6) {
            void* arr = q.I(1) ? P : nullptr;
            verdict(check_trial_map(arr, arr, arr, q.I(0), q.I(2), q.I(3), P + q.I(5), q.I(4), why, &too_large));
        } else if (q.what == "images" && q.a.size() == 8) {
            void* img[6];
            for (int i = 0; i < 6; ++i) img[i] = i == q.I(6) ? nullptr : P + 0x100 * (i + 1) + q.I(7);
            verdict(check_images(P, q.I(0), q.I(1), q.I(2), P, q.I(3), P, (uint32_t)q.I(4), (int32_t)q.I(5), img, why, &too_large));
        } else if (q.what == "curve" && q.a.size() == 4) {
            void* arr = q.I(3) ? P : nullptr;
            verdict(check_curve(q.I(0), q.I(1) ? P : nullptr, arr, arr, arr, q.I(2), why));
        } else if (q.what == "trials" && q.a.size() == 5) {
            verdict(check_trials(P, q.I(0), q.I(1), q.I(2), q.I(3) ? P : nullptr, q.I(3) ? P : nullptr, P, q.I(4), why, &too_large));
        } else if (q.what == "pairs" && q.a.size() == 3) {
            verdict(check_all_pairs(P, q.I(0), q.I(1), q.I(2), P, P, why, &too_large));
        } else {
            return 2;
        }
    }
    return 0;
}
