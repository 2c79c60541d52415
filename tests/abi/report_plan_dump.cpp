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
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "report_plan.h"

int main() {
    using namespace xvec::report_plan;
    std::string line;
    char* const P = reinterpret_cast<char*>(0x1000);      // never followed
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) return 2;
        std::vector<std::string> a;
        for (std::string x; in >> x;) a.push_back(x);
        auto I = [&](size_t k) { return std::strtoll(a.at(k).c_str(), nullptr, 10); };
        xvec::Refusal why;
        bool too_large = false;
        auto verdict = [&](int bad) {
            if (bad) std::printf("%s %s\n", too_large ? "toolarge" : "refused", why.text); else std::printf("ok\n");
        };
        if (what == "const" && a.empty()) {
            std::printf("const %d %d %d %d %d %d %d %d %d\n", kThreads, kTile, kRangeBlocks, kRangeTile, kDetItems, kDetTile, kGap, kChunk,
                        kMaxPlanes);
        } else if (what == "tiles" && a.size() == 2) {
            std::printf("tiles %lld %lld %lld %lld %lld\n", (long long)tile_rows(I(1)), (long long)tile_cols(I(1)),
                        (long long)row_tiles(I(0), I(1)), (long long)col_tiles(I(1)), (long long)image_tiles(I(0), I(1)));
        } else if (what == "wide" && a.size() == 2) {
            int64_t cell = -1;
            const int panel = wide_panel(I(1), I(0), &cell);
            std::printf("wide %d %lld %lld\n", panel, (long long)cell, (long long)panel_first(panel, I(0)));
        } else if (what == "piece" && a.size() == 2) {
            const Piece p = split_piece((uint64_t)I(0), (uint64_t)I(1));
            std::printf("piece %llu %llu\n", (unsigned long long)p.body, (unsigned long long)p.tail);
        } else if (what == "step" && a.size() == 3) {
            std::printf("step %lld\n", (long long)det_step(I(0), I(1), I(2)));
        } else if (what == "keep" && a.size() == 9) {
            std::printf("keep %d\n", det_keep(I(0), I(1), I(2), I(3), I(4), I(5), I(6), I(7) != 0, I(8) != 0) ? 1 : 0);
        } else if (what == "range" && a.size() == 2) {
            std::printf("range %lld %lld %zu\n", (long long)range_col_tiles(I(1)), (long long)range_blocks(I(0), I(1)), range_bytes());
        } else if (what == "layout" && a.size() == 2) {
            const Layout l = make_layout(I(0), (size_t)I(1));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", l.state, l.eval, l.keys, l.bits, l.row,
                        l.col, l.tgt, l.sums, l.keep_sums, l.pt_thr, l.pt_tp, l.pt_nn, l.total, (long long)l.blocks);
        } else if (what == "tmap" && a.size() == 6) {
            void* arr = I(1) ? P : nullptr;
            verdict(check_trial_map(arr, arr, arr, I(0), I(2), I(3), P + I(5), I(4), why, &too_large));
        } else if (what == "images" && a.size() == 8) {
            void* img[6];
            for (int i = 0; i < 6; ++i) img[i] = i == I(6) ? nullptr : P + 0x100 * (i + 1) + I(7);
            verdict(check_images(P, I(0), I(1), I(2), P, I(3), P, (uint32_t)I(4), (int32_t)I(5), img, why, &too_large));
        } else if (what == "curve" && a.size() == 4) {
            void* arr = I(3) ? P : nullptr;
            verdict(check_curve(I(0), I(1) ? P : nullptr, arr, arr, arr, I(2), why));
        } else if (what == "trials" && a.size() == 5) {
            verdict(check_trials(P, I(0), I(1), I(2), I(3) ? P : nullptr, I(3) ? P : nullptr, P, I(4), why, &too_large));
        } else if (what == "pairs" && a.size() == 3) {
            verdict(check_all_pairs(P, I(0), I(1), I(2), P, P, why, &too_large));
        } else {
            return 2;
        }
    }
    return 0;
}
