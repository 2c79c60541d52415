// Dumps csrc/vad_plan.h for tests/test_vad.py (host compiler only).  One request per line of standard input:
//   window <L> <cmn_window> <min_window> <center>  -> window <lo_0> <hi_0> <lo_1> <hi_1> ...        every frame t of L
//   span <cmn_window> <min_window> <center>        -> span <frames>                                  (span off: no normalisation)
//   tile <C> <span>                                -> tile <frames> <channels> <rows> <lds bytes> <run> | refused
//   grid <B> <T> <C> <span>                        -> grid <blocks>
//   layout <B> <T>                                 -> layout <prefix> <count> <total>                byte offsets
//   shape <B> <T> <C> <row stride> <utt stride>    -> ok | refused <message>                         check_shape
//   maskstride <stride> <T>                        -> ok | refused <message>
//   vad <thr> <scale> <prop> <ctx> <col> <C>       -> ok | refused <message>                         check_vad (vad null: null)
//   cmvn <cmn_window> <min_window>                 -> ok | refused <message>                         check_cmvn
#include <iostream>

#include "plan_dump.h"
#include "vad_plan.h"

int main() {
    using namespace xvec::vad_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why); };
        if (q.what == "window" && q.a.size() == 4) {
            std::printf("window");
            for (int t = 0; t < (int)q.I(0); ++t) {
                int lo, hi;
                window(t, (int)q.I(0), (int)q.I(1), (int)q.I(2), (int)q.I(3), &lo, &hi);
                std::printf(" %d %d", lo, hi);
            }
            std::printf("\n");
        } else if (q.what == "span" && q.a.size() == 1 && q.a[0] == "off") {
            std::printf("span %d\n", span(nullptr));
        } else if (q.what == "span" && q.a.size() == 3) {
            const xvec_cmvn_options o{(int32_t)q.I(0), (int32_t)q.I(1), (int32_t)q.I(2), 0};
            std::printf("span %d\n", span(&o));
        } else if (q.what == "tile" && q.a.size() == 2) {
            Tile t{};
            if (plan_tile((int32_t)q.I(0), (int32_t)q.I(1), &t)) std::printf("refused\n");
            else std::printf("tile %d %d %d %zu %d\n", t.frames, t.channels, t.rows, t.lds_bytes, t.run);
        } else if (q.what == "grid" && q.a.size() == 4) {
            Tile t{};
            if (plan_tile((int32_t)q.I(2), (int32_t)q.I(3), &t)) return 3;
            std::printf("grid %lld\n", (long long)grid_blocks((int32_t)q.I(0), (int32_t)q.I(1), (int32_t)q.I(2), t));
        } else if (q.what == "layout" && q.a.size() == 2) {
            const Layout l = make_layout((int32_t)q.I(0), (int32_t)q.I(1));
            std::printf("layout %zu %zu %zu\n", l.prefix, l.count, l.total);
        } else if (q.what == "shape" && q.a.size() == 5) {
            verdict(check_shape((int32_t)q.I(0), (int32_t)q.I(1), (int32_t)q.I(2), q.I(3), q.I(4), "x:", why));
        } else if (q.what == "maskstride" && q.a.size() == 2) {
            verdict(check_mask_stride(q.I(0), (int32_t)q.I(1), why));
        } else if (q.what == "vad" && q.a.size() == 1 && q.a[0] == "null") {
            verdict(check_vad(nullptr, 1, why));
        } else if (q.what == "vad" && q.a.size() == 6) {
            const xvec_vad_options o{q.D(0), q.D(1), q.D(2), (int32_t)q.I(3), (int32_t)q.I(4)};
            verdict(check_vad(&o, (int32_t)q.I(5), why));
        } else if (q.what == "cmvn" && q.a.size() == 2) {
            const xvec_cmvn_options o{(int32_t)q.I(0), (int32_t)q.I(1), 0, 0};
            verdict(check_cmvn(&o, why));
        } else {
            return 2;
        }
    }
    return 0;
}
