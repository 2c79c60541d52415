// Dumps csrc/resample_taps.h for tests/test_resample.py (host compiler only, built with -ffp-contract=off).  One request per line
// of standard input, doubles as the 16 hex digits of their bits:
//   ratio <ratio bits> <precision>                          -> ratio <inc bits> <scale bits> <step> <scaled 0|1>
//   len <n> <ratio bits>                                    -> len <n_out>
//   span <ratio bits> <precision> <nwin> <tile>             -> span <tile_span>
//   taps <t0> <t1> <ratio bits> <precision> <nwin> <n>      -> for every t in [t0, t1) one line:
//                                                              tap <t> <n0> <off_l> <eta_l bits> <i_min> <i_max> <off_r> <eta_r bits> <k_max>
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "resample_taps.h"

static double from_bits(uint64_t u) {
    double x;
    std::memcpy(&x, &u, sizeof(x));
    return x;
}

static uint64_t to_bits(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

int main() {
    using namespace xvec::resample_taps;
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "ratio")) {
            uint64_t u;
            int precision;
            if (std::scanf("%" SCNx64 " %d", &u, &precision) != 2) return 2;
            const RatioPlan r = plan_ratio(from_bits(u), 1 << precision);
            std::printf("ratio %016" PRIx64 " %016" PRIx64 " %d %d\n", to_bits(r.inc), to_bits(r.scale), r.step, r.scaled);
        } else if (!std::strcmp(what, "len")) {
            long long n;
            uint64_t u;
            if (std::scanf("%lld %" SCNx64, &n, &u) != 2) return 2;
            std::printf("len %lld\n", (long long)out_len(n, from_bits(u)));
        } else if (!std::strcmp(what, "span")) {
            uint64_t u;
            int precision, tile;
            long long nwin;
            if (std::scanf("%" SCNx64 " %d %lld %d", &u, &precision, &nwin, &tile) != 4) return 2;
            const RatioPlan r = plan_ratio(from_bits(u), 1 << precision);
            if (r.step < 1) return 2;
            std::printf("span %lld\n", (long long)tile_span(r, nwin, tile));
        } else if (!std::strcmp(what, "taps")) {
            long long t0, t1, nwin, n;
            uint64_t u;
            int precision;
            if (std::scanf("%lld %lld %" SCNx64 " %d %lld %lld", &t0, &t1, &u, &precision, &nwin, &n) != 6) return 2;
            const RatioPlan r = plan_ratio(from_bits(u), 1 << precision);
            if (r.step < 1) return 2;
            for (long long t = t0; t < t1; ++t) {
                const TapPlan p = plan_output(t, r, 1 << precision, nwin, n);
                std::printf("tap %lld %lld %d %016" PRIx64 " %lld %lld %d %016" PRIx64 " %lld\n", t, (long long)p.n0, p.off_l,
                            to_bits(p.eta_l), (long long)p.i_min, (long long)p.i_max, p.off_r, to_bits(p.eta_r), (long long)p.k_max);
            }
        } else {
            return 2;
        }
    }
    return 0;
}
