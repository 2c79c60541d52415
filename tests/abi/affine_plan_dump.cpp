// Dumps csrc/affine_plan.h for tests/test_affine_plan.py (host compiler only).  One request per line of standard input:
//   <M> <N> <K> <vec16_ok> <out_ok> <scratch_floats> <have_w3>
//     -> <form> <S> <trips_per_range> <s_pad> <grid_x> <grid_y> <trips> lo0 hi0 lo1 hi1 ...
// where [lo, hi) are the trips of range s = 0 .. S - 1 exactly as the kernels of csrc/affine.hip cut them:
// lo = s * trips_per_range, hi = min(trips, lo + trips_per_range).
#include <cstdio>

#include "affine_plan.h"

int main() {
    using namespace xvec::affine_plan;
    long long M, N, K, scratch;
    int vec16, out_ok, w3;
    while (std::scanf("%lld %lld %lld %d %d %lld %d", &M, &N, &K, &vec16, &out_ok, &scratch, &w3) == 7) {
        const Plan p = plan((int)M, (int)N, (int)K, vec16 != 0, out_ok != 0, scratch, w3 != 0);
        const long long trips = (K + kTripK - 1) / kTripK;
        std::printf("%d %d %d %d %lld %lld %lld", p.form, p.S, p.trips_per_range, p.s_pad, (long long)p.grid_x,
                    (long long)p.grid_y, trips);
        for (int s = 0; s < p.S; ++s) {
            const long long lo = (long long)s * p.trips_per_range;
            const long long hi = lo + p.trips_per_range < trips ? lo + p.trips_per_range : trips;
            std::printf(" %lld %lld", lo, hi);
        }
        std::printf("\n");
    }
    return 0;
}
