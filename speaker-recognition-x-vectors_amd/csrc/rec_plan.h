// What the units that work on a batch of recordings share on the host: clustering (diar_plan.h), VBx (vbx_plan.h) and DER
// scoring (der_plan.h).  The one check of rec_start, with one text per refusal, so that the three units cannot drift apart in
// what they accept, and the record of a launch.  Host-compilable (no HIP header), like the plan headers that forward to it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "plan_support.h"

namespace xvec {
namespace rec_plan {

// What a unit's recordings are made of, and how many of them one recording may have.
struct Rule {
    const char* noun;      // "segment", "frame", "tick"
    int32_t cap;           // per recording; 0 = none
    const char* cap_name;  // the cap's macro, as the text names it
};

// rec_start [n_rec + 1]: from 0, every recording with 1 .. rule.cap of the unit's noun, fewer than 2^31 in all.
// 0, or 1 with the reason in why.
inline int check_rec_start(const int64_t* rs, int32_t n_rec, const Rule& rule, Refusal& why) {
    if (n_rec < 1) return why.refuse("n_rec = %d: need at least one recording", n_rec);
    if (!rs) return why.refuse("null pointer: rec_start");
    if (rs[0] != 0) return why.refuse("rec_start must begin at 0 (got %lld)", (long long)rs[0]);
    for (int32_t r = 0; r < n_rec; ++r) {
        const int64_t n = rs[r + 1] - rs[r];
        if (n < 1)
            return why.refuse("recording %d is empty or rec_start decreases: every recording needs a %s", r, rule.noun);
        if (rule.cap && n > rule.cap)
            return why.refuse("recording %d has %lld %ss, more than %s = %d", r, (long long)n, rule.noun, rule.cap_name, rule.cap);
        if (rs[r + 1] > 0x7fffffff)
            return why.refuse("%lld %ss up to recording %d: the total must stay below 2^31", (long long)rs[r + 1], rule.noun, r);
    }
    return 0;
}

// One launch of a unit's plan.
struct Launch {
    int64_t blocks;
    int32_t threads;
};

}  // namespace rec_plan
}  // namespace xvec
