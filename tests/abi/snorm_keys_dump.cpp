// Dumps csrc/snorm_keys.h for tests/test_snorm.py (host compiler only).  One request per line of standard input, doubles as
// the 16 hex digits of their bits:
//   key <bits>                   -> key <nan 0|1> <key hex> <bits of the key's value, hex>      (key and value 0 for a NaN)
//   digits <key hex>             -> digits d0 d1 ... d7                                          digit_of, pass 0 first
//   select <k> <n> <bits> ...    -> select <cut key hex> <n_above>                               select_kth_host over cell_key
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "snorm_keys.h"

int main() {
    using namespace xvec::snorm_keys;
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "key")) {
            uint64_t u;
            if (std::scanf("%" SCNx64, &u) != 1) return 2;
            const bool nan = is_nan_bits(u);
            const uint64_t k = nan ? 0 : key_of_bits(u);
            std::printf("key %d %016" PRIx64 " %016" PRIx64 "\n", nan ? 1 : 0, k, nan ? 0 : bits_of_key(k));
        } else if (!std::strcmp(what, "digits")) {
            uint64_t k;
            if (std::scanf("%" SCNx64, &k) != 1) return 2;
            std::printf("digits");
            for (int p = 0; p < kPasses; ++p) std::printf(" %u", digit_of(k, p));
            std::printf("\n");
        } else if (!std::strcmp(what, "select")) {
            uint32_t k, n;
            if (std::scanf("%u %u", &k, &n) != 2) return 2;
            std::vector<uint64_t> keys(n);
            for (uint32_t i = 0; i < n; ++i) {
                uint64_t u;
                if (std::scanf("%" SCNx64, &u) != 1) return 2;
                keys[i] = cell_key(value_of_bits(u), false);
            }
            uint32_t above = 0;
            const uint64_t cut = select_kth_host(keys.data(), n, k, &above);
            std::printf("select %016" PRIx64 " %u\n", cut, above);
        } else {
            return 2;
        }
    }
    return 0;
}
