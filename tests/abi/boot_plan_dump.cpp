// Dumps csrc/boot_plan.h for tests/test_bootstrap.py (host compiler only).  One request per line of standard input:
//   const                                   -> const <threads> <items> <tile> <max groups> <max boot> <magic> <chunk> <max batch>
//                                                    <partials> <counters> <partial bytes> <poisson terms>
//   poisson                                 -> poisson <T_0> <T_1> ...
//   pick <word> <G>                         -> pick <group>
//   pweight <word>                          -> pweight <weight>
//   counts <seed> <b> <side> <G>            -> counts <c[0]> ... <c[G-1]>
//   tweight <seed> <b> <t>                  -> tweight <weight>
//   pack <gr> <gc> <bit>                    -> pack <word> <row> <col> <bit>
//   packi <t> <bit>                         -> packi <word> <index> <bit>
//   batch <n> <n_boot>                      -> batch <size> <count>                                        (0 0: refused)
//   layout <n> <n_boot> <G_0> <G_1>         -> layout <keys0> <keys1> <pay0> <pay1> <hist> <hist_sums> <counters> <tables>
//                                                     <sums> <totals> <eer> <dcf> <below> <total> <batch> <tiles>
//   params <n_boot> <row_group 0|1> <G_0> <col_group 0|1> <G_1> <joint> <c_miss> <c_fa> <p_target>
//                                           -> ok | refused <message>                                      check_params
//   noparams                                -> refused <message>                                           check_params(null)
//   vector <idx 0|1> <row_group 0|1> <col_group 0|1> -> ok | refused <message>                             check_vector_groups
//   outputs <summary 0|1> <records 0|1>     -> ok | refused <message>
//   hcounts <b> <side> <G> <out 0|1>        -> ok | refused <message>
//   hpoisson <b> <t> <out 0|1>              -> ok | refused <message>
//   state <P> <A>                           -> state <0 evaluated | 1 degenerate | 2 overflow>
#include <iostream>
#include <vector>

#include "boot_plan.h"
#include "plan_dump.h"

int main() {
    using namespace xvec::boot_plan;
    std::string line;
    char cells[16];
    const int32_t* const G = reinterpret_cast<const int32_t*>(cells);      // distinct, never followed
    void* const P = cells + 8;
    while (std::getline(std::cin, line)) {
        const plan_dump::Request q(line);
        xvec::Refusal why;
        auto verdict = [&](int bad) { plan_dump::answer(bad, why); };
        auto U = [&](size_t k) { return std::strtoull(q.a.at(k).c_str(), nullptr, 0); };
        if (q.what == "const" && q.a.empty()) {
            std::printf("const %d %d %d %d %d %u %d %d %lld %d %d %d\n", kThreads, kItems, kTile, kMaxGroups, kMaxBoot, kMagic, kChunk,
                        kMaxBatch, (long long)kPartials, kCounters, kPartialBytes, kPoissonTerms);
        } else if (q.what == "poisson" && q.a.empty()) {
            std::printf("poisson");
            for (int i = 0; i < kPoissonTerms; ++i) std::printf(" %u", poisson_threshold(i));
            std::printf("\n");
        } else if (q.what == "pick" && q.a.size() == 2) {
            std::printf("pick %u\n", pick_group((uint32_t)U(0), (uint32_t)U(1)));
        } else if (q.what == "pweight" && q.a.size() == 1) {
            std::printf("pweight %u\n", poisson_weight((uint32_t)U(0)));
        } else if (q.what == "counts" && q.a.size() == 4) {
            const uint32_t g = (uint32_t)U(3);
            std::vector<int> c(g, 0);
            for (uint32_t j = 0; j < g; ++j) ++c[drawn_group(U(0), (uint32_t)U(1), (uint32_t)U(2), j, g)];
            std::printf("counts");
            for (int x : c) std::printf(" %d", x);
            std::printf("\n");
        } else if (q.what == "tweight" && q.a.size() == 3) {
            std::printf("tweight %u\n", trial_poisson(U(0), (uint32_t)U(1), (uint32_t)U(2)));
        } else if (q.what == "pack" && q.a.size() == 3) {
            const uint32_t w = pack_groups((uint32_t)U(0), (uint32_t)U(1), (uint32_t)U(2));
            std::printf("pack %u %u %u %u\n", w, packed_row(w), packed_col(w), packed_bit(w));
        } else if (q.what == "packi" && q.a.size() == 2) {
            const uint32_t w = pack_index((uint32_t)U(0), (uint32_t)U(1));
            std::printf("packi %u %u %u\n", w, packed_index(w), packed_index_bit(w));
        } else if (q.what == "batch" && q.a.size() == 2) {
            std::printf("batch %d %d\n", batch_size(q.I(0), q.I(1)), batch_count(q.I(0), q.I(1)));
        } else if (q.what == "layout" && q.a.size() == 4) {
            const Layout l = make_layout(q.I(0), q.I(1), q.I(2), q.I(3));
            std::printf("layout %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %lld\n", l.keys[0], l.keys[1], l.pay[0],
                        l.pay[1], l.hist, l.hist_sums, l.counters, l.tables, l.sums, l.totals, l.eer, l.dcf, l.below, l.total,
                        l.batch, (long long)l.tiles);
        } else if (q.what == "params" && q.a.size() == 9) {
            xvec_boot_params p{};
            p.n_boot = (int32_t)q.I(0);
            p.row_group = q.I(1) ? G : nullptr;
            p.n_row_groups = (int32_t)q.I(2);
            p.col_group = q.I(3) ? G + 1 : nullptr;
            p.n_col_groups = (int32_t)q.I(4);
            p.joint = (int32_t)q.I(5);
            p.c_miss = q.D(6);
            p.c_fa = q.D(7);
            p.p_target = q.D(8);
            verdict(check_params(&p, why));
        } else if (q.what == "noparams" && q.a.empty()) {
            verdict(check_params(nullptr, why));
        } else if (q.what == "vector" && q.a.size() == 3) {
            xvec_boot_params p{};
            p.row_group = q.I(1) ? G : nullptr;
            p.col_group = q.I(2) ? G + 1 : nullptr;
            verdict(check_vector_groups(q.I(0) ? P : nullptr, &p, why));
        } else if (q.what == "outputs" && q.a.size() == 2) {
            verdict(check_outputs(q.I(0) ? P : nullptr, q.I(1) ? P : nullptr, why));
        } else if (q.what == "hcounts" && q.a.size() == 4) {
            verdict(check_host_counts((int32_t)q.I(0), (int32_t)q.I(1), (int32_t)q.I(2), q.I(3) ? P : nullptr, why));
        } else if (q.what == "hpoisson" && q.a.size() == 3) {
            verdict(check_host_poisson((int32_t)q.I(0), q.I(1), q.I(2) ? P : nullptr, why));
        } else if (q.what == "state" && q.a.size() == 2) {
            std::printf("state %d\n", replicate_state(q.I(0), q.I(1)));
        } else {
            return 2;
        }
    }
    return 0;
}
