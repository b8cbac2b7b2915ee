// The list of k_sweep instantiations and the pick of csrc/sweep_variant.hpp, printed for tests/sweep_variant_cases.py:
//   "entry <index> <mode> <order> <f32> <round> <resid> <pitch>"   one line per entry of the list, then
//   "pick <index>"                                                 one line per "<mode> <order> <f32> <residus> <pitch>"
// read from stdin (-1: the pick is not in the list).  Host compiler only; no expectation of its own -- the rules are
// restated in sweep_variant_rules.cpp, the rows that must reach every entry in tests/sweep_variant_cases.py.
#include <cstdio>

#include "../../euispice_coreg_amd/csrc/sweep_variant.hpp"

using namespace sweep_variant;

int main() {
    for (int i = 0; i < kSweepVariants.n; ++i) {
        const SweepVariant& v = kSweepVariants.v[i];
        std::printf("entry %d %d %d %d %d %d %d\n", i, v.mode, v.order, (int)v.f32, (int)v.round, (int)v.resid, v.pitch);
    }
    int mode, order, f32, residus, pitch;
    while (std::scanf("%d %d %d %d %d", &mode, &order, &f32, &residus, &pitch) == 5)
        std::printf("pick %d\n", sweep_variant_index(pick_sweep_variant(mode, order, f32 != 0, residus != 0, pitch)));
    return 0;
}
