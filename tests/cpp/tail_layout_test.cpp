// Host-side print-out of the tail layout of a pruned base reader's row pass (csrc/dct_pair_class.hpp): for every
// "W:tile48" on the command line, the eight level-2 row classes as pair_class_args answers them for the fused forward row pass
// (class-major, level 2, 128-frequency tiles), and per tile column the column tiles lo .. hi it writes, computed as the gated
// row launches compute them (dct_pair_f64_kernel.hpp, SUB == 5).  tests/test_tail_layout_cpu.py compares the lines with its
// own restatement, from which the GPU tests take every expected counter.  No GPU, no context.
//   L <W> <tile48> <split bytes of the bound kernel's bases>
//   P <eligible> <pair0> <NP> <chunks>                       what base_tail_plan answers for the pass
//   C <class index> <NP> <Kp> <tiles_n> <bn32> <gsh> <e2off> <lo:hi of tile column 0> <lo:hi of tile column 1> ...
// A pass the plan does not take has no tail: zeros in L and P, no lo:hi in C.
#include <cstdio>
#include <cstdlib>
#include "../../spread_spectrum_watermarking_amd/csrc/ssw_internal.hpp"
#include "../../spread_spectrum_watermarking_amd/csrc/dct_pair_common.hpp"

using namespace ssw;

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: tail_layout_test W:tile48 ...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        unsigned w = 0, tile48 = 0;
        if (std::sscanf(argv[i], "%u:%u", &w, &tile48) != 2 || w % 128 != 0) { std::printf("FAIL bad argument %s\n", argv[i]); return 2; }
        PairLayout lay;
        lay.class_major = true; lay.rows_l2 = true; lay.tile = 128;
        BaseTailPlan plan;
        const int prc = base_tail_plan(w, lay, tile48 != 0, plan);
        if (prc != SSW_OK) { std::printf("FAIL plan at %u: status %d\n", w, prc); return 1; }
        for (int c = 0; c < 8; ++c) {
            PairClassArgs ca;
            PairInstance inst;
            const int rc = pair_class_args(kLevel2Classes[c], true, false, w, lay, false, false, tile48 != 0, ca, inst);
            if (rc != SSW_OK) { std::printf("FAIL class %d at %u: status %d\n", c, w, rc); return 1; }
            const unsigned tw = plan.pair0;          // the width of a tile column = the first tail pair
            if (c == 0) {
                std::printf("L %u %u %zu\n", w, tile48, plan.eligible ? base_energy_split_bytes(ca.NP, ca.Kp, tw) : (size_t)0);
                std::printf("P %d %u %u %u\n", plan.eligible ? 1 : 0, plan.pair0, plan.NP, plan.chunks);
            }
            std::printf("C %d %u %u %u %u %u %u", c, ca.NP, ca.Kp, ca.tiles_n, ca.bn32, ca.gsh, ca.e2off);
            for (unsigned tn = 0; plan.eligible && tn < ca.tiles_n; ++tn) {
                // (the kernel's words; its launches start at tile column 1, where pf >= e2off)
                const unsigned pf = tn * tw, pl = pf + tw - 1u < ca.NP ? pf + tw - 1u : ca.NP - 1u;
                const unsigned lo = (pf - (tn ? ca.e2off : 0u)) >> ca.gsh, hi = pl >> ca.gsh;
                std::printf(" %u:%u", lo, hi);
            }
            std::printf("\n");
        }
    }
    return 0;
}
