// What free_pick_tile (csrc/locate_free_tile.hpp) chooses for the (suspect, size) items somebody else lists: no GPU and no
// context.  Standard input: one item per line, `sw sh channels pw ph` (the suspect's shape and the size it is scored at; the
// item is the plain front when pw x ph is the suspect's own size, as make_item of locate_free.hip decides).  Standard output,
// one line per item in the same order: `oyb oxb tiles_x tiles_y lds`, or `none` for a size that has no tile.
// tests/test_locate_free_hard_cpu.py builds it with hipcc against libssw_hip.so (build_resize_taps) and hands it the items of
// tests/locate_free_cases.py.
#include <cstdio>

#include "locate_free_tile.hpp"

using namespace ssw;

int main() {
    LadderTaps taps;
    unsigned sw, sh, ch, pw, ph;
    while (std::scanf("%u %u %u %u %u", &sw, &sh, &ch, &pw, &ph) == 5) {
        if (!sw || !sh || !pw || !ph || (ch != 3 && ch != 4)) { std::printf("bad line\n"); return 1; }
        const bool resized = pw != sw || ph != sh;
        TapRef vt{}, ht{};
        if (resized) { vt = taps.get(sh, ph); ht = taps.get(sw, pw); }
        ResizeTile tl{};
        unsigned patch_off = 0;
        size_t lds = 0;
        if (!free_pick_tile(resized, vt.shape, ht.shape, pw, ph, ch, &tl, &patch_off, &lds)) { std::printf("none\n"); continue; }
        std::printf("%u %u %u %u %zu\n", tl.oyb, tl.oxb, tl.tiles_x, tl.tiles_y, lds);
    }
    return 0;
}
