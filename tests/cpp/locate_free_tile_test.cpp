// The tile choice of ssw_locate_free_rgb8 (csrc/locate_free_tile.hpp) on the host, no GPU and no context: a sweep over
// enlargement factors 0.3 .. 8 in steps of 1 %, seven suspect shapes, 3 and 4 channels and the nine heights within +-4 of the
// ladder's ph(pw).  Every (suspect, size) that the resize alone has an LDS tile for (pick_resize_tile: what the ladder's
// refinement needs) gets a tile here too, its request within the limit the kernels raise, the patch behind the tile and
// aligned.  The sweep also counts the sizes at which the cheapest tile of the resize alone plus the patch would have passed the
// limit -- whole bands of factors, the one-third thumbnail among them -- so it says what it guards.
// tests/test_locate_free_cpp_cpu.py builds it with hipcc against libssw_hip.so (build_resize_taps) and runs it.
#include <algorithm>
#include <cstdio>

#include "locate_free_tile.hpp"

using namespace ssw;

int main() {
    const unsigned shapes[7][2] = {{240, 166}, {213, 148}, {640, 360}, {300, 200}, {200, 160}, {960, 541}, {47, 33}};
    size_t sizes = 0, tiled = 0, old_rule_refused = 0, largest = 0;
    for (const auto& s : shapes) {
        const unsigned sw = s[0], sh = s[1];
        LadderTaps taps;
        unsigned last_pw = 0;
        for (double f = 0.3; f <= 8.0; f *= 1.01) {
            const unsigned pw = (unsigned)(sw * f + 0.5);
            if (pw < 32 || pw > 4096 || pw == last_pw) continue;
            last_pw = pw;
            const long ph0 = (long)std::max<unsigned long long>(1, (2ull * sh * pw + sw) / (2ull * sw));
            for (long ph = std::max<long>(32, ph0 - 4); ph <= ph0 + 4; ++ph) {
                const bool resized = pw != sw || (unsigned)ph != sh;
                const TapRef vt = taps.get(sh, (size_t)ph), ht = taps.get(sw, pw);
                for (unsigned ch = 3; ch <= 4; ++ch) {
                    ++sizes;
                    ResizeTile alone{}, tl{};
                    size_t alone_lds = 0, lds = 0;
                    unsigned patch_off = 0;
                    const bool has = !resized || pick_resize_tile(vt.shape, ht.shape, pw, (size_t)ph, ch, &alone, &alone_lds);
                    const bool got = free_pick_tile(resized, vt.shape, ht.shape, pw, (unsigned)ph, ch, &tl, &patch_off, &lds);
                    if (has && !got) { std::printf("FAILED: %ux%ux%u -> %ux%ld has a resize tile and no item\n", sw, sh, ch, pw, ph); return 1; }
                    if (!got) continue;
                    ++tiled;
                    largest = std::max(largest, lds);
                    if (lds > RESIZE_LDS_LIMIT || patch_off % 16 || lds != patch_off + free_patch_bytes(tl.oyb, tl.oxb) ||
                        tl.tiles_x != (pw + tl.oxb - 1) / tl.oxb || tl.tiles_y != ((unsigned)ph + tl.oyb - 1) / tl.oyb || tl.oxb != 1u << tl.oxb_log2) {
                        std::printf("FAILED: %ux%ux%u -> %ux%ld: request %zu, patch at %u\n", sw, sh, ch, pw, ph, lds, patch_off);
                        return 1;
                    }
                    if (resized && (alone_lds + 15) / 16 * 16 + free_patch_bytes(alone.oyb, alone.oxb) > RESIZE_LDS_LIMIT) ++old_rule_refused;
                }
            }
        }
    }
    // the one-third thumbnails by name
    for (const auto& c : {std::pair<unsigned, unsigned>{240, 166}, {213, 148}, {640, 360}}) {
        LadderTaps taps;
        ResizeTile tl{};
        size_t lds = 0;
        unsigned off = 0;
        if (!free_pick_tile(true, taps.get(c.second, 3 * c.second).shape, taps.get(c.first, 3 * c.first).shape, 3 * c.first, 3 * c.second, 3, &tl, &off, &lds)) {
            std::printf("FAILED: %ux%u enlarged three times has no item\n", c.first, c.second);
            return 1;
        }
    }
    if (sizes < 30000 || tiled < sizes / 2 || old_rule_refused == 0) { std::printf("FAILED: %zu sizes, %zu tiled, %zu under the old rule\n", sizes, tiled, old_rule_refused); return 1; }
    std::printf("%zu sizes, %zu with a resize tile and every one of those with an item; largest request %zu bytes; %zu of them past the limit had the patch not been counted\n", sizes, tiled, largest, old_rule_refused);
    std::printf("locate_free tiles: ok\n");
    return 0;
}
