// The tile of locate_free_kernel (locate_free.hip) and the LDS it asks for, shared with tests/cpp/locate_free_tile_test.cpp:
// the window of the original's luma plane lies behind the fused resize tile of resize_common.hpp, so the tile is chosen with
// the window counted -- a size that the resize alone has a tile for always gets one here.
#pragma once

#include "resize_common.hpp"

namespace ssw {

constexpr unsigned FREE_NEAR = 4;                         // positions within +-4 of the ladder's
constexpr unsigned FREE_SIDE = 2 * FREE_NEAR + 1;         // 9
constexpr unsigned FREE_POS = FREE_SIDE * FREE_SIDE;      // 81 sums per item
constexpr unsigned FREE_PLAIN_OYB = 32, FREE_PLAIN_OXB_LOG2 = 6;      // the tile of the suspect's own size

// words of a patch row: the tile's own + the 8 bytes the window adds (the last window of word k ends in byte 4 k + 11: word k + 2)
__host__ __device__ inline unsigned free_patch_words(unsigned oxb) { return oxb / 4 + 2; }
__host__ __device__ inline unsigned free_patch_bytes(unsigned oyb, unsigned oxb) { return (oyb + 2 * FREE_NEAR) * free_patch_words(oxb) * 4; }
// what the patch adds to a tile's LDS: itself and the alignment of its start to 16
inline size_t free_patch_extra(unsigned oyb, unsigned oxb) { return (size_t)free_patch_bytes(oyb, oxb) + 15; }

// The tile of one (suspect, size): resized (vt, ht: the tap shapes of sh -> ph and sw -> pw) or the suspect's own size.
// *patch_off: bytes of dynamic LDS in front of the patch (a multiple of 16), *lds: the whole request.  false: no tile.
inline bool free_pick_tile(bool resized, const DeviceTaps& vt, const DeviceTaps& ht, unsigned pw, unsigned ph, unsigned ch, ResizeTile* tl,
                           unsigned* patch_off, size_t* lds) {
    size_t front = 0;
    if (resized) {
        if (!pick_resize_tile(vt, ht, pw, ph, ch, tl, &front, 0, 2, free_patch_extra)) return false;
    } else {
        const unsigned oyb = FREE_PLAIN_OYB, oxb = 1u << FREE_PLAIN_OXB_LOG2;
        *tl = ResizeTile{oyb, oxb, 0u, 0u, (pw + oxb - 1) / oxb, (ph + oyb - 1) / oyb, FREE_PLAIN_OXB_LOG2};
        front = (size_t)oyb * oxb;
    }
    *patch_off = (unsigned)((front + 15) / 16 * 16);
    *lds = *patch_off + free_patch_bytes(tl->oyb, tl->oxb);
    return *lds <= RESIZE_LDS_LIMIT;
}

}  // namespace ssw
