// locate_free_stub.cpp -- the contract stand-in of ssw_locate_free_rgb8, which include/ssw_locate_free.hpp names, beside
// ssw_stub.cpp (every entry point of ssw.hpp; it owns the "device" blocks: heap blocks of exactly the bytes asked for, so a read
// past one is an AddressSanitizer report).  A call READS every byte its contract says it reads -- the original, every suspect
// at its w x h x channels, every range and slack -- and WRITES every output with a pattern that encodes the position:
//   placements[i].pw = wmax_i, .ph = wmin_i + slack_i, .x = i + 1, .y = 2 i + slack_i;  host_sad[i] = 1000 i + w_i
// locate_free_stub_last(k): the scalar arguments of the last call (n, w, h, the last suspect's w, h, channels, the last range's
// wmin, wmax, the last slack); locate_free_stub_fail(status): the next call answers `status` with no effect.
#include <cstdint>
#include <vector>

#include "ssw.h"

namespace {
std::vector<double> g_last;
int g_fail = SSW_OK;
uint64_t g_sum = 0;
}  // namespace

extern "C" {
double locate_free_stub_last(size_t k) { return k < g_last.size() ? g_last[k] : -1.0; }
void locate_free_stub_fail(int status) { g_fail = status; }
uint64_t locate_free_stub_checksum(void) { return g_sum; }

int ssw_locate_free_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* const* dev_suspects, ssw_placement* placements,
                         const ssw_scale_range* ranges, const uint32_t* slack, size_t n, uint64_t* host_sad) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base_rgb || !dev_suspects || !placements || !ranges || !slack || !host_sad || w == 0 || h == 0) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i) {
        const ssw_placement& p = placements[i];
        if (!dev_suspects[i] || (p.channels != 3 && p.channels != 4) || p.w == 0 || p.h == 0) return SSW_ERR_BAD_ARG;
        if (slack[i] < 1 || slack[i] > 4 || ranges[i].wmin > ranges[i].wmax || ranges[i].wmin < 32) return SSW_ERR_BAD_ARG;
    }
    const ssw_placement& last = placements[n - 1];
    g_last = {(double)n, (double)w, (double)h, (double)last.w, (double)last.h, (double)last.channels, (double)ranges[n - 1].wmin,
              (double)ranges[n - 1].wmax, (double)slack[n - 1]};
    for (size_t b = 0; b < w * h * 3; ++b) g_sum = g_sum * 31 + dev_base_rgb[b];
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* s = static_cast<const uint8_t*>(dev_suspects[i]);
        for (size_t b = 0; b < (size_t)placements[i].w * placements[i].h * placements[i].channels; ++b) g_sum = g_sum * 31 + s[b];
        placements[i].pw = ranges[i].wmax; placements[i].ph = ranges[i].wmin + slack[i];
        placements[i].x = (uint32_t)i + 1; placements[i].y = 2 * (uint32_t)i + slack[i];
        host_sad[i] = 1000 * i + placements[i].w;
    }
    return SSW_OK;
}

// the diagnostic beside it: the argument checks of include/ssw.h; reads the original, the suspect and the start; nothing is
// scored, so every slot holds all ones and the answer is the start with SAD 0
int ssw_locate_free_sums_rgb8(ssw_ctx* ctx, const uint8_t* dev_base_rgb, size_t w, size_t h, const void* dev_suspect, size_t sw, size_t sh,
                              size_t channels, const uint32_t start[4], uint32_t wmin, uint32_t wmax, uint32_t slack, uint64_t* host_sums,
                              ssw_placement* answer, uint64_t* host_sad) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx || !dev_base_rgb || !dev_suspect || !start || !host_sums || !answer || !host_sad || w == 0 || h == 0) return SSW_ERR_BAD_ARG;
    if ((channels != 3 && channels != 4) || sw == 0 || sh == 0 || slack < 1 || slack > 4 || wmin > wmax) return SSW_ERR_BAD_ARG;
    if (start[0] == 0 || start[1] == 0 || start[0] > w || start[1] > h || start[2] > w - start[0] || start[3] > h - start[1]) return SSW_ERR_BAD_ARG;
    for (size_t b = 0; b < w * h * 3; ++b) g_sum = g_sum * 31 + dev_base_rgb[b];
    for (size_t b = 0; b < sw * sh * channels; ++b) g_sum = g_sum * 31 + static_cast<const uint8_t*>(dev_suspect)[b];
    const size_t side = 2 * (size_t)slack + 1;
    for (size_t i = 0; i < side * side * 81; ++i) host_sums[i] = UINT64_MAX;
    *answer = ssw_placement{(uint32_t)sw, (uint32_t)sh, (uint32_t)channels, start[2], start[3], start[0], start[1]};
    *host_sad = 0;
    return SSW_OK;
}
}
