// crop_stub.cpp -- the contract stand-ins of ssw_crop_attack_rgb8 and ssw_crop_search_attack_rgb8, which include/ssw_crop.hpp
// names, beside ssw_stub.cpp (every entry point of ssw.hpp; it owns the "device" blocks: heap blocks of exactly the bytes asked
// for, so a read or a write past one is an AddressSanitizer report).  A call READS every byte its contract says it reads and
// WRITES every byte it says it writes, with a pattern that encodes the position; src = frame jobs[i].frame, T = tw x th or cw x ch:
//   dev_out[i][b] = src[b] ^ 0x3C
//   dev_thumbs, T_i [b] = (first byte of the rectangle in src) + b + i (when given), packed in job order
//   host_found[i] = {T's w, T's h, 3, x + 1, y + 2, wmax or T's w, wmin or T's h};  host_sad[i] = 1000 i + cw
// crop_stub_last(k): the scalar arguments of the last call (n_frames, w, h, n_jobs, dev_thumbs given, searched, the last job's
// x, y, cw, ch, tw, th, filter, the last search's wmin, wmax); crop_stub_fail(status): the next call answers `status` with no effect.
#include <cstdint>
#include <vector>

#include "ssw.h"

namespace {
std::vector<double> g_last;
int g_fail = SSW_OK;
uint64_t g_sum = 0;

int run(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_crop_job* jobs,
        const ssw_crop_search* searches, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs, ssw_placement* host_found, uint64_t* host_sad) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_base || !dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n_jobs; ++i) {
        const ssw_crop_job& j = jobs[i];
        if (j.frame >= n_frames || j.cw == 0 || j.ch == 0 || (j.tw == 0) != (j.th == 0)) return SSW_ERR_BAD_ARG;
        if ((uint64_t)j.x + j.cw > w || (uint64_t)j.y + j.ch > h) return SSW_ERR_BAD_ARG;
        if (j.tw && j.filter > (uint32_t)SSW_RESAMPLE_LANCZOS) return SSW_ERR_BAD_ARG;
        if (j.tw > 65535 || j.th > 65535) return SSW_ERR_BAD_DIMS;
    }
    const ssw_crop_job& last = jobs[n_jobs - 1];
    g_last = {(double)n_frames, (double)w, (double)h, (double)n_jobs, dev_thumbs ? 1.0 : 0.0, searches ? 1.0 : 0.0, (double)last.x, (double)last.y,
              (double)last.cw, (double)last.ch, (double)last.tw, (double)last.th, (double)last.filter,
              searches ? (double)searches[n_jobs - 1].wmin : -1.0, searches ? (double)searches[n_jobs - 1].wmax : -1.0};
    const size_t fb = w * h * 3;
    for (size_t i = 0; i < fb; ++i) g_sum = g_sum * 31 + dev_base[i];
    for (size_t i = 0; i < n_frames * fb; ++i) g_sum = g_sum * 31 + dev_frames[i];
    size_t at = 0;
    for (size_t i = 0; i < n_jobs; ++i) {
        const ssw_crop_job& j = jobs[i];
        const uint8_t* src = dev_frames + (size_t)j.frame * fb;
        for (size_t b = 0; b < fb; ++b) dev_out[i * fb + b] = (uint8_t)(src[b] ^ 0x3C);
        const uint32_t tw = j.tw ? j.tw : j.cw, th = j.tw ? j.th : j.ch;
        const size_t tb = (size_t)tw * th * 3;
        const uint8_t first = src[((size_t)j.y * w + j.x) * 3];
        for (size_t b = 0; dev_thumbs && b < tb; ++b) dev_thumbs[at + b] = (uint8_t)(first + b + i);
        at += tb;
        if (searches) {
            host_found[i] = ssw_placement{tw, th, 3, j.x + 1, j.y + 2, searches[i].wmax ? searches[i].wmax : tw, searches[i].wmin ? searches[i].wmin : th};
            host_sad[i] = 1000 * i + j.cw;
        }
    }
    return SSW_OK;
}
}  // namespace

extern "C" {
double crop_stub_last(size_t k) { return k < g_last.size() ? g_last[k] : -1.0; }
void crop_stub_fail(int status) { g_fail = status; }
uint64_t crop_stub_checksum(void) { return g_sum; }

int ssw_crop_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                         const ssw_crop_job* jobs, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs) {
    return run(ctx, dev_base, dev_frames, n_frames, w, h, jobs, nullptr, n_jobs, dev_out, dev_thumbs, nullptr, nullptr);
}

int ssw_crop_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                const ssw_crop_job* jobs, const ssw_crop_search* searches, size_t n_jobs, uint8_t* dev_out, uint8_t* dev_thumbs,
                                ssw_placement* host_found, uint64_t* host_sad) {
    if (n_jobs && g_fail == SSW_OK && ctx && (!searches || !host_found || !host_sad)) return SSW_ERR_BAD_ARG;
    return run(ctx, dev_base, dev_frames, n_frames, w, h, jobs, searches, n_jobs, dev_out, dev_thumbs, host_found, host_sad);
}
}
