// rotate_search_stub.cpp -- the contract stand-in of ssw_rotate_search_attack_rgb8, which include/ssw_rotate_search.hpp names,
// beside ssw_stub.cpp (every entry point of ssw.hpp; it owns the "device" blocks: heap blocks of exactly the bytes asked for, so a
// read or a write past one is an AddressSanitizer report) and angle_stub.cpp.  The call READS every byte its contract says it
// reads and WRITES every byte it says it writes, with a pattern that encodes the position; src = frame jobs[i].frame:
//   dev_out[i][b] = src[b] ^ 0x5A, dev_turned[i][b] = src[b] + 1 (when given)
//   host_found[i] = {n = first byte of src - 128, n_rungs = j1 - j0 + 1, sad = 1000 i + last byte of src, count = w h}
//   host_kept[i] = w h - i
//   host_rungs[(i * n_rungs + r) * 2] = 100 i + r, [.. + 1] = first byte of the original + r (when given)
// rotate_search_stub_last(k): the scalar arguments of the last call (n_frames, w, h, n_jobs, amin, amax, dev_turned given,
// host_rungs given, the last job's filter, its forward[0], its fill[1]); rotate_search_stub_fail(status): the next call answers
// `status` with no effect.
#include <cmath>
#include <cstdint>
#include <vector>

#include "ssw.h"

namespace {
std::vector<double> g_last;
int g_fail = SSW_OK;
uint64_t g_sum = 0;
}  // namespace

extern "C" {
double rotate_search_stub_last(size_t k) { return k < g_last.size() ? g_last[k] : -1.0; }
void rotate_search_stub_fail(int status) { g_fail = status; }
uint64_t rotate_search_stub_checksum(void) { return g_sum; }

int ssw_rotate_search_attack_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h,
                                  const ssw_rotate_job* jobs, size_t n_jobs, double amin, double amax, uint8_t* dev_out, uint8_t* dev_turned,
                                  ssw_angle_found* host_found, uint64_t* host_rungs, uint64_t* host_kept) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_base || !dev_frames || !jobs || !dev_out || !host_found || !host_kept) return SSW_ERR_BAD_ARG;
    if (!std::isfinite(amin) || !std::isfinite(amax) || amin > amax || amin < -45.0 || amax > 45.0) return SSW_ERR_BAD_ARG;
    if (w < 32 || h < 32 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    if (w * h > ((size_t)1 << 27)) return SSW_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n_jobs; ++i) {
        if (jobs[i].frame >= n_frames || jobs[i].filter > (uint32_t)SSW_AFFINE_BICUBIC) return SSW_ERR_BAD_ARG;
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(jobs[i].forward[k])) return SSW_ERR_BAD_ARG;
    }
    const ssw_rotate_job& last = jobs[n_jobs - 1];
    g_last = {(double)n_frames, (double)w, (double)h, (double)n_jobs, amin, amax, dev_turned ? 1.0 : 0.0, host_rungs ? 1.0 : 0.0,
              (double)last.filter, last.forward[0], (double)last.fill[1]};
    const size_t fb = w * h * 3;
    for (size_t i = 0; i < fb; ++i) g_sum = g_sum * 31 + dev_base[i];
    for (size_t i = 0; i < n_frames * fb; ++i) g_sum = g_sum * 31 + dev_frames[i];
    const int j0 = (int)std::floor(4.0 * amin), j1 = (int)std::ceil(4.0 * amax);
    const uint32_t n_rungs = (uint32_t)(j1 - j0 + 1);
    for (size_t i = 0; i < n_jobs; ++i) {
        const uint8_t* src = dev_frames + (size_t)jobs[i].frame * fb;
        for (size_t b = 0; b < fb; ++b) {
            dev_out[i * fb + b] = (uint8_t)(src[b] ^ 0x5A);
            if (dev_turned) dev_turned[i * fb + b] = (uint8_t)(src[b] + 1);
        }
        host_found[i] = ssw_angle_found{(int32_t)src[0] - 128, n_rungs, 1000 * i + src[fb - 1], (uint64_t)(w * h)};
        host_kept[i] = (uint64_t)(w * h) - i;
        for (uint32_t r = 0; host_rungs && r < n_rungs; ++r) {
            host_rungs[(i * n_rungs + r) * 2] = 100 * i + r;
            host_rungs[(i * n_rungs + r) * 2 + 1] = (uint64_t)dev_base[0] + r;
        }
    }
    return SSW_OK;
}
}
