// turned_stub.cpp -- the contract stand-in of the C functions include/ssw_turned.hpp names, beside ssw_stub.cpp (which states
// every entry point of ssw.hpp and owns the "device" blocks: heap blocks of exactly the bytes asked for, so a read or a write
// past one is an AddressSanitizer report).  Both READ every byte their contract says they read and WRITE every byte they say
// they write, with a pattern that encodes the position:
//   host_found[i] = {n = first byte of suspect i - 128, x = 10 i, y = 10 i + 1, tw = 8 (sw / 8), th = 8 (sh / 8), n_rungs, sad = 1000 i + last byte of suspect i}
//   host_rungs[(i * n_rungs + r) * 4 + k] = 100 i + 4 r + k (k = 0 .. 2), first byte of the original + r (k = 3)
//   dev_out[i] = the original, its first byte replaced by the first byte of suspect i and its last by (uint8) (angle + cx + cy)
// turned_stub_last(k): the scalar arguments of the last call (n, w, h, amin, amax, host_rungs given); turned_stub_fail(status):
// the next call answers `status` with no effect.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ssw.h"

namespace {
std::vector<double> g_last;
int g_fail = SSW_OK;
uint64_t g_sum = 0;

int check_shapes(const void* const* sus, const ssw_turned_shape* shapes, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!sus[i] || (shapes[i].channels != 3 && shapes[i].channels != 4)) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (shapes[i].w == 0 || shapes[i].h == 0 || shapes[i].w > 65535 || shapes[i].h > 65535) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n; ++i)
        if (shapes[i].channels == 4) return SSW_ERR_UNSUPPORTED;
    return SSW_OK;
}
}  // namespace

extern "C" {
double turned_stub_last(size_t k) { return k < g_last.size() ? g_last[k] : -1.0; }
void turned_stub_fail(int status) { g_fail = status; }
uint64_t turned_stub_checksum(void) { return g_sum; }

int ssw_locate_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, const ssw_turned_shape* shapes,
                           size_t n, double amin, double amax, ssw_turned_found* host_found, uint64_t* host_rungs) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_suspects || !shapes || !host_found) return SSW_ERR_BAD_ARG;
    if (!std::isfinite(amin) || !std::isfinite(amax) || amin > amax || amin < -45.0 || amax > 45.0) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    if (const int s = check_shapes(dev_suspects, shapes, n)) return s;
    for (size_t i = 0; i < n; ++i)
        if (shapes[i].w < 40 || shapes[i].h < 40 || w < 32 || h < 32) return SSW_ERR_BAD_DIMS;          // (every rung dropped)
    g_last = {(double)n, (double)w, (double)h, amin, amax, host_rungs ? 1.0 : 0.0};
    for (size_t i = 0; i < w * h * 3; ++i) g_sum = g_sum * 31 + dev_base[i];
    const int j0 = (int)std::floor(4.0 * amin), j1 = (int)std::ceil(4.0 * amax);
    const uint32_t n_rungs = (uint32_t)(j1 - j0 + 1);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* s = static_cast<const uint8_t*>(dev_suspects[i]);
        const size_t sb = (size_t)shapes[i].w * shapes[i].h * 3;
        for (size_t b = 0; b < sb; ++b) g_sum = g_sum * 31 + s[b];
        host_found[i] = ssw_turned_found{(int32_t)s[0] - 128, (uint32_t)(10 * i), (uint32_t)(10 * i + 1), shapes[i].w / 8 * 8, shapes[i].h / 8 * 8, n_rungs,
                                         1000 * i + s[sb - 1]};
        for (uint32_t r = 0; host_rungs && r < n_rungs; ++r) {
            for (uint32_t k = 0; k < 3; ++k) host_rungs[(i * n_rungs + r) * 4 + k] = 100 * i + 4 * r + k;
            host_rungs[(i * n_rungs + r) * 4 + 3] = (uint64_t)dev_base[0] + r;
        }
    }
    return SSW_OK;
}

int ssw_restore_turned_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t w, size_t h, const void* const* dev_suspects, const ssw_turned_shape* shapes,
                            const ssw_turned_job* jobs, size_t n, uint8_t* dev_out) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_suspects || !shapes || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(jobs[i].angle) || !std::isfinite(jobs[i].cx) || !std::isfinite(jobs[i].cy)) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > 65535 || h > 65535) return SSW_ERR_BAD_DIMS;
    if (const int s = check_shapes(dev_suspects, shapes, n)) return s;
    g_last = {(double)n, (double)w, (double)h, jobs[0].angle, jobs[n - 1].cy, 0.0};
    const size_t fb = w * h * 3;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* s = static_cast<const uint8_t*>(dev_suspects[i]);
        const size_t sb = (size_t)shapes[i].w * shapes[i].h * 3;
        for (size_t b = 0; b < sb; ++b) g_sum = g_sum * 31 + s[b];
        std::memcpy(dev_out + i * fb, dev_base, fb);
        dev_out[i * fb] = s[0];
        dev_out[(i + 1) * fb - 1] = (uint8_t)(int)(jobs[i].angle + jobs[i].cx + jobs[i].cy);
    }
    return SSW_OK;
}
}
