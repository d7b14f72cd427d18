// angle_stub.cpp -- the contract stand-in of the two C functions include/ssw_angle.hpp names, beside ssw_stub.cpp (which states
// every entry point of ssw.hpp and owns the "device" blocks: heap blocks of exactly the bytes asked for, so a read or a write
// past one is an AddressSanitizer report).  ssw_find_angle_rgb8 READS every byte its contract says it reads and WRITES every
// byte it says it writes, with a pattern that encodes the position:
//   host_found[i] = {n = first byte of suspect i - 128, n_rungs = j1 - j0 + 1, sad = 1000 i + last byte of suspect i, count = w h}
//   host_rungs[(i * n_rungs + r) * 2] = 100 i + r, [.. + 1] = first byte of the original + r
// angle_stub_last(k): the scalar arguments of the last call (n, w, h, amin, amax, host_rungs given); angle_stub_fail(status): the
// next call answers `status` with no effect.
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
double angle_stub_last(size_t k) { return k < g_last.size() ? g_last[k] : -1.0; }
void angle_stub_fail(int status) { g_fail = status; }
uint64_t angle_stub_checksum(void) { return g_sum; }

int ssw_angle_table(int32_t n, int32_t* c, int32_t* s) {
    if (!c || !s) return SSW_ERR_BAD_ARG;
    *c = 65536 - (n < 0 ? -n : n);
    *s = -n;
    return SSW_OK;
}

int ssw_find_angle_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, const uint8_t* dev_suspects, size_t n, size_t w, size_t h, double amin, double amax,
                        ssw_angle_found* host_found, uint64_t* host_rungs) {
    if (g_fail != SSW_OK) { const int s = g_fail; g_fail = SSW_OK; return s; }
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_suspects || !host_found) return SSW_ERR_BAD_ARG;
    if (!std::isfinite(amin) || !std::isfinite(amax) || amin > amax || amin < -45.0 || amax > 45.0) return SSW_ERR_BAD_ARG;
    if (w < 32 || h < 32) return SSW_ERR_BAD_DIMS;
    if (w * h > ((size_t)1 << 27)) return SSW_ERR_UNSUPPORTED;
    g_last = {(double)n, (double)w, (double)h, amin, amax, host_rungs ? 1.0 : 0.0};
    const size_t fb = w * h * 3;
    for (size_t i = 0; i < fb; ++i) g_sum = g_sum * 31 + dev_base[i];
    for (size_t i = 0; i < n * fb; ++i) g_sum = g_sum * 31 + dev_suspects[i];
    const int j0 = (int)std::floor(4.0 * amin), j1 = (int)std::ceil(4.0 * amax);
    const uint32_t n_rungs = (uint32_t)(j1 - j0 + 1);
    for (size_t i = 0; i < n; ++i) {
        host_found[i] = ssw_angle_found{(int32_t)dev_suspects[i * fb] - 128, n_rungs, 1000 * i + dev_suspects[(i + 1) * fb - 1], (uint64_t)(w * h)};
        for (uint32_t r = 0; host_rungs && r < n_rungs; ++r) {
            host_rungs[(i * n_rungs + r) * 2] = 100 * i + r;
            host_rungs[(i * n_rungs + r) * 2 + 1] = (uint64_t)dev_base[0] + r;
        }
    }
    return SSW_OK;
}
}
