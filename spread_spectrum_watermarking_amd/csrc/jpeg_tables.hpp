// The integer pieces of ssw_jpeg_rgb8 that the host computes or that can be proven on the host (jpeg.hip includes this file;
// tests/cpp/jpeg_tables_test.cpp checks it without a GPU): the quantisation tables of a quality, and the quantiser's division
// as a multiplication with a reciprocal.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SSW_JPEG_HD __host__ __device__
#else
#define SSW_JPEG_HD
#endif

namespace ssw {

// ITU-T T.81 Annex K.1 / K.2 in natural (row-major) order: what libjpeg's jpeg_set_quality scales
constexpr uint8_t JPEG_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                   14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t JPEG_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// jpeg_quality_scaling + jpeg_add_quant_table with force_baseline: quality 1 .. 100 -> entries 1 .. 255
inline void jpeg_qtable(const uint8_t (&base)[64], uint32_t quality, uint8_t (&out)[64]) {
    const uint32_t scale = quality < 50 ? 5000u / quality : 200u - 2u * quality;
    for (int i = 0; i < 64; ++i) {
        const uint32_t v = (base[i] * scale + 50u) / 100u;
        out[i] = (uint8_t)(v < 1u ? 1u : v > 255u ? 255u : v);
    }
}

// n / d = the high half of n * jpeg_reciprocal(d): exact while n * d < 2^32 -- the quantiser's d = 8 q <= 2040 and
// n = |coefficient| + 4 q <= 2^17 + 1020 are far inside; the test goes through every pair.  A power of two gets 2^32 / d itself.
SSW_JPEG_HD inline uint32_t jpeg_reciprocal(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }
SSW_JPEG_HD inline uint32_t jpeg_divide(uint32_t n, uint32_t reciprocal) { return (uint32_t)(((uint64_t)n * reciprocal) >> 32); }

}  // namespace ssw
