// The three constants of a Gaussian blur as Pillow makes them (ImageFilter.GaussianBlur: three box passes per axis, after
// Gwosdek et al.), shared by filter.hip's host code and tests/cpp/filter_tables_test.cpp.  Host only: `float` arithmetic in the
// order of Pillow's C, every operation rounded on its own (the library is built with -ffp-contract=off), the square root and the
// floor in double as there.  include/ssw.h states the rule; tests/test_filter_cpu.py restates it in numpy.
#pragma once

#include <cmath>
#include <cstdint>

namespace ssw {

constexpr float FILTER_RADIUS_MAX = 8.0f;        // keeps r <= 7: a pass reaches 8 samples, three passes 24
constexpr uint32_t FILTER_R_MAX = 7;

// a box pass: out = (ww * (sum of the 2 r + 1 samples around x) + fw * (the two samples r + 1 away) + 2^23) >> 24
struct BlurConstants { uint32_t r, ww, fw; };

inline BlurConstants blur_constants(float radius) {
    const float sigma2 = radius * radius / 3;
    const float L = (float)std::sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)std::floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float rho = l + a;
    BlurConstants c;
    c.r = (uint32_t)(int)rho;
    c.ww = (uint32_t)((float)(1u << 24) / (rho * 2 + 1));
    c.fw = ((1u << 24) - (2 * c.r + 1) * c.ww) / 2;
    return c;
}

}  // namespace ssw
