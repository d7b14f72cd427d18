// The tap tables of one axis of a Pillow resample (Image.resize on 8-bit frames: BOX, BILINEAR, BICUBIC, LANCZOS), shared by
// resample.hip's host code and tests/cpp/resample_tables_test.cpp.  Host only: `double` arithmetic in the order of Pillow's C
// (Resample.c: precompute_coeffs, normalize_coeffs_8bpc), every operation rounded on its own -- the pragma below keeps any
// compiler flag from fusing a multiply-add into it -- and libm's sin.  include/ssw.h states the rule; tests/test_resample_cpu.py
// restates it in numpy.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

namespace ssw {

constexpr int RESAMPLE_BOX = 0, RESAMPLE_BILINEAR = 1, RESAMPLE_BICUBIC = 2, RESAMPLE_LANCZOS = 3;   // = ssw_resample_filter
constexpr int RESAMPLE_FILTERS = 4;
constexpr int RESAMPLE_BITS = 22;                 // taps are fixed point with 22 fractional bits

inline double resample_support(int filter) {
    switch (filter) {
        case RESAMPLE_BOX: return 0.5;
        case RESAMPLE_BILINEAR: return 1.0;
        case RESAMPLE_BICUBIC: return 2.0;
        default: return 3.0;
    }
}

inline double resample_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return std::sin(x) / x;
}

inline double resample_filter(int filter, double x) {
    switch (filter) {
        case RESAMPLE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
        case RESAMPLE_BILINEAR:
            if (x < 0.0) x = -x;
            return x < 1.0 ? 1.0 - x : 0.0;
        case RESAMPLE_BICUBIC: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        default:
            if (-3.0 <= x && x < 3.0) return resample_sinc(x) * resample_sinc(x / 3);
            return 0.0;
    }
}

// output xx of the axis reads samples left[xx] .. left[xx] + count[xx] - 1 with the integer taps taps[xx * kmax ..]; the taps
// beyond count[xx] are 0.  kmax: the largest count (at least 1)
struct ResampleTable {
    std::vector<uint32_t> left, count;
    std::vector<int32_t> taps;
    uint32_t kmax = 1;
};

inline void build_resample_table(size_t in_len, size_t out_len, int filter, ResampleTable& t) {
    const double scale = (double)in_len / (double)out_len;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = resample_support(filter) * fs;
    const double ss = 1.0 / fs;
    t.left.assign(out_len, 0);
    t.count.assign(out_len, 0);
    std::vector<std::vector<double>> k(out_len);
    t.kmax = 1;
    for (size_t xx = 0; xx < out_len; ++xx) {
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > (int)in_len) xmax = (int)in_len;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        double ww = 0.0;
        k[xx].resize((size_t)xmax);
        for (int x = 0; x < xmax; ++x) {
            const double w = resample_filter(filter, ((double)(x + xmin) - center + 0.5) * ss);
            k[xx][(size_t)x] = w;
            ww += w;
        }
        if (ww != 0.0)
            for (int x = 0; x < xmax; ++x) k[xx][(size_t)x] /= ww;
        t.left[xx] = (uint32_t)xmin;
        t.count[xx] = (uint32_t)xmax;
        t.kmax = std::max(t.kmax, (uint32_t)xmax);
    }
    t.taps.assign(out_len * t.kmax, 0);
    for (size_t xx = 0; xx < out_len; ++xx)
        for (size_t x = 0; x < k[xx].size(); ++x) {
            const double v = k[xx][x];
            t.taps[xx * t.kmax + x] = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << RESAMPLE_BITS)) : (int32_t)(0.5 + v * (double)(1 << RESAMPLE_BITS));
        }
}

}  // namespace ssw
