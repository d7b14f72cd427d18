// The host side of the affine transform (ssw_affine_rgb8, ssw_rotate_attack_rgb8, ssw_unrotate_rgb8), shared by affine.hip and
// tests/cpp/affine_tables_test.cpp; it compiles without HIP.  include/ssw.h states the definition: PIL.Image.rotate's matrix
// as Python makes it, the sample point of an output pixel, and the plan of a launch -- the box of source pixels a tile of
// output pixels can read, and whether that box is staged in LDS or the taps come from global memory.  `double` arithmetic, every
// operation rounded on its own: the pragma below keeps any compiler flag from fusing a multiply-add into it.
// tests/test_rotate_cpu.py restates all of it in numpy and compares number for number.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#if defined(__HIPCC__)
#define SSW_AFFINE_HD __host__ __device__
#else
#define SSW_AFFINE_HD
#endif

namespace ssw {

constexpr int AFFINE_BILINEAR = 0, AFFINE_BICUBIC = 1;      // = ssw_affine_filter
constexpr unsigned AFFINE_TILE_W = 32, AFFINE_TILE_H = 8;   // output pixels of a block: one a thread
constexpr size_t AFFINE_LDS_BYTES = 16 << 10;               // the largest staged box; a larger one: the global form

// Python's round(x, 15) for |x| <= 1: the correctly rounded decimal of 15 places, read back (ties to even on the exact binary
// value, as the C library prints it; -0.0 stays -0.0)
inline double affine_round15(double x) {
    char text[64];
    std::snprintf(text, sizeof text, "%.15f", x);
    return std::strtod(text, nullptr);
}

// Python's angle % 360.0: the remainder takes the divisor's sign
inline double affine_mod360(double angle) {
    double r = std::fmod(angle, 360.0);
    if (r != 0.0) {
        if (r < 0.0) r += 360.0;
    } else {
        r = 0.0;
    }
    return r;
}

// PIL.Image.rotate(angle) with expand=False and the default centre on a w x h frame: the matrix it hands to Image.transform
inline void rotation_matrix(double angle, size_t w, size_t h, double m[6]) {
    const double a = -(affine_mod360(angle) * (3.14159265358979323846 / 180.0));       // -math.radians(angle % 360.0)
    const double c = affine_round15(std::cos(a)), s = affine_round15(std::sin(a));
    m[0] = c; m[1] = s; m[2] = 0.0; m[3] = affine_round15(-std::sin(a)); m[4] = c; m[5] = 0.0;
    const double cx = (double)w / 2.0, cy = (double)h / 2.0;
    m[2] = (m[0] * -cx + m[1] * -cy + 0.0) + cx;
    m[5] = (m[3] * -cx + m[4] * -cy + 0.0) + cy;
}

inline bool affine_is_identity(const double m[6]) {
    return m[0] == 1.0 && m[1] == 0.0 && m[2] == 0.0 && m[3] == 0.0 && m[4] == 1.0 && m[5] == 0.0;
}

// the sample point of output pixel (X, Y): summed from the left
SSW_AFFINE_HD inline void affine_point(const double* m, uint32_t X, uint32_t Y, double& xin, double& yin) {
    const double px = (double)X + 0.5, py = (double)Y + 0.5;
    xin = m[0] * px + m[1] * py + m[2];
    yin = m[3] * px + m[4] * py + m[5];
}

// inside: what Pillow's `xin < 0 || xin >= w || yin < 0 || yin >= h` lets through, and not a NaN (an overflowing matrix; Pillow
// would convert it to an integer)
SSW_AFFINE_HD inline bool affine_inside(double xin, double yin, uint32_t w, uint32_t h) {
    return xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h;
}

// The box of source pixels that the output pixels X0 .. X1, Y0 .. Y1 (inclusive) can read: every term of the sum is monotone in
// X and in Y after rounding, so the four corners' sample points bound all others; a pixel that reads at all has its point
// inside the frame; BICUBIC reaches from floor(xin - 0.5) - 1 to floor(xin - 0.5) + 2, and taps are clamped to the frame.
struct AffineBox { int x0, y0, bw, bh; };
SSW_AFFINE_HD inline AffineBox affine_tile_box(const double* m, uint32_t X0, uint32_t Y0, uint32_t X1, uint32_t Y1, uint32_t w, uint32_t h) {
    double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
    for (int k = 0; k < 4; ++k) {
        double x, y;
        affine_point(m, (k & 1) ? X1 : X0, (k & 2) ? Y1 : Y0, x, y);
        if (k == 0 || !(x >= xlo)) xlo = x;
        if (k == 0 || !(x <= xhi)) xhi = x;
        if (k == 0 || !(y >= ylo)) ylo = y;
        if (k == 0 || !(y <= yhi)) yhi = y;
    }
    // into 0 .. w and 0 .. h, whatever they are (an infinity or a NaN of an overflowing matrix too): a tile that lies outside
    // altogether reads nothing, any box will do for it
    const auto into = [](double v, double hi) { return !(v >= 0.0) ? 0.0 : !(v <= hi) ? hi : v; };
    xlo = into(xlo, (double)w); xhi = into(xhi, (double)w);
    ylo = into(ylo, (double)h); yhi = into(yhi, (double)h);
    const int W = (int)w, H = (int)h;
    const int x0 = (int)floor(xlo - 0.5) - 1, x1 = (int)floor(xhi - 0.5) + 2;
    const int y0 = (int)floor(ylo - 0.5) - 1, y1 = (int)floor(yhi - 0.5) + 2;
    AffineBox b;
    b.x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
    b.y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    b.bw = (x1 > W - 1 ? W - 1 : (x1 < b.x0 ? b.x0 : x1)) - b.x0 + 1;
    b.bh = (y1 > H - 1 ? H - 1 : (y1 < b.y0 ? b.y0 : y1)) - b.y0 + 1;
    return b;
}

// The plan of a launch: no tile's box is wider than box_w or taller than box_h -- |m0| (TILE_W - 1) + |m1| (TILE_H - 1) bounds
// the spread of the sample points of a tile, its floor adds one column, the BICUBIC reach three, and one is spare for the
// rounding of the sums.  lds: the box (rows of `pitch` bytes, a multiple of 4) fits AFFINE_LDS_BYTES.
struct AffinePlan { bool lds; uint32_t box_w, box_h, pitch; size_t lds_bytes; };
inline AffinePlan affine_plan(const double m[6], size_t w, size_t h) {
    const double sx = std::fabs(m[0]) * (AFFINE_TILE_W - 1) + std::fabs(m[1]) * (AFFINE_TILE_H - 1);
    const double sy = std::fabs(m[3]) * (AFFINE_TILE_W - 1) + std::fabs(m[4]) * (AFFINE_TILE_H - 1);
    AffinePlan p{false, 0, 0, 0, 0};
    if (!(sx < 65536.0) || !(sy < 65536.0)) return p;
    p.box_w = (uint32_t)std::min<size_t>(w, (size_t)std::ceil(sx) + 6);
    p.box_h = (uint32_t)std::min<size_t>(h, (size_t)std::ceil(sy) + 6);
    p.pitch = (p.box_w * 3 + 3) & ~3u;
    p.lds_bytes = (size_t)p.pitch * p.box_h;
    p.lds = p.lds_bytes <= AFFINE_LDS_BYTES;
    return p;
}

}  // namespace ssw
