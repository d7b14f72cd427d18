// The host side of the search for cut-outs of a turned copy (ssw_locate_turned_rgb8), shared by locate_turned.hip and
// tests/cpp/turned_tables_test.cpp; it compiles without HIP.  include/ssw.h states the definition: the template of an angle is
// the suspect's luma turned back about its own centre, as large as its four corner pixels stay valid; the restoring matrix lays
// a suspect whose centre and angle are known back into the original's frame.  tests/test_locate_turned_cpu.py restates both.
#pragma once

#include <algorithm>
#include <cstdint>

#include "angle_tables.hpp"

namespace ssw {

constexpr uint32_t TURNED_SIDE_MIN = 32;     // a template's smaller side
constexpr int TURNED_NEAR_XY = 8;            // the refinement's window: +-8 positions around the rung's entry
constexpr uint32_t TURNED_STRIDE = 4;        // the ladder's candidate positions
constexpr uint32_t TURNED_BOX = 8;

// the sample point of template pixel (X, Y) of the angle (C, S) at size tw x th, in 1 / 131072 of a suspect pixel
inline void turned_point(int64_t sw, int64_t sh, int32_t C, int32_t S, int64_t tw, int64_t th, int64_t X, int64_t Y, int64_t* Rx, int64_t* Ry) {
    const int64_t p = 2 * X + 1 - tw, q = 2 * Y + 1 - th;
    *Rx = (sw - 1) * 65536 + C * p - S * q;
    *Ry = (sh - 1) * 65536 + S * p + C * q;
}

// tw x th of angle n for a suspect sw x sh (sides 1 .. 65535): the largest i in 1 .. sw / 8 whose four corner pixels are valid;
// false: there is none
inline bool turned_template_size(uint32_t sw, uint32_t sh, int32_t n, uint32_t* tw, uint32_t* th) {
    int32_t C = 0, S = 0;
    angle_table(n, &C, &S);
    for (uint64_t i = sw / 8; i >= 1; --i) {
        const int64_t w = 8 * (int64_t)i, h = 8 * (int64_t)std::max<uint64_t>(1, (2 * i * sh + sw) / (2 * (uint64_t)sw));
        bool ok = true;
        for (int k = 0; k < 4 && ok; ++k) {
            int64_t Rx = 0, Ry = 0;
            turned_point(sw, sh, C, S, w, h, (k & 1) ? w - 1 : 0, (k & 2) ? h - 1 : 0, &Rx, &Ry);
            const int64_t X0 = Rx >> 17, Y0 = Ry >> 17;
            ok = X0 >= 0 && X0 <= (int64_t)sw - 2 && Y0 >= 0 && Y0 <= (int64_t)sh - 2;
        }
        if (ok) { *tw = (uint32_t)w; *th = (uint32_t)h; return true; }
    }
    return false;
}

// ... and whether the search uses the angle at all in a W x H frame
inline bool turned_usable_size(size_t W, size_t H, uint32_t sw, uint32_t sh, int32_t n, uint32_t* tw, uint32_t* th) {
    return turned_template_size(sw, sh, n, tw, th) && std::min(*tw, *th) >= TURNED_SIDE_MIN && *tw <= W && *th <= H;
}

// the matrix that lays a suspect sw x sh, turned by `angle` degrees and centred at (cx, cy) pixels of the original, back into the
// original's frame: every operation rounded on its own
inline void turned_restore_matrix(double angle, double cx, double cy, uint32_t sw, uint32_t sh, double m[6]) {
    double b[6];
    rotation_matrix(-angle, 0, 0, b);
    m[0] = b[0]; m[1] = b[1]; m[3] = b[3]; m[4] = b[4];
    m[2] = (b[0] * -cx + b[1] * -cy + 0.0) + (double)sw / 2.0;
    m[5] = (b[3] * -cx + b[4] * -cy + 0.0) + (double)sh / 2.0;
}

}  // namespace ssw
