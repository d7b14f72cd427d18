// The host side of the angle search (ssw_find_angle_rgb8), shared by angle.hip and tests/cpp/angle_tables_test.cpp; it compiles
// without HIP.  include/ssw.h states the definition: an angle is a / 32 degrees, and all the search uses of its matrix are two
// integers, C(a) and S(a); the ladder of a range is the rungs j0 .. j1.  tests/test_angle_cpu.py restates both in Python.
#pragma once

#include <cmath>
#include <cstdint>

#include "affine_tables.hpp"

namespace ssw {

constexpr int ANGLE_PER_DEGREE = 32;        // the answer's resolution: angles are a / 32 degrees
constexpr int ANGLE_RUNG_STEP = 8;          // a rung every 8 / 32 = 0.25 degrees
constexpr int ANGLE_RUNG_MAX = 180;         // |j| of a rung: +-45 degrees
constexpr unsigned ANGLE_KEEP = 4;          // rungs that are refined
constexpr int ANGLE_NEAR = 7;               // ... by every a within 7 of them
constexpr unsigned ANGLE_SLOTS = ANGLE_KEEP * (2 * ANGLE_NEAR + 1);      // candidates of the refinement, duplicates included
constexpr size_t ANGLE_SIDE_MIN = 32;
constexpr size_t ANGLE_PIXELS_MAX = (size_t)1 << 27;

// C(a), S(a): the first two entries of PIL.Image.rotate(a / 32)'s matrix in 16.16 fixed point, rounded half up in doubles
inline void angle_table(int32_t a, int32_t* c, int32_t* s) {
    double m[6];
    rotation_matrix((double)a / (double)ANGLE_PER_DEGREE, 0, 0, m);
    *c = (int32_t)std::floor(m[0] * 65536.0 + 0.5);
    *s = (int32_t)std::floor(m[1] * 65536.0 + 0.5);
}

// the rungs of a range: rounded outwards, clipped to +-45 degrees; false: not finite, reversed or beyond +-45
inline bool angle_rungs(double amin, double amax, int* j0, int* j1) {
    if (!std::isfinite(amin) || !std::isfinite(amax) || amin > amax || amin < -45.0 || amax > 45.0) return false;
    const int lo = (int)std::floor(4.0 * amin), hi = (int)std::ceil(4.0 * amax);
    *j0 = lo < -ANGLE_RUNG_MAX ? -ANGLE_RUNG_MAX : lo;
    *j1 = hi > ANGLE_RUNG_MAX ? ANGLE_RUNG_MAX : hi;
    return true;
}

}  // namespace ssw
