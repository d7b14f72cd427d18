// The host arithmetic of the search for turned cut-outs (csrc/turned_tables.hpp) as a stand-alone program;
// tests/test_locate_turned_cpu.py compares its output with Python's.
//   "size sw sh n tw th"    the template size of every angle n / 32 degrees, n = -1440 .. 1440, on a few suspect shapes (0 0: none)
//   "matrix m0 .. m5"       a few restoring matrices, as hexadecimal doubles
#include <cstdio>

#include "turned_tables.hpp"

int main() {
    const uint32_t shapes[][2] = {{64, 64}, {70, 66}, {1000, 64}, {640, 444}, {67, 65}, {33, 200}};
    for (const auto& s : shapes)
        for (int32_t n = -1440; n <= 1440; ++n) {
            uint32_t tw = 0, th = 0;
            if (!ssw::turned_template_size(s[0], s[1], n, &tw, &th)) tw = th = 0;
            std::printf("size %u %u %d %u %u\n", s[0], s[1], (int)n, tw, th);
        }
    const struct { double angle, cx, cy; uint32_t sw, sh; } jobs[] = {{3.3125, 319.0, 240.0, 400, 300}, {-8.03125, 360.5, 222.25, 320, 256},
                                                                      {0.0, 10.0, 7.5, 5, 4}, {45.0, -3.0, 900.5, 64, 64},
                                                                      {-0.03125, 32768.0, 1.0, 65535, 1}};
    for (const auto& j : jobs) {
        double m[6];
        ssw::turned_restore_matrix(j.angle, j.cx, j.cy, j.sw, j.sh, m);
        std::printf("matrix %a %a %a %a %a %a\n", m[0], m[1], m[2], m[3], m[4], m[5]);
    }
    return 0;
}
