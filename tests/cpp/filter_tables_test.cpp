// Host-only check of csrc/filter_tables.hpp (tests/test_filter_cpu.py builds and runs it): prints the three constants the
// library makes for a Gaussian blur of every radius 0.1, 0.2 .. 8.0 and then of 2.4, 2.5 (either side of the step from r = 1 to
// r = 2) and 8.0 (the largest accepted), one line each ("radius <radius> <r> <ww> <fw>"), for the Python test to compare with its
// own restatement of Pillow's rule.
#include <cstdint>
#include <cstdio>

#include "filter_tables.hpp"

static void line(float radius) {
    const ssw::BlurConstants c = ssw::blur_constants(radius);
    std::printf("radius %.9g %u %u %u\n", (double)radius, c.r, c.ww, c.fw);
}

int main() {
    for (int i = 1; i <= 80; ++i) line((float)(i / 10.0));
    line(2.4f);
    line(2.5f);
    line(8.0f);
    return 0;
}
