// Host-only check of csrc/resample_tables.hpp (tests/test_resample_cpu.py builds and runs it): prints the tables the library
// makes for one axis of a Pillow resample, one line per (in, out, filter):
//   "<in> <out> <filter> <kmax> | left count tap tap ... | left count tap ..."     (count taps per output, nothing padded)
// for every in, out in 1 .. 48, the 4K pairs 3840 -> 1920, 1280, 960, 480, 7 and 2160 -> 1080, 720, 270, 1, and 640 -> 1280,
// each with the four filters, for the Python test to compare number for number with its own restatement of Pillow's rule.
#include <cstdint>
#include <cstdio>

#include "resample_tables.hpp"

static void line(size_t in, size_t out, int filter) {
    ssw::ResampleTable t;
    ssw::build_resample_table(in, out, filter, t);
    std::printf("%zu %zu %d %u", in, out, filter, t.kmax);
    for (size_t xx = 0; xx < out; ++xx) {
        std::printf(" | %u %u", t.left[xx], t.count[xx]);
        for (uint32_t x = 0; x < t.count[xx]; ++x) std::printf(" %d", t.taps[xx * t.kmax + x]);
    }
    std::printf("\n");
}

int main() {
    static const size_t big[][2] = {{3840, 1920}, {3840, 1280}, {3840, 960}, {3840, 480}, {3840, 7},
                                    {2160, 1080}, {2160, 720},  {2160, 270}, {2160, 1},   {640, 1280}};
    for (int f = 0; f < ssw::RESAMPLE_FILTERS; ++f) {
        for (size_t in = 1; in <= 48; ++in)
            for (size_t out = 1; out <= 48; ++out) line(in, out, f);
        for (const auto& p : big) line(p[0], p[1], f);
    }
    return 0;
}
