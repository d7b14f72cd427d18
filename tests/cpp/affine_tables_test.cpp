// Host-only check of csrc/affine_tables.hpp (tests/test_rotate_cpu.py builds and runs it).  Two forms:
//   affine_tables_test matrix <w> <h> <angle> ...
//       one line per angle, the six entries of PIL.Image.rotate's matrix for a w x h frame as hexadecimal floats ("%a": every
//       bit), for the Python test to compare with the numbers Python makes
//   affine_tables_test plan <w> <h> <ow> <oh> <m0> ... <m5>
//       "<lds> <box_w> <box_h> <pitch> <lds_bytes>", then one line per tile of the output "<X0> <Y0> <x0> <y0> <bw> <bh>": the plan
//       of that transform and the box of source pixels each tile stages, for the Python test to hold every tap of its
//       restatement against
// Numbers are read with strtod, so the test passes them as repr() or float.hex() text.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "affine_tables.hpp"

int main(int argc, char** argv) {
    if (argc >= 5 && std::strcmp(argv[1], "matrix") == 0) {
        const size_t w = std::strtoul(argv[2], nullptr, 10), h = std::strtoul(argv[3], nullptr, 10);
        for (int i = 4; i < argc; ++i) {
            double m[6];
            ssw::rotation_matrix(std::strtod(argv[i], nullptr), w, h, m);
            std::printf("%a %a %a %a %a %a\n", m[0], m[1], m[2], m[3], m[4], m[5]);
        }
        return 0;
    }
    if (argc == 12 && std::strcmp(argv[1], "plan") == 0) {
        const uint32_t w = (uint32_t)std::strtoul(argv[2], nullptr, 10), h = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        const uint32_t ow = (uint32_t)std::strtoul(argv[4], nullptr, 10), oh = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        double m[6];
        for (int i = 0; i < 6; ++i) m[i] = std::strtod(argv[6 + i], nullptr);
        const ssw::AffinePlan p = ssw::affine_plan(m, w, h);
        std::printf("%d %u %u %u %zu\n", p.lds ? 1 : 0, p.box_w, p.box_h, p.pitch, p.lds_bytes);
        for (uint32_t Y0 = 0; Y0 < oh; Y0 += ssw::AFFINE_TILE_H)
            for (uint32_t X0 = 0; X0 < ow; X0 += ssw::AFFINE_TILE_W) {
                const ssw::AffineBox b = ssw::affine_tile_box(m, X0, Y0, std::min(X0 + ssw::AFFINE_TILE_W, ow) - 1,
                                                              std::min(Y0 + ssw::AFFINE_TILE_H, oh) - 1, w, h);
                std::printf("%u %u %d %d %d %d\n", X0, Y0, b.x0, b.y0, b.bw, b.bh);
            }
        return 0;
    }
    std::fprintf(stderr, "usage: affine_tables_test matrix W H ANGLE... | plan W H OW OH M0 .. M5\n");
    return 2;
}
