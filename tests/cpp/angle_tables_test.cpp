// The host arithmetic of the angle search (csrc/angle_tables.hpp) as a stand-alone program; tests/test_angle_cpu.py compares its
// output with Python's.
//   angle_tables_test table              "n C S" of every angle n / 32 degrees, n = -1440 .. 1440
//   angle_tables_test rungs LO HI ...    per pair of hexadecimal doubles "ok j0 j1" of the ladder of that range (ok 0: refused)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "angle_tables.hpp"

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "table")) {
        for (int32_t n = -1440; n <= 1440; ++n) {
            int32_t c = 0, s = 0;
            ssw::angle_table(n, &c, &s);
            std::printf("%d %d %d\n", (int)n, (int)c, (int)s);
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "rungs") && argc % 2 == 0) {
        for (int i = 2; i + 1 < argc; i += 2) {
            int j0 = 0, j1 = 0;
            const bool ok = ssw::angle_rungs(std::strtod(argv[i], nullptr), std::strtod(argv[i + 1], nullptr), &j0, &j1);
            std::printf("%d %d %d\n", ok ? 1 : 0, j0, j1);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: angle_tables_test table | rungs LO HI ...\n");
    return 2;
}
