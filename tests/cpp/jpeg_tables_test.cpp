// Host-only check of csrc/jpeg_tables.hpp (tests/test_jpeg_cpu.py builds and runs it):
//   1. the quantiser's division: the high half of n * jpeg_reciprocal(d) equals n / d for EVERY divisor d = 8 .. 2040 (8 q and
//      everything between) and EVERY numerator n = 0 .. 2^17 + 1020 -- about 2.7e8 pairs, a second or two;
//   2. prints the two tables of every quality, one line each ("q <quality> <64 luma> <64 chroma>"), for the Python test to
//      compare with its own restatement of libjpeg's scaling rule.
#include <cstdint>
#include <cstdio>

#include "jpeg_tables.hpp"

int main() {
    const uint32_t n_max = (1u << 17) + 1020u;
    unsigned divisors = 0;
    for (uint32_t d = 8; d <= 2040; ++d, ++divisors) {
        const uint32_t m = ssw::jpeg_reciprocal(d);
        for (uint32_t n = 0; n <= n_max; ++n)
            if (ssw::jpeg_divide(n, m) != n / d) {
                std::printf("%u / %u: got %u, want %u\n", n, d, ssw::jpeg_divide(n, m), n / d);
                return 1;
            }
    }
    std::printf("checked %u divisors, numerators 0 .. %u\n", divisors, n_max);
    for (uint32_t q = 1; q <= 100; ++q) {
        uint8_t l[64], c[64];
        ssw::jpeg_qtable(ssw::JPEG_LUMA, q, l);
        ssw::jpeg_qtable(ssw::JPEG_CHROMA, q, c);
        std::printf("q %u", q);
        for (int i = 0; i < 64; ++i) std::printf(" %u", l[i]);
        for (int i = 0; i < 64; ++i) std::printf(" %u", c[i]);
        std::printf("\n");
    }
    return 0;
}
