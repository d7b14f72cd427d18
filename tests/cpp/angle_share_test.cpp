// The host side of the shared angle search (csrc/angle_share.hpp) on slot lists a test hands it: the share-groups and, per group,
// the union of its members' candidates with who wants which and at which slot.  A program of its own:
// tests/test_rotate_search_cpp_cpu.py writes the cases, runs it plain and under ASan/UBSan and compares with a restatement.
//   input (the file argv[1]): the number of suspects n; n key numbers (equal numbers: turned by one matrix); n lists of 60 slots
//   output: "G n_members first_cand n_cands member..." per group, then "C a mask slot0 .. slot15" per candidate
#include <array>
#include <cstdio>
#include <vector>

#include "angle_share.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    size_t n = 0;
    if (std::fscanf(f, "%zu", &n) != 1) return 2;
    std::vector<std::array<double, 6>> mats(n);
    for (size_t i = 0; i < n; ++i) {
        long key = 0;
        if (std::fscanf(f, "%ld", &key) != 1) return 2;
        mats[i] = {{1.0, 0.0, (double)key, -0.0, 1.0, 0.5 * (double)key}};      // (-0.0 equals 0.0: keys compare by value)
    }
    std::vector<int32_t> slots(n * ssw::ANGLE_SLOTS);
    for (int32_t& s : slots) {
        long v = 0;
        if (std::fscanf(f, "%ld", &v) != 1) return 2;
        s = (int32_t)v;
    }
    std::fclose(f);
    std::vector<const double*> keys(n);
    for (size_t i = 0; i < n; ++i) keys[i] = mats[i].data();
    std::vector<ssw::ShareGroup> groups = ssw::angle_share_groups(keys);
    std::vector<ssw::ShareCand> cands;
    ssw::angle_share_cands(slots.data(), groups, cands);
    for (const ssw::ShareGroup& g : groups) {
        std::printf("G %u %u %u", g.n_members, g.first_cand, g.n_cands);
        for (uint32_t m = 0; m < g.n_members; ++m) std::printf(" %u", g.member[m]);
        std::printf("\n");
    }
    for (const ssw::ShareCand& c : cands) {
        std::printf("C %d %u", c.a, c.mask);
        for (unsigned m = 0; m < ssw::ANGLE_SHARE_MAX; ++m) std::printf(" %u", (unsigned)c.slot[m]);
        std::printf("\n");
    }
    return 0;
}
