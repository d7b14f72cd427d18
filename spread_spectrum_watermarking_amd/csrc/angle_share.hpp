// Share-groups of the angle search inside ssw_rotate_search_attack_rgb8 (angle.hip: angle_cost_shared_kernel), shared by angle.hip
// and tests/cpp/angle_share_test.cpp; it compiles without HIP.  A share-group is at most ANGLE_SHARE_MAX suspects that have the
// original in common and one list of candidate angles: the kernel makes the turned values of a (candidate, tile) once and
// compares them with every member that wants the candidate.  The ladder's candidates are the rungs and every member wants every
// rung; the refinement's are the union of the members' slot lists (angle_keep_kernel writes them), and a member wants only the
// angles of its own list -- its sums go to its own slot, so the pick per suspect never sees a neighbour's candidates.
// tests/test_rotate_search_cpp_cpu.py restates both functions in Python.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "angle_tables.hpp"

namespace ssw {

constexpr unsigned ANGLE_SHARE_MAX = 16;                 // members of a share-group
constexpr uint8_t ANGLE_SHARE_NONE = 255;                // ShareCand::slot of a member that does not want the candidate
constexpr int32_t ANGLE_SLOT_SKIP = INT32_MIN;           // a slot that holds no angle (angle.hip: ANG_SKIP)
static_assert(ANGLE_SLOTS < ANGLE_SHARE_NONE, "a slot index fits a byte beside the marker");

// member[m]: the suspect's index in its group of planes; cands first_cand .. first_cand + n_cands - 1 (the refinement)
struct ShareGroup { uint32_t n_members, first_cand, n_cands, spare; uint32_t member[ANGLE_SHARE_MAX]; };
// one candidate of the refinement: the angle, bit m of `mask` set when member m wants it, and the slot of that member's list it is
struct ShareCand { int32_t a; uint32_t mask; uint8_t slot[ANGLE_SHARE_MAX]; };
static_assert(sizeof(ShareGroup) == 80 && sizeof(ShareCand) == 24, "as the kernel reads them");

// The share-groups of n suspects: suspects whose keys (6 doubles each: the matrix that turned them) compare equal go together in
// the order they come, in chunks of ANGLE_SHARE_MAX; groups in the order of their first member.
inline std::vector<ShareGroup> angle_share_groups(const std::vector<const double*>& keys) {
    std::vector<ShareGroup> out;
    std::vector<size_t> open;                            // per distinct key: the group that still takes members
    std::vector<const double*> seen;
    for (size_t i = 0; i < keys.size(); ++i) {
        size_t k = 0;
        while (k < seen.size() && !std::equal(keys[i], keys[i] + 6, seen[k])) ++k;
        if (k == seen.size()) { seen.push_back(keys[i]); open.push_back(SIZE_MAX); }
        if (open[k] == SIZE_MAX || out[open[k]].n_members == ANGLE_SHARE_MAX) { open[k] = out.size(); out.push_back(ShareGroup{}); }
        ShareGroup& g = out[open[k]];
        g.member[g.n_members++] = (uint32_t)i;
    }
    return out;
}

// The refinement's candidates: slots [suspect][ANGLE_SLOTS] as angle_keep_kernel leaves them (a suspect's angles are distinct).
// Per group the union of its members' angles in ascending order, appended to `cands`; first_cand and n_cands are set.
inline void angle_share_cands(const int32_t* slots, std::vector<ShareGroup>& groups, std::vector<ShareCand>& cands) {
    cands.clear();
    for (ShareGroup& g : groups) {
        std::vector<int32_t> all;
        for (uint32_t m = 0; m < g.n_members; ++m)
            for (unsigned t = 0; t < ANGLE_SLOTS; ++t) {
                const int32_t a = slots[(size_t)g.member[m] * ANGLE_SLOTS + t];
                if (a != ANGLE_SLOT_SKIP) all.push_back(a);
            }
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        g.first_cand = (uint32_t)cands.size();
        g.n_cands = (uint32_t)all.size();
        for (const int32_t a : all) {
            ShareCand c{};
            c.a = a;
            std::fill(c.slot, c.slot + ANGLE_SHARE_MAX, ANGLE_SHARE_NONE);
            cands.push_back(c);
        }
        for (uint32_t m = 0; m < g.n_members; ++m)
            for (unsigned t = 0; t < ANGLE_SLOTS; ++t) {
                const int32_t a = slots[(size_t)g.member[m] * ANGLE_SLOTS + t];
                if (a == ANGLE_SLOT_SKIP) continue;
                ShareCand& c = cands[g.first_cand + (size_t)(std::lower_bound(all.begin(), all.end(), a) - all.begin())];
                if (c.slot[m] != ANGLE_SHARE_NONE) continue;            // (a list with a repeated angle: its first slot)
                c.mask |= 1u << m;
                c.slot[m] = (uint8_t)t;
            }
    }
}

}  // namespace ssw
