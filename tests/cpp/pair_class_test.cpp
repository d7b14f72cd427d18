// Host-side check of the launch-class table (csrc/dct_pair_class.hpp).  No GPU, no context.
//  (1) Replay: tests/golden/pair_class_parent.txt holds what the launcher's per-class function answered BEFORE the table
//      existed -- for every (kind 0..9, sub 0..2, row / column, forward / inverse, five layouts, sink, tmp_out, seven lengths,
//      tile48) either the status or every argument and the template instance -- and the class rows of the pruned plan.  The
//      table must answer the same on all 33600 tuples, the rejected ones included; a (kind, sub) that names no class is
//      "no such row".
//  (2) The table against its neighbours: every forward class's frequency map equals ForwardClassLayout's natural(pos(slot, i));
//      the classes of a level-2 pass and of a deep level-1 pass partition the frequencies; the flop of the eight level-2 classes
//      is eight times that of O rotated "+", as the set-up of build_deep_l2 assumes (level2_pass).
//  (3) The class sources of the pruned row pass: tests/golden/prune_class_src_parent.txt holds what build_pruned_derived's own
//      loop resolved per class of the plan BEFORE prune_class_sources existed (row plans of 3840, 1920, 1024 at level 2, 512
//      deep at level 1, 1040 split and not split); the function must answer the same, and prune_gathered_offsets must lay the
//      gathered bases out back to back in whole tiles of 16 rows.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../spread_spectrum_watermarking_amd/csrc/dct_pair_common.hpp"

using namespace ssw;
typedef PairClass C;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s (line %d): ", #cond, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the class a recorded (kind, sub, direction) named; Count: none
static C legacy_class(int kind, int sub, bool inverse) {
    static const C by_sub[5][3] = {{C::OneLevel, C::Count, C::Count}, {C::EvenHalf, C::R1R2, C::R1A}, {C::OddHalf, C::OddHalf2, C::OddHalf4},
                                   {C::E, C::E2, C::E4}, {C::O, C::O2, C::O4}};
    static const C level2[5] = {C::EE, C::EO, C::O5, C::O3, C::R2A};
    if (kind < 5) return by_sub[kind][sub];
    if (kind == 9) return sub == (inverse ? 2 : 0) ? C::R2A : C::Count;      // recorded at sub 0 forward, sub 2 inverse
    return sub == 0 ? level2[kind - 5] : C::Count;
}

static int replay(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("FAIL cannot open %s\n", path); return 1; }
    const size_t lens[7] = {256, 1080, 1920, 2160, 3840, 4320, 7680};
    char line[512];
    int kind = 0, sub = 0, is_row = 0, inverse = 0, layout = 0, at = 56;
    long tuples = 0, groups = 0, prune_plans = 0;
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        if (line[0] == 'G') {
            CHECK(at == 56, "group before %d %d %d %d %d has %d tuples", kind, sub, is_row, inverse, layout, at);
            if (std::sscanf(line + 1, "%d %d %d %d %d", &kind, &sub, &is_row, &inverse, &layout) != 5) { std::printf("FAIL bad line %s", line); return 1; }
            at = 0; ++groups;
        } else if (line[0] == 'R' || line[0] == 'A') {
            long count = 0; int status = SSW_OK, epi = 0, samex = 0, subname = 0;
            unsigned v[14] = {0};
            if (line[0] == 'R') { if (std::sscanf(line + 1, "%ld %d", &count, &status) != 2) { std::printf("FAIL bad line %s", line); return 1; } }
            else if (std::sscanf(line + 1, "%ld %u %u %u %u %u %u %u %u %u %u %u %u %u %u %d %d %d", &count, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7],
                                 &v[8], &v[9], &v[10], &v[11], &v[12], &v[13], &epi, &samex, &subname) != 18) { std::printf("FAIL bad line %s", line); return 1; }
            for (long i = 0; i < count; ++i, ++at, ++tuples) {
                if (at >= 56) { std::printf("FAIL group overflows: %s", line); return 1; }
                const size_t len = lens[at / 8];
                const bool sink = (at >> 2) & 1, tmp_out = (at >> 1) & 1, tile48 = at & 1;
                PairLayout lay;
                lay.class_major = layout != 0; lay.rows_l2 = layout >= 3;
                lay.tile = layout == 0 ? 0u : (layout == 1 || layout == 3) ? (unsigned)len : 128u;
                PairClassArgs ca;
                PairInstance in{-1, false, -1};
                std::memset(&ca, 0xEE, sizeof ca);
                const int rc = pair_class_args(legacy_class(kind, sub, inverse != 0), is_row != 0, inverse != 0, len, lay, sink, tmp_out, tile48, ca, in);
                const unsigned got[14] = {ca.NP, ca.Kp, ca.yrows, ca.tiles_n, ca.c1, ca.c2, ca.cs, ca.pm, ca.np1, ca.p2lo, ca.bn32, ca.fold0, ca.gsh, ca.e2off};
                CHECK(rc == status, "status %d, recorded %d: kind %d sub %d row %d inverse %d layout %d tuple %d", rc, status, kind, sub, is_row, inverse, layout, at);
                if (rc != SSW_OK || status != SSW_OK) continue;
                for (int k = 0; k < 14; ++k)
                    CHECK(got[k] == v[k], "field %d = %u, recorded %u: kind %d sub %d row %d inverse %d layout %d tuple %d", k, got[k], v[k], kind, sub, is_row, inverse, layout, at);
                CHECK(in.epi == epi && (int)in.samex == samex && in.subname == subname, "instance {%d %d %d}, recorded {%d %d %d}: kind %d sub %d row %d inverse %d layout %d tuple %d",
                      in.epi, (int)in.samex, in.subname, epi, samex, subname, kind, sub, is_row, inverse, layout, at);
            }
        } else if (line[0] == 'P') {
            int variant = 0; unsigned cap = 0, n = 0;
            if (std::sscanf(line + 1, "%d %u %u", &variant, &cap, &n) != 3 || variant < 0 || variant > 6) { std::printf("FAIL bad line %s", line); return 1; }
            PassPlan rows;      // 0 level 2; deep level 1: 1 split, 2 not; two levels: 3 split, 4 not; three levels: 5 split, 6 not
            rows.strategy = variant == 0 ? PassStrategy::DeepL2 : variant <= 2 ? PassStrategy::Deep : variant <= 4 ? PassStrategy::PairTwo : PassStrategy::PairThree;
            rows.levels = variant >= 5 ? 3 : 2;
            rows.split = variant == 0 || (variant & 1);
            C cls[8];
            PrunePlan plan;
            prune_plan_classes(cls, prune_class_list(rows, cls), cap, plan);
            CHECK(plan.n_classes == n, "pruned plan %d cap %u: %u classes, recorded %u", variant, cap, plan.n_classes, n);
            for (unsigned c = 0; c < n; ++c) {
                unsigned r[6] = {0};
                if (!std::fgets(line, sizeof line, f) || std::sscanf(line, "%u %u %u %u %u %u", &r[0], &r[1], &r[2], &r[3], &r[4], &r[5]) != 6) { std::printf("FAIL bad prune row\n"); return 1; }
                if (c >= plan.n_classes) continue;
                const PruneClass& k = plan.c[c];
                CHECK(k.mod == r[0] && k.rem == r[1] && k.cap == r[2] && k.off == r[3] && k.rem2 == r[4] && k.radd == r[5],
                      "pruned plan %d cap %u class %u: (%u %u %u %u %u %u), recorded (%u %u %u %u %u %u)", variant, cap, c, k.mod, k.rem, k.cap, k.off, k.rem2, k.radd,
                      r[0], r[1], r[2], r[3], r[4], r[5]);
            }
            ++prune_plans;
        } else { std::printf("FAIL bad line %s", line); return 1; }
    }
    std::fclose(f);
    CHECK(at == 56 && groups == 600 && tuples == 33600, "the recording has %ld groups, %ld tuples", groups, tuples);
    CHECK(prune_plans == 21, "the recording has %ld pruned plans", prune_plans);
    return 0;
}

// the frequencies class c produces on a line of length len: first outputs of pairs 0 .. NP-1, second outputs of the same
// pairs -- of pairs 1 .. NP for a class of E's shape (frequency cs p - r), NP pairs on for a shared operand
static void frequencies(C c, unsigned len, std::vector<unsigned>& first, std::vector<unsigned>& second) {
    const PairClassRow& r = pair_class_row(c);
    const unsigned np = len / r.ldiv / r.np_div;
    first.clear(); second.clear();
    for (unsigned p = 0; p < np; ++p) {
        first.push_back((unsigned)r.fwd.r1 + r.fwd.cs * p);
        second.push_back((unsigned)r.fwd.r2 + r.fwd.cs * (p + (r.eshape ? 1u : r.samex ? np : 0u)));
    }
}

static void neighbours() {
    std::vector<unsigned> f1, f2;
    for (unsigned len : {256u, 1920u, 3840u}) {
        for (unsigned tile : {128u, len})
            for (bool level2 : {false, true}) {
                const ForwardClassLayout fl{len, tile, level2};
                for (int c = 0; c < (int)C::Count; ++c) {
                    const PairClassRow& r = kPairClasses[c];
                    const int slot = level2 ? r.slot2 : r.slot1;
                    if (slot < 0) continue;
                    CHECK(r.class_major, "%s has a slot", r.name);
                    frequencies((C)c, len, f1, f2);
                    CHECK(f1.size() == len / fl.mod(slot) && fl.mod(slot) == r.fwd.cs, "%s: entries of slot %d at %u", r.name, slot, len);
                    for (unsigned i = 0; i < f1.size(); ++i) {
                        CHECK(fl.natural(fl.pos(slot, i)) == f1[i], "%s: first output %u at len %u tile %u", r.name, i, len, tile);
                        CHECK(fl.natural(fl.pos(slot + 1, i)) == f2[i], "%s: second output %u at len %u tile %u", r.name, i, len, tile);
                    }
                }
            }
        // the classes of one pass partition the frequencies
        const std::vector<C> level2(kLevel2Classes, kLevel2Classes + 8), deep1 = {C::R1R2, C::E2, C::O2, C::E, C::O};
        for (const std::vector<C>* pass : {&level2, &deep1}) {
            std::vector<int> seen(len, 0);
            for (C c : *pass) {
                frequencies(c, len, f1, f2);
                for (const std::vector<unsigned>* fs : {&f1, &f2})
                    for (unsigned u : *fs) { CHECK(u < len, "%s: frequency %u of %u", pair_class_row(c).name, u, len); if (u < len) ++seen[u]; }
            }
            for (unsigned u = 0; u < len; ++u) CHECK(seen[u] == 1, "frequency %u of %u is produced %d times", u, len, seen[u]);
        }
        double flop = 0.0;
        for (C c : level2) flop += pair_class_flop(c, 1000, len);
        CHECK(flop == 8.0 * pair_class_flop(C::O5, 1000, len), "level-2 flop at %u", len);
        CHECK(pair_class_flop(C::O5, 1000, len) == 4.0 * 1000.0 * (len / 16) * (len / 16), "flop of O rotated \"+\" at %u", len);
    }
}

static int sources(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("FAIL cannot open %s\n", path); return 1; }
    char line[256];
    int plans = 0;
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        unsigned w = 0, n = 0; int strategy = 0, levels = 0, split = 0;
        if (std::sscanf(line, "S %u %d %d %d %u", &w, &strategy, &levels, &split, &n) != 5 || n > 9) { std::printf("FAIL bad line %s", line); return 1; }
        PassPlan rows;
        rows.strategy = (PassStrategy)strategy; rows.levels = levels; rows.split = split != 0;
        C cls[8];
        const int n_cls = prune_class_list(rows, cls);
        PruneClassSrc src[9];
        PrunePlan plan;
        const unsigned cap = 128;
        prune_plan_classes(cls, n_cls, cap, plan);
        const int got = prune_class_sources(cls, n_cls, rows, w, src);
        CHECK(got == (int)n && plan.n_classes == n, "width %u: %d sources, %u plan classes, recorded %u", w, got, plan.n_classes, n);
        for (unsigned c = 0; c < n; ++c) {
            int r[10] = {0};
            if (!std::fgets(line, sizeof line, f) || std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d", &r[0], &r[1], &r[2], &r[3], &r[4], &r[5], &r[6], &r[7], &r[8], &r[9]) != 10) {
                std::printf("FAIL bad source row\n"); return 1;
            }
            if ((int)c >= got) continue;
            const PruneClassSrc& s = src[c];
            CHECK(s.p1 == r[0] && s.p2 == r[1] && (int)s.y1 == r[2] && (!s.split || (int)s.y2 == r[3]) && (s.split || r[3] == -1), "width %u class %u: planes %d %d bases %d %d, recorded %d %d %d %d",
                  w, c, s.p1, s.p2, (int)s.y1, (int)s.y2, r[0], r[1], r[2], r[3]);
            CHECK((int)s.ydiv == r[4] && (int)s.src_rows == r[5] && (int)s.Kp == r[6] && (int)s.ktrue == r[7] && (int)s.split == r[8] && s.lane_buf == r[9],
                  "width %u class %u: (%u %u %u %u %d %d), recorded (%d %d %d %d %d %d)", w, c, s.ydiv, s.src_rows, s.Kp, s.ktrue, (int)s.split, s.lane_buf, r[4], r[5], r[6], r[7], r[8], r[9]);
        }
        // the gathered bases: [Kp][cap rounded up to 16] doubles per basis, a split class's two one after the other, no gaps
        size_t at = 0;
        const size_t total = prune_gathered_offsets(plan, src);
        for (unsigned c = 0; c < plan.n_classes && (int)c < got; ++c) {
            const size_t bytes = (size_t)src[c].Kp * ((plan.c[c].cap + 15) & ~15u) * 8;
            CHECK(src[c].goff == at, "width %u class %u: gathered offset %zu, expected %zu", w, c, src[c].goff, at);
            at += bytes;
            CHECK(src[c].goff2 == at, "width %u class %u: second gathered offset %zu, expected %zu", w, c, src[c].goff2, at);
            if (src[c].split) at += bytes;
        }
        CHECK(total == at, "width %u: gathered bytes %zu, expected %zu", w, total, at);
        ++plans;
    }
    std::fclose(f);
    CHECK(plans == 6, "the recording has %d source plans", plans);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: pair_class_test <recording> <class sources>\n"); return 2; }
    if (replay(argv[1])) return 1;
    if (sources(argv[2])) return 1;
    neighbours();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
