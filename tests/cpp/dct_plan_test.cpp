// Host-side check of the transform planner (csrc/dct_plan.hpp): the plans DESIGN §4.0 names, the folding levels and the odd
// split off, lowered thresholds through ssw_tuning_set, and the SSW_PLAN_* flags as a function of the plan.  No GPU and no
// context: the planner takes the shape and a snapshot of the settings.
#include <cstdio>
#include <initializer_list>
#include "../../include/ssw.h"
#include "../../spread_spectrum_watermarking_amd/csrc/dct_plan.hpp"

using namespace ssw;
typedef PassStrategy S;

static int failures = 0;
#define CHECK(cond, what) do { if (!(cond)) { std::printf("FAIL %s: %s (line %d)\n", what, #cond, __LINE__); ++failures; } } while (0)

static TransformPlan plan(size_t n, size_t w, size_t h, int type = SSW_DCT2, PlanSettings s = PlanSettings()) {
    PlanInput in;
    in.type = type; in.precision = SSW_PRECISION_F64;
    in.n = n; in.w = w; in.h = h;
    in.s = s;
    return plan_transform(in);
}
static PlanSettings level(int l) { PlanSettings s; s.fold = l != 0; s.fold_level = l; return s; }

enum : uint32_t { PAIR = SSW_PLAN_PAIR_F64, RD = SSW_PLAN_ROWS_DEEP, CD = SSW_PLAN_COLS_DEEP, R2 = SSW_PLAN_ROWS_LEVEL2,
                  C2 = SSW_PLAN_COLS_LEVEL2, CM = SSW_PLAN_CLASS_MAJOR, FUSED = SSW_PLAN_FUSED_COLS };

int main() {
    // 4K, forward: batches of 7 frames and more, and 1-2 frames (one launch per stage) fused at level 2; 3-6 frames unfused,
    // level 2, class-major (64-line tiles: the column operands would not be whole k-blocks)
    for (size_t n : {1, 2, 7, 8, 128}) {
        const TransformPlan p = plan(n, 3840, 2160);
        CHECK(p.rows_first && p.rows().strategy == S::FusedRows && p.cols().strategy == S::FusedCols, "4K fused");
        CHECK(p.rows().layout.class_major && p.rows().layout.rows_l2 && p.rows().layout.tile == 128, "4K fused layout");
        CHECK(p.rows().merge == (n <= 2) && p.cols().merge == (n <= 2), "4K fused merge");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | C2 | CM | FUSED), "4K fused flags");
    }
    for (size_t n : {3, 4, 5, 6}) {
        const TransformPlan p = plan(n, 3840, 2160);
        CHECK(p.rows().strategy == S::DeepL2 && p.cols().strategy == S::DeepL2, "4K unfused level 2");
        CHECK(p.rows().layout.class_major && p.cols().layout.class_major && p.cols().prep == PrepFamily::L2, "4K unfused class-major");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | C2 | CM), "4K unfused flags");
    }
    // the inverse is never fused
    for (size_t n : {1, 2, 4, 128}) {
        const TransformPlan p = plan(n, 3840, 2160, SSW_DCT3);
        CHECK(p.rows().strategy == S::DeepInvL2 && p.cols().strategy == S::DeepInvL2, "4K inverse");
        CHECK(p.rows().prep == PrepFamily::L2 && p.cols().prep == PrepFamily::L2 && p.rows().layout.class_major, "4K inverse pre-passes");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | C2 | CM), "4K inverse flags");
    }
    // 1920 x 1080: level-2 rows over semi-deep columns (the staged pre-pass reads the class-major plane)
    {
        const TransformPlan p = plan(256, 1920, 1080);
        CHECK(p.rows().strategy == S::DeepL2 && p.cols().strategy == S::SemiDeep, "1080p");
        CHECK(p.cols().layout.class_major && p.cols().prep == PrepFamily::Staged, "1080p columns");
        CHECK(plan_flags(p) == (PAIR | RD | R2 | CM), "1080p flags");
        const TransformPlan q = plan(12, 1920, 1080, SSW_DCT3);
        CHECK(q.rows().strategy == S::DeepInvL2 && q.cols().strategy == S::SemiDeepInv && q.cols().prep == PrepFamily::Staged, "1080p inverse");
        CHECK(plan_flags(q) == (PAIR | RD | R2 | CM), "1080p inverse flags");
    }
    // 8K: fused from one frame on (one frame merges its classes)
    for (size_t n : {1, 2}) {
        const TransformPlan p = plan(n, 7680, 4320);
        CHECK(p.rows().strategy == S::FusedRows && p.cols().strategy == S::FusedCols && p.rows().merge == (n == 1), "8K");
        CHECK(plan(n, 7680, 4320, SSW_DCT3).cols().strategy == S::DeepInvL2, "8K inverse");
    }
    // 1280 x 720: both passes at level 2, too small a grid for the fusion
    {
        const TransformPlan p = plan(20, 1280, 720);
        CHECK(p.rows().strategy == S::DeepL2 && p.cols().strategy == S::DeepL2 && p.cols().prep == PrepFamily::L2, "720p");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | C2 | CM), "720p flags");
    }
    // 512 x 272: deep at level 1 (rows shorter than efold_min, columns than efold_cols_min), staged column pre-pass
    {
        const TransformPlan p = plan(40, 512, 272);
        CHECK(p.rows().strategy == S::Deep && p.cols().strategy == S::Deep && p.cols().prep == PrepFamily::Staged, "512x272");
        CHECK(!p.rows().merge && p.rows().layout.class_major && !p.rows().layout.rows_l2, "512x272 layout");
        CHECK(plan_flags(p) == (PAIR | RD | CD | CM), "512x272 flags");
        const TransformPlan q = plan(40, 512, 272, SSW_DCT3);
        CHECK(q.rows().strategy == S::DeepInv && q.cols().strategy == S::DeepInv && q.rows().prep == PrepFamily::Staged, "512x272 inverse");
    }
    // rows whose length 128 does not divide: the class-major plane is one tile as wide as the line, which the one-tile deep
    // forward column pre-pass reads (level 1: 320 x 256; behind a level-2 row pass: 1344 x 256).  The inverse has no
    // deep row pass there (it needs a multiple of 128), so its plane stays natural and its columns take the staged kernels.
    {
        const TransformPlan p = plan(3, 320, 256);
        CHECK(p.rows().strategy == S::Deep && p.rows().layout.class_major && p.rows().layout.tile == 320, "320x256 rows");
        CHECK(p.cols().strategy == S::Deep && p.cols().prep == PrepFamily::OneTile && p.cols().layout.class_major, "320x256 columns");
        CHECK(plan_flags(p) == (PAIR | RD | CD | CM), "320x256 flags");
        const TransformPlan q = plan(3, 1344, 256);
        CHECK(q.rows().strategy == S::DeepL2 && q.rows().layout.class_major && q.rows().layout.tile == 1344, "1344x256 rows");
        CHECK(q.cols().strategy == S::Deep && q.cols().prep == PrepFamily::OneTile && !plan_is_level2(q.cols()), "1344x256 columns");
        for (size_t w : {320, 1344}) {
            const TransformPlan r = plan(3, w, 256, SSW_DCT3);
            CHECK(!plan_is_deep(r.rows()) && !r.rows().layout.class_major && !r.cols().layout.class_major, "one-tile widths, inverse rows");
            CHECK(r.cols().strategy == S::DeepInv && r.cols().prep == PrepFamily::Staged, "one-tile widths, inverse columns");
        }
    }
    // the reference's 640 x 444 cat: 444 rows do not fold -- the dense kernels
    {
        const TransformPlan p = plan(3, 640, 444);
        CHECK(p.rows().strategy == S::Dense && p.cols().strategy == S::Dense && plan_flags(p) == 0, "640x444");
    }
    // SSW_PRECISION_F32 takes the dense kernels at every folding level (the pair path is f64 only)
    for (int l : {1, 3, 5, 6}) {
        PlanInput in;
        in.type = SSW_DCT2; in.precision = SSW_PRECISION_F32; in.n = 8; in.w = 3840; in.h = 2160; in.s = level(l);
        const TransformPlan p = plan_transform(in);
        CHECK(p.rows().strategy == S::Dense && p.cols().strategy == S::Dense && plan_flags(p) == 0, "f32 dense");
    }
    // folding levels 1 / 2 run dense too
    for (int l : {1, 2}) CHECK(plan(8, 3840, 2160, SSW_DCT2, level(l)).rows().strategy == S::Dense, "levels 1 / 2 dense");
    // frames per group of build_transform, both precisions: f64 keeps a pass's operand planes below 4 GB; f32 (dense) keeps the
    // group size it has always had (values recorded before the f32 pair path was removed)
    {
        struct Limit { size_t w, h, f64, f32; };
        const Limit limits[] = {{3840, 2160, 129, 257}, {7680, 4320, 32, 64}, {1920, 1080, 514, 1028}, {1280, 720, 1165, 2184},
                                {512, 272, 7710, 13107}, {256, 144, 29127, 43690}, {3840, 96, 2912, 4369}, {1024, 96, 10922, 16383},
                                {640, 444, 3744, 7489}};
        for (const Limit& l : limits) {
            CHECK(plan_frame_limit(PlanSettings(), true, l.w, l.h) == l.f64, "frame limit f64");
            CHECK(plan_frame_limit(PlanSettings(), false, l.w, l.h) == l.f32, "frame limit f32");
        }
        CHECK(plan_frame_limit(level(0), true, 3840, 2160) == ~(size_t)0 && plan_frame_limit(level(0), false, 3840, 2160) == ~(size_t)0,
              "level 0: no frame limit");
    }
    // unaligned planes take the dense kernels as well
    {
        PlanInput in;
        in.type = SSW_DCT2; in.precision = SSW_PRECISION_F64; in.n = 1; in.w = 3840; in.h = 2160; in.aligned = false;
        CHECK(plan_pass(in, true, true).strategy == S::Dense, "unaligned");
    }
    // folding levels: 0 dense, 3 one level, 4..6 as the default at 4K (the deep strategies take precedence over three levels)
    CHECK(plan(8, 3840, 2160, SSW_DCT2, level(0)).rows().strategy == S::Dense && plan_flags(plan(8, 3840, 2160, SSW_DCT2, level(0))) == 0, "level 0");
    for (int type : {SSW_DCT2, SSW_DCT3}) {
        const TransformPlan p = plan(8, 3840, 2160, type, level(3));
        CHECK(p.rows().strategy == S::PairL1 && p.cols().strategy == S::PairL1 && p.rows().levels == 1, "level 3");
        CHECK(plan_flags(p) == PAIR, "level 3 flags: the single-level path, nothing deep, nothing fused");
    }
    for (int l : {4, 5, 6}) CHECK(plan_flags(plan(8, 3840, 2160, SSW_DCT2, level(l))) == (PAIR | RD | CD | R2 | C2 | CM | FUSED), "levels 4-6");
    CHECK(plan(8, 1024, 96, SSW_DCT2, level(4)).rows().strategy == S::Deep, "level 4, short columns");
    CHECK(plan(8, 4096, 96, SSW_DCT2, level(6)).cols().strategy == S::PairTwo, "level 6, 96 rows: no third level on columns this short");
    // the odd split off: the pair GEMMs still run, without the deep strategies (three levels on 4K rows at level 5)
    {
        PlanSettings s;
        s.split = false;
        const TransformPlan p = plan(8, 3840, 2160, SSW_DCT2, s);
        CHECK(p.rows().strategy == S::PairThree && p.cols().strategy == S::PairTwo && !p.rows().split, "odd split off");
        CHECK(plan_flags(p) == PAIR, "odd split off flags");
        CHECK(plan(8, 3840, 2160, SSW_DCT3, s).rows().strategy == S::PairTwo, "odd split off, inverse");
    }
    // thresholds through the tuning table; the retired switches back to the r3 pre-passes are unknown names
    CHECK(ssw_tuning_set("prep_staged", 0) == SSW_ERR_BAD_ARG && ssw_tuning_set("class_tile", 0) == SSW_ERR_BAD_ARG, "retired switches");
    CHECK(ssw_tuning_set("fuse_cols", 0) == SSW_OK, "set fuse_cols");
    {
        const TransformPlan p = plan(128, 3840, 2160);
        CHECK(p.rows().strategy == S::DeepL2 && p.cols().strategy == S::DeepL2, "fuse_cols = 0");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | C2 | CM), "fuse_cols = 0 flags: the fusion off and nothing else");
    }
    ssw_tuning_reset(nullptr);
    CHECK(ssw_tuning_set("efold_cols_min", 800) == SSW_OK, "set efold_cols_min");
    {
        const TransformPlan p = plan(20, 1280, 720);
        CHECK(p.rows().strategy == S::DeepL2 && p.cols().strategy == S::Deep && p.cols().prep == PrepFamily::Staged, "efold_cols_min 800");
        CHECK(plan_flags(p) == (PAIR | RD | CD | R2 | CM), "efold_cols_min 800 flags");
    }
    ssw_tuning_reset(nullptr);
    CHECK(ssw_tuning_set("deep_min_cols", 4096) == SSW_OK, "set deep_min_cols");
    {
        const TransformPlan p = plan(8, 3840, 2160);
        CHECK(p.rows().strategy == S::DeepL2 && !p.rows().layout.class_major && p.cols().strategy == S::PairTwo, "deep_min_cols 4096");
        CHECK(plan_flags(p) == (PAIR | RD | R2), "deep_min_cols 4096 flags");
    }
    ssw_tuning_reset(nullptr);
    // with the column thresholds lowered below 128 rows the column pass cannot take its deep strategy (no split),
    // so the row pass must neither fuse nor write the class-major plane
    CHECK(ssw_tuning_set("deep_min_cols", 16) == SSW_OK && ssw_tuning_set("efold_cols_min", 16) == SSW_OK, "lower the column thresholds");
    {
        const TransformPlan p = plan(64, 3840, 96);
        CHECK(p.rows().strategy == S::DeepL2 && !p.rows().layout.class_major, "ADVICE r5 rows");
        CHECK(p.cols().strategy == S::PairTwo && !p.cols().layout.class_major, "ADVICE r5 columns");
        CHECK(plan_flags(p) == (PAIR | RD | R2), "ADVICE r5 flags");
        // 128 rows split: there the lowered thresholds take the deep level-2 columns behind a class-major row pass (not fused:
        // the column operands of 8 units would be narrower than the two k-blocks of a plane)
        const TransformPlan q = plan(64, 3840, 128);
        CHECK(q.rows().strategy == S::DeepL2 && q.rows().layout.class_major && q.cols().strategy == S::DeepL2, "lowered thresholds, 128 rows");
    }
    ssw_tuning_reset(nullptr);
    CHECK(ssw_tuning_set("merge_max_lines", 0) == SSW_OK, "set merge_max_lines");
    CHECK(!plan(1, 3840, 2160).rows().merge && !plan_merge(1), "merge_max_lines 0");
    ssw_tuning_reset(nullptr);
    // the flags are a function of the plan alone
    {
        TransformPlan p;
        p.rows_first = false;
        p.pass[0].strategy = S::SemiDeep; p.pass[0].levels = 2;            // the column pass, first
        p.pass[1].strategy = S::DeepInvL2; p.pass[1].levels = 2;           // the row pass
        CHECK(plan_flags(p) == (PAIR | RD | R2), "hand-made plan");
        p.pass[1].layout.class_major = true;
        p.pass[0].strategy = S::FusedCols;
        CHECK(plan_flags(p) == (PAIR | RD | R2 | CD | C2 | CM | FUSED), "hand-made plan, fused");
        TransformPlan d;
        CHECK(plan_flags(d) == 0, "dense plan");
    }
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
