// The strategy of every pass of the 2-D transform, decided once.  Host code only: plan_pass takes the shape
// and a snapshot of the context's settings, reads the strategy thresholds of the tuning table once, and names the builder of
// ssw_pipeline.hip that runs the pass and the cross-pass facts its launches need (PairLayout, PrepFamily).
#pragma once

#include <cstddef>
#include <cstdint>

namespace ssw {

// Dense GEMMs (dct.hip: every shape the pair path does not take, and SSW_PRECISION_F32); the f64 operand-ready pair path at
// one, two or three folding levels; deep pre-passes (one pre-pass for all launches, level 1 or level 2 = every launch sums
// len/16 terms); FusedRows / FusedCols (r5: the row epilogue writes the column operands); SemiDeep(Inv) (columns of 8- but
// not 16-divisible length); DeepInv(L2).
enum class PassStrategy { Dense, PairL1, PairTwo, PairThree, Deep, DeepL2, FusedRows, FusedCols, SemiDeep, SemiDeepInv,
                          DeepInv, DeepInvL2 };
// Kernels of a deep / semi-deep column or deep inverse row pre-pass: at level 2, LDS-staged, or -- deep forward columns only --
// the kernel that reads a class-major plane of ONE tile (the row pass's length is no multiple of PREP_STAGED_TILE).
enum class PrepFamily { None, OneTile, Staged, L2 };
constexpr unsigned PREP_STAGED_TILE = 128;           // the LDS-staged pre-passes read class-major tiles of this many columns

// The plane between the passes as a launch sees it (dct_pair_common.hpp): class-major or natural; whether the transform's row
// pass runs at level 2, and its class tile width (both describe the row pass whichever pass launches).
struct PairLayout { bool class_major = false, rows_l2 = false; unsigned tile = 0; };
struct PlanSettings { bool fold = true; int fold_level = 5; bool split = true; };     // ssw_ctx: fold, fold_level, split
struct PlanInput {                  // (aggregate: the fields in this order)
    int type = 0, precision = 0;    // SSW_DCT*, SSW_PRECISION_*
    size_t n = 0, w = 0, h = 0;
    size_t full_h = 0;              // a band of rows of a frame this tall (0: the whole frame)
    bool natural_order = false;     // the plane between the passes stays in the natural column order
    bool aligned = true;            // source and destination planes are 16-byte aligned
    PlanSettings s;
};
struct PassPlan {
    PassStrategy strategy = PassStrategy::Dense;
    int levels = 0;                 // folding levels of the pair path along the pass (0: not the pair path)
    bool split = false;             // the odd half as rotated quarter-length cosine / sine pairs
    bool merge = false;             // a stage's classes in one launch (a single frame's launches are too small alone)
    PrepFamily prep = PrepFamily::None;
    PairLayout layout;              // class_major: this pass writes (rows) / reads (columns) the class-major plane
};
struct TransformPlan {
    bool rows_first = true;         // src/dct2d.rs:93-98
    PassPlan pass[2];               // in the order they run
    const PassPlan& rows() const { return pass[rows_first ? 0 : 1]; }
    const PassPlan& cols() const { return pass[rows_first ? 1 : 0]; }
};

PassPlan plan_pass(const PlanInput& in, bool first_pass, bool is_row);
TransformPlan plan_transform(const PlanInput& in);
uint32_t plan_flags(const TransformPlan& p);                 // SSW_PLAN_* of include/ssw.h
bool plan_is_level2(const PassPlan& p);                      // DeepL2, FusedRows, FusedCols, DeepInvL2
bool plan_is_deep(const PassPlan& p);                        // those, Deep and DeepInv
bool plan_merge(size_t lines);                               // the merge rule (merge_max_lines)
bool plan_derived_fused(const PassPlan& rows, size_t lines); // the pruned derived pass in one kernel (derived_fused)
// the (f64) pair path fits the shape: folding shapes, aligned planes, operand planes below 4 GB
bool dct_pair_can_run(size_t n_frames, size_t w, size_t h, bool aligned);
size_t plan_frame_limit(const PlanSettings& s, bool f64, size_t w, size_t h);      // frames per group (f64: 32-bit operand offsets)
// doubles of a lane's `deep` operand slot: what the passes of both directions of this shape use (they share the lane)
size_t split_scratch_elems(size_t n, size_t w, size_t h);

}  // namespace ssw
