// The transform planner (dct_plan.hpp): the strategy predicates of the 2-D transform and the one function that combines them.
// This unit is the only reader of the strategy thresholds of the tuning table (tuning.hip); they are read once per plan.
#include <algorithm>

#include "ssw_internal.hpp"
#include "dct_pair_common.hpp"

namespace ssw {
namespace {

struct PlanTuning {
    size_t efold_min, efold_inv_min, efold_cols_min, deep_min_rows, deep_min_cols, merge_max_lines;
    bool fuse_cols, derived_fused;
};
PlanTuning read_tuning() {
    auto z = [](int which) { return (size_t)tuning(which); };
    return {z(TUNE_EFOLD_MIN), z(TUNE_EFOLD_INV_MIN), z(TUNE_EFOLD_COLS_MIN), z(TUNE_DEEP_MIN_ROWS), z(TUNE_DEEP_MIN_COLS),
            z(TUNE_MERGE_MAX_LINES), z(TUNE_FUSE_COLS) != 0, z(TUNE_DERIVED_FUSED) != 0};
}

// the shape / alignment conditions of the folded transforms (the operand-ready path asks for them too)
bool rows_can_fold(size_t w, bool aligned) { return w >= 16 && w % 8 == 0 && aligned; }
bool cols_can_fold(size_t w, size_t h, bool aligned) { return h >= 16 && h % 8 == 0 && w % 4 == 0 && aligned; }
// second level: quarter length a multiple of 4 (rows read quads; the transposing column pre-pass needs an even quarter)
bool can_fold2(size_t len) { return len % 16 == 0 && len >= 64; }
bool can_fold2_cols(size_t len) { return len % 8 == 0 && len >= 64; }     // column passes: H % 8 == 0 suffices (1080 rows)
bool can_fold3(size_t len) { return len % 32 == 0 && len >= 128; }
// the odd half split once more (dct_pair_prep.hip "Split odd half"): any axis whose quarter length folds
bool can_split(size_t len) { return len % 8 == 0 && len >= 128; }
// deep pre-passes: forward rows (% 64), columns (% 16), inverse rows (% 128); semi-deep columns: % 8, not % 16 (1080 rows)
bool deep_rows(const PlanTuning& t, size_t len) { return len % 64 == 0 && len >= t.deep_min_rows; }
bool deep_cols(const PlanTuning& t, size_t len) { return len % 16 == 0 && len >= t.deep_min_cols; }
bool deep_inv_rows(const PlanTuning& t, size_t len) { return len % 128 == 0 && len >= t.deep_min_rows && len <= 128 * 256; }
bool semi_deep_cols(const PlanTuning& t, size_t len) { return len % 8 == 0 && len % 16 != 0 && len >= t.deep_min_cols; }
// The staged column kernels take the natural column order or class-major tiles of PREP_STAGED_TILE: not the class-major plane of
// a row pass whose length 128 does not divide (one tile as wide as the line, class_tile(), dct_pair_common.hpp).
bool staged_cols_ok(size_t w, bool class_major) {
    return w % 4 == 0 && w >= 4 && (!class_major || class_tile((unsigned)w) == PREP_STAGED_TILE);
}
// LEVEL 2 (r4b / r4c): forward rows of efold_min = 1280 columns or more, inverse rows of efold_inv_min, columns of
// efold_cols_min = 720 rows (natural order or 128-column class tiles).  Every launch sums len/16 terms: 240 at 4K rows, 79 % of peak
// against 84 % for len/8 at 2/3 of the multiply-adds; K = 135 columns at 50 TFLOP/s against 64 for 270 at half of them.  Measured a gain
// from 1280 x 720 up, once the plane between the passes is class-major.
bool efold(const PlanTuning& t, size_t len) { return deep_rows(t, len) && len >= t.efold_min; }
bool efold_inv(const PlanTuning& t, size_t len) { return deep_inv_rows(t, len) && len >= t.efold_inv_min; }
bool efold_cols(const PlanTuning& t, size_t h, size_t w, bool class_major) {
    return deep_cols(t, h) && staged_cols_ok(w, class_major) && h >= t.efold_cols_min;
}
// Can the column pre-pass of an `fh`-row plane read the class-major order of a deep row pass?  The deep kernels all can, the
// semi-deep ones (staged only) when 128 divides the row length; and the column pass reaches those strategies only through the
// split (fh >= 128).
bool cols_read_class_major(const PlanTuning& t, size_t fh, size_t w) {
    return can_fold2_cols(fh) && can_split(fh) && (deep_cols(t, fh) || (semi_deep_cols(t, fh) && staged_cols_ok(w, true)));
}
// the GEMM launcher's rule: 64-line tiles when 128-line ones (x 8 classes when merged) would not fill 448 block slots
bool launch_is_small(const PlanTuning& t, size_t lines, size_t pairs) {
    const unsigned long long classes = lines <= t.merge_max_lines ? 8 : 1;
    return (unsigned long long)((lines + 127) / 128) * ((pairs + 63) / 64) * classes < 448;
}
// r5, fused forward transform: rows first, both passes at level 2, 128-frequency class tiles, column planes exactly as wide
// as the padded units, both passes on 128-line tiles (small batches keep the unfused path).  The column pass must take its
// deep strategy by itself (can_split): else it would read an f32 plane the fused row pass never wrote.
bool can_fuse_cols(const PlanTuning& t, size_t n_frames, size_t w, size_t h) {
    if (!t.fuse_cols || n_frames == 0 || w < h || w % 128 != 0 || h % 16 != 0) return false;
    if (!efold(t, w) || !efold_cols(t, h, w, true) || !can_split(h) || !can_fold2_cols(h)) return false;
    const size_t hup = dct_pair_fused_units(h);
    if (pair_kpad(h / 8) != hup) return false;
    if (n_frames * 16 * hup > 0xFFFFFFFFull || n_frames * w > 0xFFFFFFFFull) return false;      // 32-bit line indices in both passes
    return !launch_is_small(t, n_frames * 16 * hup, w / 16) && !launch_is_small(t, n_frames * w, h / 16);
}

PassPlan plan_pass_t(const PlanTuning& t, const PlanInput& in, bool first_pass, bool is_row) {
    PassPlan p;
    const bool inverse = in.type == SSW_DCT3, f64 = in.precision == SSW_PRECISION_F64;
    const size_t n = in.n, w = in.w, h = in.h, len = is_row ? w : h;
    const PlanSettings& s = in.s;
    p.merge = (is_row ? n * h : n * w) <= t.merge_max_lines;
    p.layout.rows_l2 = inverse ? efold_inv(t, w) : efold(t, w);
    p.layout.tile = class_tile((unsigned)w);
    const bool can_fold = s.fold && (is_row ? rows_can_fold(w, in.aligned) : cols_can_fold(w, h, in.aligned));
    if (!(can_fold && s.fold_level >= 3 && f64 && dct_pair_can_run(n, w, h, in.aligned))) return p;        // Dense
    const bool two = s.fold_level >= 4 && (is_row ? can_fold2(len) : can_fold2_cols(len));
    // a third level pays once the sums are long enough (4K: +1.6 %, 1080p: -3 %); level 6 forces it
    const bool three = two && !inverse && can_fold3(len) && (s.fold_level >= 6 || (s.fold_level == 5 && len >= 3072));
    p.levels = three ? 3 : two ? 2 : 1;
    // the odd half as a rotated pair of quarter-length cosine / sine transforms: a quarter of its multiply-adds
    p.split = two && s.split && can_split(len);
    // rows first, both passes deep: the row pass writes the plane between the passes class-major, the column pre-pass reads it
    const size_t fh = in.full_h ? in.full_h : h;
    const bool cm = !in.natural_order && w >= fh && w % 4 == 0 && (inverse ? deep_inv_rows(t, w) : deep_rows(t, w)) &&
                    cols_read_class_major(t, fh, w) && is_row == first_pass;
    // column pre-pass: level 2 and staged read the natural order or 128-column class tiles; a class-major plane whose row length
    // 128 does not divide is one tile, which only the deep forward kernel of dct_pair_prep.hip reads (cols_read_class_major)
    auto col_prep = [&](bool l2) { return l2 ? PrepFamily::L2 : staged_cols_ok(w, cm) ? PrepFamily::Staged : PrepFamily::OneTile; };
    const bool deep = p.split && (is_row ? (inverse ? deep_inv_rows(t, len) : deep_rows(t, len)) : deep_cols(t, len) && w % 4 == 0);
    if (deep) {
        p.layout.class_major = cm;
        const bool l2 = is_row ? (inverse ? efold_inv(t, len) : efold(t, len)) : efold_cols(t, len, w, cm);
        if (inverse) {
            p.strategy = l2 ? PassStrategy::DeepInvL2 : PassStrategy::DeepInv;
            p.prep = !is_row ? col_prep(l2) : l2 ? PrepFamily::L2 : PrepFamily::Staged;
        } else if (l2 && cm && !in.full_h && can_fuse_cols(t, n, w, h)) {
            p.strategy = is_row ? PassStrategy::FusedRows : PassStrategy::FusedCols;
            if (is_row) p.merge = n * 16 * dct_pair_fused_units(h) <= t.merge_max_lines;      // the unit-ordered, padded lines
        } else {
            p.strategy = l2 ? PassStrategy::DeepL2 : PassStrategy::Deep;
            if (!is_row) p.prep = col_prep(l2);
        }
        return p;
    }
    if (p.split && !is_row && semi_deep_cols(t, len) && w % 4 == 0) {
        p.strategy = inverse ? PassStrategy::SemiDeepInv : PassStrategy::SemiDeep;
        p.layout.class_major = cm;
        p.prep = col_prep(false);
        return p;
    }
    p.strategy = three ? PassStrategy::PairThree : two ? PassStrategy::PairTwo : PassStrategy::PairL1;
    return p;
}

}  // namespace

PassPlan plan_pass(const PlanInput& in, bool first_pass, bool is_row) { return plan_pass_t(read_tuning(), in, first_pass, is_row); }

TransformPlan plan_transform(const PlanInput& in) {
    const PlanTuning t = read_tuning();
    const bool rf = in.w >= in.h;
    return {rf, {plan_pass_t(t, in, true, rf), plan_pass_t(t, in, false, !rf)}};
}

uint32_t plan_flags(const TransformPlan& p) {
    const PassPlan &r = p.rows(), &c = p.cols();
    return (r.levels > 0 || c.levels > 0 ? SSW_PLAN_PAIR_F64 : 0) | (plan_is_deep(r) ? SSW_PLAN_ROWS_DEEP : 0) |
           (plan_is_deep(c) ? SSW_PLAN_COLS_DEEP : 0) | (plan_is_level2(r) ? SSW_PLAN_ROWS_LEVEL2 : 0) |
           (plan_is_level2(c) ? SSW_PLAN_COLS_LEVEL2 : 0) | (r.layout.class_major ? SSW_PLAN_CLASS_MAJOR : 0) |
           (c.strategy == PassStrategy::FusedCols ? SSW_PLAN_FUSED_COLS : 0);
}

bool plan_is_level2(const PassPlan& p) {
    typedef PassStrategy S;
    return p.strategy == S::DeepL2 || p.strategy == S::FusedRows || p.strategy == S::FusedCols || p.strategy == S::DeepInvL2;
}
bool plan_is_deep(const PassPlan& p) { return plan_is_level2(p) || p.strategy == PassStrategy::Deep || p.strategy == PassStrategy::DeepInv; }

bool plan_merge(size_t lines) { return lines <= (size_t)tuning(TUNE_MERGE_MAX_LINES); }

// r5: marks of up to 1024 entries at level 2 -- the whole pruned row pass in one kernel; a single frame (135 blocks of 16
// lines for 256 CUs) takes the merged launches instead, 35 us faster there
bool plan_derived_fused(const PassPlan& rows, size_t lines) {
    const PlanTuning t = read_tuning();
    return t.derived_fused && plan_is_level2(rows) && lines > t.merge_max_lines;
}

bool dct_pair_can_run(size_t n_frames, size_t w, size_t h, bool aligned) {
    // an operand plane must stay below 4 GB (32-bit scalar offsets walk its k-blocks)
    return rows_can_fold(w, aligned) && cols_can_fold(w, h, aligned) && w % 8 == 0 && h % 8 == 0 &&
           dct_pair_operand_elems(n_frames, w, h) * sizeof(double) <= 0xFFFFFFFFull;
}

bool dct_pair_can_prep_from_rgb(size_t w, size_t h, const void* rgb, PixFmt fmt) {
    return w >= h && can_fold2(w) && (reinterpret_cast<uintptr_t>(rgb) & pix_align_mask(fmt)) == 0;
}

size_t plan_frame_limit(const PlanSettings& s, bool f64, size_t w, size_t h) {
    // Dense f32 group size: SSW_PRECISION_F32 has no operand planes (it runs dense), but its frames keep the groups the planes of
    // a retired f32 pair path set (k-steps of 16 floats, an even number of them), so that its dense launches stay as they were.
    auto f32_kpad = [](size_t len) { return (len / 2 + 31) / 32 * 32; };
    const size_t per_frame = f64 ? dct_pair_operand_elems(1, w, h) * sizeof(double)
                                 : std::max(h * f32_kpad(w), w * f32_kpad(h)) * sizeof(float);
    const size_t m = per_frame && s.fold && s.fold_level >= 3 ? 0xFFFFFFFFull / per_frame : 0;
    return m >= 1 ? m : ~(size_t)0;
}

size_t split_scratch_elems(size_t n, size_t w, size_t h) {
    const PlanTuning t = read_tuning();
    size_t e = dct_pair_split_elems(n, w, h);
    if (deep_rows(t, w) || deep_inv_rows(t, w)) e = std::max(e, dct_pair_deep_elems(n * h, w));
    if (deep_cols(t, h)) e = std::max(e, dct_pair_deep_elems(n * w, h));
    if (can_fuse_cols(t, n, w, h)) e = std::max(e, dct_pair_deep_elems(n * 16 * dct_pair_fused_units(h), w));      // unit-ordered, padded lines
    if (semi_deep_cols(t, h)) e = std::max(e, dct_pair_semi_deep_elems(n * w, h));
    return e;
}

}  // namespace ssw
