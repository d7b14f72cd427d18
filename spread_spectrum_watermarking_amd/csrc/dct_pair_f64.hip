// The launchers of the operand-ready f64 GEMM (dct_pair_f64_kernel.hpp describes the kernel, dct_pair_class.hpp the launch
// classes) and its forward template instances; the inverse instances are dct_pair_f64_inv*.hip.
#include "dct_pair_common.hpp"

#include <cstdlib>
#include <type_traits>

#ifdef SSW_TILE_TRACE
namespace ssw {
// diagnostic build only: per block (thread 0) the 100 MHz wall clock at entry, after the first tile is staged, after
// the main loop and after the epilogue, plus the hardware id (XCC / SE / CU) -- tools/tile_trace.py
__device__ unsigned long long* g_tile_trace = nullptr;
__device__ unsigned int g_tile_trace_cap = 0;
__device__ unsigned int g_tile_trace_n = 0;
__device__ unsigned int* g_tile_kstep = nullptr;        // [cap][32] per-k-step stamps (tools/tile_trace.py --ksteps)
extern "C" int ssw_debug_set_tile_kstep(void* dev_ptr) {
    unsigned int* p = static_cast<unsigned int*>(dev_ptr);
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tile_kstep), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
extern "C" int ssw_debug_set_tile_trace(void* dev_ptr, unsigned cap) {
    unsigned long long* p = static_cast<unsigned long long*>(dev_ptr);
    unsigned zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_tile_trace), &p, sizeof(p)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_tile_trace_cap), &cap, sizeof(cap)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_tile_trace_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
extern "C" int ssw_debug_get_tile_trace_count(unsigned* n) {
    return hipMemcpyFromSymbol(n, HIP_SYMBOL(g_tile_trace_n), sizeof(*n)) == hipSuccess ? 0 : -1;
}
}  // namespace ssw
#endif
#include "dct_pair_f64_kernel.hpp"
#if defined(SSW_TILE_TRACE) && !defined(SSW_TILE_TRACE_FWD_ONLY)
#define SSW_INV_PART -1
#include "dct_pair_f64_inv.inc"      // the diagnostic build keeps one unit (one set of trace globals)
#endif                               // (-DSSW_TILE_TRACE_FWD_ONLY: only the forward instances trace; the inverse ones come from the normal objects: 3 min instead of 9)

namespace ssw {


// One launch over `n_classes` classes (see PairMulti) of the same lines and the same template instance: the per-class
// arguments come from the class table (pair_class_args), the rest here is what belongs to the launch -- tile sizes, the
// shared output description, the instance.  x*, y*: k-blocked planes.
// A forward transform of n frames whose row launches write the column operands themselves (EPI_FWD_COLOP): whether a
// transform takes it is the planner's decision (dct_plan.hip, PassStrategy::FusedRows / FusedCols).

int launch_dct_pair_gemm_multi_f64(hipStream_t st, bool is_row, bool inverse, int n_classes, const PairClassDesc* desc, float* out,
                                   double* tmp, size_t n_frames, size_t w, size_t h, Epilogue ep, const RgbSink* sink, double* tmp_out,
                                   const PairLayout& lay, const FuseCols* fuse) {
    if (n_frames == 0 || n_classes == 0) return SSW_OK;
    if (n_classes < 0 || n_classes > 8 || !desc) return SSW_ERR_BAD_ARG;
    if (w > 0xFFFFFFull || h > 0xFFFFFFull) return SSW_ERR_BAD_DIMS;
    // fused forward transform: the row launches (fuse->cop set) run over the unit-ordered, padded lines and write the
    // column operands; the column launches (fuse set, cop null) read their tiles in the row launches' class-major order
    const bool fuse_rows = fuse && fuse->mode == FUSE_ROWS_COP, fuse_cols = fuse && fuse->mode == FUSE_COLS;
    if (fuse && (!(fuse_rows || fuse_cols) || fuse_rows != is_row || inverse || w % 128 != 0 || h % 16 != 0 ||
                 pair_kpad(h / 8) != dct_pair_fused_units(h))) return SSW_ERR_BAD_ARG;
    if (fuse_rows && (!lay.class_major || sink || !fuse->cop || !fuse->rot1 || !fuse->rot2 || !fuse->rot3)) return SSW_ERR_BAD_ARG;
    // pruned base reader: the part this launch is, on the pass it belongs to and with the pointers it reads
    typedef BasePart P;
    const P part = fuse ? fuse->part : P::None;
    const bool energy = part == P::EnergyRows || part == P::HeadRows, gated = part == P::TailRows || part == P::Phase2Cols;
    const bool col_part = part == P::Phase1Cols || part == P::Phase2Cols;
    if (part != P::None && (col_part ? !fuse_cols : !fuse_rows)) return SSW_ERR_BAD_ARG;
    if ((energy && !fuse->energy) || (gated && !fuse->need)) return SSW_ERR_BAD_ARG;
    const size_t lines = fuse_rows ? n_frames * 16 * dct_pair_fused_units(h) : is_row ? n_frames * h : n_frames * w;
    const size_t len = is_row ? w : h;
    if (lines > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
    const unsigned L = (unsigned)lines;
    const bool with_sink = sink && sink->rgb;
    PairMulti ml;
    PairInstance inst{0, false, 0};
    unsigned tiles_n = 0, leff0 = 0;
    const bool tile48 = tuning(TUNE_TILE48) != 0;                 // A/B switch
    for (int c = 0; c < n_classes; ++c) {
        PairInstance ic{0, false, 0};
        PairClassArgs& ca = ml.c[c];
        SSW_TRY(pair_class_args(desc[c].cls, is_row, inverse, len, lay, with_sink, tmp_out != nullptr, tile48, ca, ic));
        ca.x1 = desc[c].x1; ca.x2 = desc[c].x2; ca.y1 = desc[c].y1; ca.y2 = desc[c].y2;
        const unsigned ninv = inverse ? (unsigned)(len / pair_class_row(desc[c].cls).inv_ndiv) : 0u;      // the transform whose positions it writes
        if (c == 0) { inst = ic; leff0 = ninv; }
        else if (!(ic == inst) && !(ic.epi == inst.epi && ic.samex == inst.samex && n_classes > 1)) return SSW_ERR_BAD_ARG;
        if (ninv != leff0) return SSW_ERR_BAD_ARG;      // po.n is shared
        if ((unsigned long long)ml.c[c].Kp * L * 8 > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;   // scalar k-block offsets are 32-bit
        tiles_n += ml.c[c].tiles_n;
    }
    if (n_classes > 1) inst.subname = inverse ? inst.subname : 3;
    // 64-line tiles when 128-line ones would not fill the 512 block slots of the chip (2 per CU)
    const bool small = (unsigned long long)((L + 127) / 128) * tiles_n < 448;
    if (fuse && small) return SSW_ERR_BAD_ARG;
    // low-precision tail bound (base_energy.hip): the head launches run tile column 0 of every class, the gated tail
    // launches the others (the planner sized the launch by all of them: `small` above)
    if (part == P::HeadRows || part == P::TailRows) {
        tiles_n = 0;
        for (int c = 0; c < n_classes; ++c) {
            PairClassArgs& ca = ml.c[c];
            if (!base_tail_class_ok(ca)) return SSW_ERR_BAD_ARG;
            if (part == P::HeadRows) ca.tiles_n = 1;
            else { ca.tn0 = 1; ca.tiles_n -= 1; }
            tiles_n += ca.tiles_n;
        }
    }
    const unsigned BM = small ? 64 : 128;
    if (small)                                                     // 48-pair tiles are three pair tiles of a 128-line block
        for (int c = 0; c < n_classes; ++c)
            if (ml.c[c].bn32 == 2) { tiles_n -= ml.c[c].tiles_n; ml.c[c].bn32 = 0; ml.c[c].tiles_n = (ml.c[c].NP + 63) / 64; tiles_n += ml.c[c].tiles_n; }
    // (phase 1 of a pruned base reader computes one 128-line tile per frame: its grid is that small, the kernel maps it)
    const unsigned tiles_m = part == P::Phase1Cols ? (unsigned)n_frames : (L + BM - 1) / BM;
    // ... and 32-pair tiles when that spreads such a (single-class) launch more evenly over the 256 CUs (all its blocks are
    // resident at once, so a launch takes as long as the fullest CU): balance = blocks / (256 * ceil(blocks / 256)); the
    // smaller tiles reuse their basis fragments less, hence the 8 % handicap
    if (small && n_classes == 1) {
        const int force = (int)tuning(TUNE_BN32);
        auto balance = [](unsigned long long n) { return (double)n / (256.0 * (double)((n + 255) / 256)); };
        const unsigned tn32 = (ml.c[0].NP + 31) / 32;
        const bool bn32 = force >= 0 ? force != 0 : 0.92 * balance((unsigned long long)tiles_m * tn32) > balance((unsigned long long)tiles_m * tiles_n);
        if (bn32) { ml.c[0].tiles_n = tiles_n = tn32; ml.c[0].bn32 = 1; }
    }
    const unsigned long long nblk = (unsigned long long)tiles_m * tiles_n;
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    ml.n_classes = (unsigned)n_classes; ml.L = L; ml.tiles_m = tiles_m; ml.tiles_n_total = tiles_n;
    PairOut po{out, tmp, (unsigned)w, (unsigned)h, (unsigned)(inverse ? leff0 : len), 0, 1, 2};
    po.tmp_out = tmp_out;
    const PairClass c0 = desc[0].cls;
    if (lay.class_major && inverse && pair_class_row(c0).split && c0 != PairClass::R2A) { po.cm = lay.rows_l2 ? 2u : 1u; po.cmt = lay.tile; }
    // level 2: T2 (written by R2 rotated, read by the half-length launches AS2 BD2 | AD2 BS2) keeps the mod-4 class order, so
    // that those launches read runs instead of two doubles of every four
    if (lay.class_major && inverse && c0 == PairClass::R2A) po.cm = 1;
    if (lay.class_major && inverse && is_row && lay.rows_l2 && (c0 == PairClass::E2 || c0 == PairClass::O2)) po.tcm = 1;
    if (lay.class_major && !inverse) po.ft = lay.tile;
    if (fuse_rows) {
        if (inst.samex || inst.epi != EPI_FWD || po.ft != 128) return SSW_ERR_BAD_ARG;
        po.cop = fuse->cop; po.cop_k16 = (unsigned)pair_kpad(h / 8); po.cop_lines = (unsigned)(n_frames * w);
        po.cop_hup = (unsigned)dct_pair_fused_units(h);
        po.crot1 = fuse->rot1; po.crot2 = fuse->rot2; po.crot3 = fuse->rot3;
        inst.epi = EPI_FWD_COLOP;
    }
    if (fuse_cols) po.xperm = 1;
    po.col_energy = energy ? fuse->energy : nullptr;
    ml.need = nullptr; ml.need_mode = 0; ml.need_tpf = 1;
    if (col_part) {                                      // need_mode: 1 = the grid over tile 0, 2 = the flagged tiles beyond it
        if (inst.epi != EPI_FWD || inst.samex || small) return SSW_ERR_BAD_ARG;
        ml.need = fuse->need; ml.need_mode = part == P::Phase1Cols ? 1u : 2u; ml.need_tpf = (unsigned)(w / 128);
    }
    if (part == P::TailRows) {
        if (po.ft != 128) return SSW_ERR_BAD_ARG;
        ml.need = fuse->need; ml.need_tpf = (unsigned)(w / 128);
        ml.tail = fuse->tail; ml.tail_flop = fuse->tail_flop; ml.tail_bytes = fuse->tail_bytes;
    }
    auto al = [](const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    po.wide = (!is_row && w % 4 == 0 && al(out, 16) && (n_frames * w) % 4 == 0 && (!tmp || al(tmp, 16)) && (!tmp_out || al(tmp_out, 16))) ? 1u : 0u;
    if (with_sink && !(al(sink->iq_i, 16) && al(sink->iq_q, 16) && al(sink->rgb, sink->u8 ? 4 : 16))) po.wide = 0;
    if (with_sink) {
        if (is_row) return SSW_ERR_BAD_ARG;
        po.iq_i = sink->iq_i; po.iq_q = sink->iq_q; po.rgb = sink->rgb; po.rgb_u8 = sink->u8 ? 1u : 0u;
    }
    ml.po = po;
    switch (inst.epi) {
    case EPI_FWD_COLOP:
        // (the energy instances are named SUB + 10: the writer's row launches stay the kernels they were)
        if (part == P::TailRows) SSW_LAUNCH_PAIR_BM(false, EPI_FWD_COLOP, false, 5, 128);      // (the gated tail launches: one instance)
        else if (energy) { if (inst.subname == 4) SSW_LAUNCH_PAIR_BM(false, EPI_FWD_COLOP, false, 14, 128); else SSW_LAUNCH_PAIR_BM(false, EPI_FWD_COLOP, false, 13, 128); }
        else if (inst.subname == 4) SSW_LAUNCH_PAIR_BM(false, EPI_FWD_COLOP, false, 4, 128);
        else SSW_LAUNCH_PAIR_BM(false, EPI_FWD_COLOP, false, 3, 128);
        break;
    case EPI_FWD_ADJ: SSW_LAUNCH_PAIR(false, EPI_FWD_ADJ, false); break;
    case EPI_FWD:
        if (ml.need_mode) SSW_LAUNCH_PAIR_BM(true, EPI_FWD, false, 13, 128);      // (the two phases of a pruned base reader: eight classes, one launch)
        else if (inst.subname == 4) SSW_LAUNCH_PAIR_SUB(false, EPI_FWD, false, 4);
        else if (inst.subname == 3) { if (is_row) SSW_LAUNCH_PAIR_SUB(false, EPI_FWD, false, 3); else SSW_LAUNCH_PAIR_SUB(true, EPI_FWD, false, 3); }
        else if (inst.samex) SSW_LAUNCH_ROWCOL(EPI_FWD, true);
        else SSW_LAUNCH_ROWCOL(EPI_FWD, false);
        break;
    default: return launch_pair_gemm_inverse_instances(st, ml, ep, inst, is_row, small, nblk);
    }
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// Forward row pass restricted to a gathered set of frequencies (pruned derived transform, prune.hip): one
// shared image operand `x` (k-blocked, Kp wide) against a gathered half basis `y` of `cap` rows (k-blocked,
// [Kp / 8][cap][8]); row j of y produces compact output column off + j of `out` (row stride out_stride).
// Same kernel, operands and k order as the full transform's launches -> bit-identical values.
int launch_dct_pair_gemm_rows_subset_f64(hipStream_t st, const double* x, const double* y, unsigned cap, unsigned Kp, float* out,
                                         unsigned out_stride, unsigned off, size_t lines) {
    if (lines == 0 || cap == 0) return SSW_OK;
    if (lines > 0xFFFFFFFFull || (cap & 1)) return SSW_ERR_BAD_DIMS;
    const unsigned L = (unsigned)lines, NP = cap / 2;
    const unsigned tiles_m = (L + 127) / 128, tiles_n = (NP + 63) / 64;
    const unsigned long long nblk = (unsigned long long)tiles_m * tiles_n;
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    if ((unsigned long long)Kp * L * sizeof(double) > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
    PairMulti ml;
    ml.c[0] = PairClassArgs{x, x, y, y + (size_t)NP * 8, NP, Kp, cap, tiles_n, off, off + NP, 1, 0, 0xFFFFFFFFu, 0, 0, 0};
    ml.n_classes = 1; ml.L = L; ml.tiles_m = tiles_m; ml.tiles_n_total = tiles_n;
    ml.po = PairOut{out, nullptr, out_stride, 0, 0, off, off + NP, 1};
    const Epilogue ep{1.f, 1.f};
    pair_gemm_f64_kernel<false, EPI_FWD, true, 2><<<(unsigned)nblk, PT, 0, st>>>(ml, ep);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// The same for a class of the split odd half: gathered cosine rows `y1` and gathered sine rows `y2` (negated where the
// output is the difference) against the class's operand pair; pair j -> compact column off + j = acc1 + acc2.
int launch_dct_pair_gemm_rows_subset_split_f64(hipStream_t st, const double* x1, const double* x2, const double* y1, const double* y2,
                                               unsigned cap, unsigned Kp, float* out, unsigned out_stride, unsigned off, size_t lines) {
    if (lines == 0 || cap == 0) return SSW_OK;
    if (lines > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
    const unsigned L = (unsigned)lines, NP = cap;
    const unsigned tiles_m = (L + 127) / 128, tiles_n = (NP + 63) / 64;
    const unsigned long long nblk = (unsigned long long)tiles_m * tiles_n;
    if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    if ((unsigned long long)Kp * L * sizeof(double) > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
    PairMulti ml;
    ml.c[0] = PairClassArgs{x1, x2, y1, y2, NP, Kp, cap, tiles_n, off, 0, 1, 2, 0xFFFFFFFFu, 0, 0, 0};
    ml.n_classes = 1; ml.L = L; ml.tiles_m = tiles_m; ml.tiles_n_total = tiles_n;
    ml.po = PairOut{out, nullptr, out_stride, 0, 0, off, 0, 1};
    const Epilogue ep{1.f, 1.f};
    pair_gemm_f64_kernel<false, EPI_FWD, false, 3><<<(unsigned)nblk, PT, 0, st>>>(ml, ep);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

// Small passes (a single frame's derived transform: 17 tile rows, one or two tile columns per class -- nine launches of
// 13-22 us each, every one a fraction of the chip's block slots): the classes of one kind side by side in one launch's tile
// grid, like the merged launches of the full passes.  classes[c].x2 != nullptr: a class of the split odd half.
int launch_dct_pair_gemm_rows_subset_merged_f64(hipStream_t st, const PairSubsetClass* classes, unsigned n_classes, float* out,
                                                unsigned out_stride, size_t lines) {
    if (lines == 0) return SSW_OK;
    if (lines > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
    const unsigned L = (unsigned)lines, tiles_m = (L + 127) / 128;
    for (int split = 0; split < 2; ++split) {
        PairMulti ml;
        ml.n_classes = 0; ml.L = L; ml.tiles_m = tiles_m; ml.tiles_n_total = 0;
        auto flush = [&]() -> int {
            if (ml.n_classes == 0) return SSW_OK;
            const unsigned long long nblk = (unsigned long long)tiles_m * ml.tiles_n_total;
            if (nblk > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
            ml.po = PairOut{out, nullptr, out_stride, 0, 0, 0, 0, 1};
            const Epilogue ep{1.f, 1.f};
            if (split) pair_gemm_f64_kernel<false, EPI_FWD, false, 3><<<(unsigned)nblk, PT, 0, st>>>(ml, ep);
            else       pair_gemm_f64_kernel<false, EPI_FWD, true, 2><<<(unsigned)nblk, PT, 0, st>>>(ml, ep);
            SSW_HIP_CHECK(hipGetLastError());
            ml.n_classes = 0; ml.tiles_n_total = 0;
            return SSW_OK;
        };
        for (unsigned c = 0; c < n_classes; ++c) {
            const PairSubsetClass& k = classes[c];
            if ((k.x2 != nullptr) != (split != 0) || k.cap == 0) continue;
            if (!split && (k.cap & 1)) return SSW_ERR_BAD_DIMS;
            if ((unsigned long long)k.Kp * L * sizeof(double) > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;
            const unsigned NP = split ? k.cap : k.cap / 2, tiles_n = (NP + 63) / 64;
            if (split) ml.c[ml.n_classes] = PairClassArgs{k.x1, k.x2, k.y1, k.y2, NP, k.Kp, k.cap, tiles_n, k.off, 0, 1, 2, 0xFFFFFFFFu, 0, 0, 0};
            else       ml.c[ml.n_classes] = PairClassArgs{k.x1, k.x1, k.y1, k.y1 + (size_t)NP * 8, NP, k.Kp, k.cap, tiles_n, k.off, k.off + NP, 1, 0, 0xFFFFFFFFu, 0, 0, 0};
            ml.tiles_n_total += tiles_n;
            if (++ml.n_classes == 8) SSW_TRY(flush());
        }
        SSW_TRY(flush());
    }
    return SSW_OK;
}

}  // namespace ssw
