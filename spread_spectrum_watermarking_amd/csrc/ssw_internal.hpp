// Internal declarations shared by the HIP translation units of libssw_hip.so.
// gfx950 (MI355X / CDNA4) only: wave64, MFMA, 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/ssw.h"
#include "dct_plan.hpp"
#include "dct_pair_class.hpp"

namespace ssw {

void set_last_error(const std::string& s);

#define SSW_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) {                                                         \
            ::ssw::set_last_error(std::string(#expr) + ": " + hipGetErrorString(e__));   \
            return (e__ == hipErrorOutOfMemory) ? SSW_ERR_OUT_OF_MEMORY : SSW_ERR_HIP;   \
        }                                                                                \
    } while (0)

#define SSW_TRY(expr)                         \
    do {                                      \
        int s__ = (expr);                     \
        if (s__ != SSW_OK) return s__;        \
    } while (0)

// ---- launchers implemented in the kernel translation units -----------------
// All are asynchronous on `st` and return the status of the launch.

// color.hip
int launch_rgb_to_yiq(hipStream_t st, const float* rgb, size_t npix, float* y, float* i, float* q);
int launch_yiq_to_rgb(hipStream_t st, const float* y, const float* i, const float* q, size_t npix,
                      float* rgb);
int launch_synth(hipStream_t st, uint32_t seed, uint32_t first_frame, size_t n_frames, size_t w,
                 size_t h, float* rgb);

// dct.hip
// Basis matrices, layout [out][sum], N x N:
//   forward: D[k][n] = 2 cos(pi k (2n+1) / 2N)          (rustdct DCT-II x the reference's x2)
//   inverse: E[n][k] = k == 0 ? 1/4 : cos(pi k (2n+1) / 2N) / 2   (rustdct DCT-III x 1/2)
size_t dense_basis_kpad(size_t n);   // row stride of a dense basis: N rounded up to 32, zero padded
int launch_make_basis_f32(hipStream_t st, size_t n, bool inverse, float* out);
int launch_make_basis_f64(hipStream_t st, size_t n, bool inverse, double* out);

struct Epilogue {    // stored value = f32(acc) * (output index == 0 ? first : base); both 1 = plain store
    float first, base;
};
// Row pass: out[r][v] = sum_c in[r][c] * basis[v][c]   for rows = n_frames*h rows of width w.
int launch_dct_rows(hipStream_t st, int precision, const float* in, float* out, size_t rows, size_t w,
                    const void* basis, Epilogue ep);
// Column pass: out[f][u][c] = sum_r basis[u][r] * in[f][r][c].
int launch_dct_cols(hipStream_t st, int precision, const float* in, float* out, size_t n_frames,
                    size_t w, size_t h, const void* basis, Epilogue ep);
// The f64 passes with the unrounded sums stored as f64 (no epilogue): the base plane of the fingerprint update
int launch_dct_rows_f64out(hipStream_t st, const float* in, double* out, size_t rows, size_t w, const double* basis);
int launch_dct_cols_f64out(hipStream_t st, const float* in, double* out, size_t n_frames, size_t w, size_t h, const double* basis);

// dct_pair_prep.hip / dct_pair_f64.hip: "operand-ready" folded GEMMs in f64 (no VALU work in the MFMA loop): pre-passes
// write the folded operands once per pass as k-blocked f64 planes, the half bases are cached in the same layout.
// Half bases: (N/2)x(N/2), layout [out][sum], parity 0 = even frequencies, 1 = odd.
size_t dct_pair_kpad(size_t n);                                         // row stride of operands / bases of a length-n axis
size_t dct_pair_operand_elems(size_t n_frames, size_t w, size_t h);     // elements per operand plane
int launch_make_half_basis_blocked(hipStream_t st, size_t n, bool inverse, int parity, double* out);
// one level: (S, D) forward / (E, O) inverse
int launch_dct_pair_prep(hipStream_t st, bool is_row, bool inverse, const float* in, size_t n_frames, size_t w, size_t h,
                         double* o1, double* o2);
// Sample format of an interleaved RGB frame at the boundary: what `into_rgb32f()` accepts (src/algorithm.rs:308, :476):
// f32 as it is, 8-bit v / 255, 16-bit v / 65535
enum class PixFmt { F32, U8, U16 };
constexpr size_t pix_bytes(PixFmt f) { return f == PixFmt::U8 ? 1 : f == PixFmt::U16 ? 2 : 4; }                 // per sample
constexpr unsigned pix_align_mask(PixFmt f) { return f == PixFmt::U8 ? 3u : f == PixFmt::U16 ? 7u : 15u; }     // of a 4-pixel load
bool dct_pair_can_prep_from_rgb(size_t w, size_t h, const void* rgb, PixFmt fmt);       // dct_plan.hip: a rows-first RGB pre-pass reads these frames
// What a forward row pre-pass reads: an f32 plane, or the interleaved RGB frame itself (Y formed on the fly)
enum class RowSrc { Plane, RgbF32, RgbU8, RgbU16 };
constexpr RowSrc row_src(PixFmt f) { return f == PixFmt::U8 ? RowSrc::RgbU8 : f == PixFmt::U16 ? RowSrc::RgbU16 : RowSrc::RgbF32; }
constexpr PixFmt pix_fmt(RowSrc s) { return s == RowSrc::RgbU8 ? PixFmt::U8 : s == RowSrc::RgbU16 ? PixFmt::U16 : PixFmt::F32; }   // of an RGB source
// ... and what it writes besides its operand planes: the I and Q planes (both or neither; RGB sources only -- the writer's)
struct RowInput {
    RowSrc kind; const void* p; float *i, *q;
    static RowInput plane(const float* y) { return {RowSrc::Plane, y, nullptr, nullptr}; }
    static RowInput rgb(PixFmt f, const void* frames, float* i = nullptr, float* q = nullptr) { return {row_src(f), frames, i, q}; }
};
// two levels: (SS, SD | EE, EO) [kpad(len/2) wide] and (D | O) [kpad(len) wide] in one sweep; column and inverse passes read a plane
int launch_dct_pair_prep4(hipStream_t st, bool is_row, bool inverse, const RowInput& in, size_t n_frames, size_t w, size_t h,
                          double* q1, double* q2, double* p);
// three levels on a forward row pass: (SSS, SS-) [kpad(w/4) wide], S- [kpad(w/2)], x- [kpad(w)]
int launch_dct_pair_prep8_rows(hipStream_t st, const RowInput& in, size_t n_frames, size_t w, size_t h,
                               double* r1, double* r2, double* m, double* p);
// Writer::result fused into the last inverse pass (EPI_INV_O_RGB): the frames' I / Q planes and the RGB output
struct RgbSink {
    const float* iq_i = nullptr;
    const float* iq_q = nullptr;
    void* rgb = nullptr;          // [n][h][w][3] f32, or u8 when `u8`
    bool u8 = false;
};
int launch_dct_pair_prep8_cols(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h,
                               double* r1, double* r2, double* m, double* p);
// r5, fused forward transform: how a launch takes part.
//   FUSE_ROWS_COP    row launch over the unit-ordered, padded lines whose epilogue writes the sixteen column-operand planes
//                    `cop`; needs the rotation tables of H, H/2, H/4
//   FUSE_COLS        column launch behind such a row pass: its 128-line tiles are in the row launches' class-major order
enum { FUSE_ROWS_COP = 1, FUSE_COLS = 2 };
// ... and which part of a pruned base reader (base_prune.hip, base_energy.hip) it is, with the pointers that part reads:
//   EnergyRows   row launch over every tile column; `energy` [n][W] receives the sum of squares of every column-operand
//                line's f32 row-pass values (atomic adds; zeroed by the caller)
//   HeadRows     low-precision tail bound: tile column 0 of every class only (the head: exact energies into `energy`)
//   TailRows     ... the other tile columns, each block gated on `need` (no energies); `tail`: [0] jobs that ran, [1] [2]
//                their flop / bytes as doubles, tail_flop / tail_bytes per pair of a job
//   Phase1Cols   column launch on a grid over column tile 0 of every frame only
//   Phase2Cols   column launch that runs the blocks of the tiles t > 0 whose need[frame * (W / 128) + t] is set
enum class BasePart { None, EnergyRows, HeadRows, TailRows, Phase1Cols, Phase2Cols };
struct FuseCols {
    int mode = 0; double* cop = nullptr; const double *rot1 = nullptr, *rot2 = nullptr, *rot3 = nullptr;
    BasePart part = BasePart::None;
    float* energy = nullptr;
    const unsigned* need = nullptr;
    unsigned long long* tail = nullptr;
    double tail_flop = 0.0, tail_bytes = 0.0;
};
// one or several classes (same lines, same template instance) in one launch: the class (dct_pair_class.hpp) with its operand
// and basis planes; sink (last inverse column pass): colour conversion in the epilogue
struct PairClassDesc { PairClass cls; const double *x1, *x2, *y1, *y2; };
int launch_dct_pair_gemm_multi_f64(hipStream_t st, bool is_row, bool inverse, int n_classes, const PairClassDesc* desc, float* out,
                                   double* tmp, size_t n_frames, size_t w, size_t h, Epilogue ep, const RgbSink* sink = nullptr,
                                   double* tmp_out = nullptr, const PairLayout& layout = PairLayout(), const FuseCols* fuse = nullptr);

int launch_dct_pair_gemm_rows_subset_f64(hipStream_t st, const double* x, const double* y, unsigned cap, unsigned Kp, float* out,
                                         unsigned out_stride, unsigned off, size_t lines);
int launch_dct_pair_gemm_rows_subset_split_f64(hipStream_t st, const double* x1, const double* x2, const double* y1, const double* y2,
                                               unsigned cap, unsigned Kp, float* out, unsigned out_stride, unsigned off, size_t lines);
// the classes of a small pruned row pass in one or two launches (x2 == nullptr: y1 holds cap gathered rows, pairs j / j + cap/2;
// else a class of the split odd half: y1 / y2 the gathered cosine / sine rows)
struct PairSubsetClass {
    const double *x1, *x2, *y1, *y2;
    unsigned cap, Kp, off;
};
int launch_dct_pair_gemm_rows_subset_merged_f64(hipStream_t st, const PairSubsetClass* classes, unsigned n_classes, float* out,
                                                unsigned out_stride, size_t lines);
// split odd half (f64 only; dct_pair_prep.hip "Split odd half"): quarter-length cosine / sine bases (which: 0 cosE, 1 sinE,
// 2 cosO, 3 sinO), the rotation table of an axis, and the pass that turns an odd operand plane into AS | BD | AD | BS
size_t dct_pair_split_kpad(size_t len);
// tuning.hip: the process-wide table of strategy thresholds / A-B switches (ssw_tuning_set, include/ssw.h)
enum { TUNE_EFOLD_MIN, TUNE_EFOLD_INV_MIN, TUNE_EFOLD_COLS_MIN, TUNE_DEEP_MIN_ROWS, TUNE_DEEP_MIN_COLS,
       TUNE_MERGE_MAX_LINES, TUNE_BN32, TUNE_BAND_SPLIT, TUNE_FUSE_COLS, TUNE_UPLOAD_BANDS, TUNE_SPECULATE_K, TUNE_PREP_LIGHT, TUNE_LANE_STAGGER, TUNE_DERIVED_FUSED, TUNE_TILE48, TUNE_BASE_PRUNE, TUNE_BASE_ENERGY_LOWP, TUNE_COUNT };
long long tuning(int which);
// the level-2 and LDS-staged forms of the deep forward column pre-pass (dct_pair_prep_staged.hip), as
// launch_dct_pair_prep16_cols calls them; PrepFamily::OneTile keeps the kernel of dct_pair_prep.hip
int launch_prep16_cols_l2(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                          const double* rot1, const double* rot2, const double* rot3, bool class_major, bool in_l2, unsigned K16);
int launch_prep16_cols_staged(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                              const double* rot1, const double* rot2, bool class_major, bool semi, unsigned K8, unsigned K16, bool efold);
size_t dct_pair_split_elems(size_t n_frames, size_t w, size_t h);
size_t dct_pair_split_basis_rows(size_t len, int which);
int launch_make_split_basis_blocked(hipStream_t st, size_t n, bool inverse, int which, double* out);
int launch_make_rot_table(hipStream_t st, size_t n, double* out);
int launch_dct_pair_rotate(hipStream_t st, const double* p, const double* rot, double* sp, size_t lines, size_t len);
// deep forward row pre-pass (len % 64 == 0): D and SD split, SS folded a third time, in one sweep over the source
// (a RowInput); base: AS BD AD BS R1 R2 (lines * split_kpad(len) each), AS2 BD2 AD2 BS2 (lines * split_kpad(len/2))
size_t dct_pair_semi_deep_elems(size_t lines, size_t len);
// deep inverse pre-passes (dct_pair_prep_staged.hip: coefficient plane -> the same ten planes; R1 = c[8q], R2 = c[8q+4]);
// `prep` / `lay`: of the plan
int launch_dct_pair_prep16_inv_rows(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                                    const double* rot1, const double* rot2, const double* rot3, PrepFamily prep);
int launch_dct_pair_prep16_inv_cols(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                                    const double* rot1, const double* rot2, const double* rot3, PrepFamily prep, const PairLayout& lay);
int launch_dct_pair_prep16_cols(hipStream_t st, const float* in, size_t n_frames, size_t w, size_t h, double* base,
                                const double* rot1, const double* rot2, const double* rot3, PrepFamily prep, const PairLayout& lay);
size_t dct_pair_deep_elems(size_t lines, size_t len);
// l2: the row pass runs at level 2 (sixteen planes K16 wide); unit_order: the fused transform's line order (needs l2)
int launch_dct_pair_prep16_rows(hipStream_t st, const RowInput& in, size_t n_frames, size_t w, size_t h, double* base,
                                const double* rot1, const double* rot2, const double* rot3, bool l2, bool unit_order = false);
// r5, fused forward transform: units per frame of the row pass's line order (H/16 rounded up to whole k-blocks of 8)
inline size_t dct_pair_fused_units(size_t h) { return ((h / 16 + 7) / 8) * 8; }

// prune.hip: the derived frame's transform restricted to the frequency columns a chunk's index lists use
// v is in the class when v % mod == rem, or == rem2 (classes of the split odd half: there the output is the cosine
// part MINUS the sine part and the gathered sine row is negated); basis row (v + radd) / mod
constexpr unsigned PRUNE_NO_REM = 0xFFFFFFFFu;
constexpr uint32_t PRUNE_NEG = 0x40000000u;              // rows[] flag: negate the gathered sine row
constexpr unsigned SSW_PRUNE_INFO = 16;                  // u32 words of a chunk's info block: [0] overflow flag, [1 + c] members of class c
struct PruneClass { unsigned mod, rem, cap, off, rem2 = PRUNE_NO_REM, radd = 0; };
struct PrunePlan {
    unsigned n_classes = 0;
    PruneClass c[9];        // info[] of launch_prune_build: SSW_PRUNE_INFO words, 1 + one per class
    unsigned W = 0, cap_total = 0;
};
static_assert(SSW_PRUNE_INFO >= 1 + sizeof(PrunePlan::c) / sizeof(PruneClass), "a chunk's info block holds the flag and one count per class");
int launch_prune_build(hipStream_t st, const uint32_t* idx, size_t n_frames, size_t k, const PrunePlan& plan,
                       uint32_t* flag /*[W]*/, uint32_t* rows /*[cap_total]*/, uint32_t* pos /*[W]*/, uint32_t* info /*[SSW_PRUNE_INFO]*/);
// one gathered basis: rows[] of `src` ([kblocks][src_rows] 64-byte pieces) into `dst` ([kblocks][cap]); `negate`: rows flagged
// PRUNE_NEG change sign (f64 sine rows)
struct PruneGatherJob {
    const uint32_t* rows;
    const char* src;
    char* dst;
    unsigned cap, src_rows, kblocks, first_block;
    bool negate;
    bool frag = false;         // MFMA B-fragment order for the fused derived pass (whole tiles of 16 rows)
};
struct PruneGatherJobs {
    PruneGatherJob j[18];
    unsigned n;
};
int launch_prune_gather_bases(hipStream_t st, PruneGatherJobs jobs);
int launch_extract_pruned(hipStream_t st, const float* base, const float* compact, size_t n_frames, size_t w, size_t h,
                          size_t cap, const uint32_t* pos, const uint32_t* indices, size_t k, int method, float alpha,
                          float* out);

// base_prune.hip: the base reader's column pass only where a column can hold one of the first k keys.
constexpr unsigned SSW_BASE_PRUNE_TILE = 128;
// The context's counters: one device block of SSW_BASE_PRUNE_STATS 64-bit words.  The kernels get sub-blocks of it by pointer
// and index them: the decide kernel `stats` (from `tiles`) and `work` (from `col_flop`), the gated tail row launches `tail`
// (from `tail_jobs`, the doubles behind it as [1] [2]) -- hence the offsets below.
constexpr unsigned SSW_BASE_PRUNE_STATS = 16;
struct BasePruneCounters {
    unsigned long long tiles, tiles_computed, frames_extended;      // frames_extended: frames whose second phase computed a tile
    unsigned long long pad0;
    double col_flop, col_bytes, select_bytes;      // second phase: the column launches' computed tiles, the masked selection's reads of them
    unsigned long long pad1;
    unsigned long long tail_jobs;                  // a frame's tile column of one class of the gated row launches (base_energy.hip)
    double tail_flop, tail_bytes;
    unsigned long long pad2[5];
};
static_assert(sizeof(BasePruneCounters) == SSW_BASE_PRUNE_STATS * sizeof(unsigned long long), "the context's block");
static_assert(offsetof(BasePruneCounters, tiles) == 0 && offsetof(BasePruneCounters, col_flop) == 4 * 8 &&
              offsetof(BasePruneCounters, tail_jobs) == 8 * 8 && offsetof(BasePruneCounters, tail_flop) == 9 * 8, "the kernels' sub-blocks");
// What the decide kernel gets.  One lane's buffers: energy [n][W] f32 | need [n][W / 128] u32; `stats` / `work`: the context's
// counters (BasePruneCounters::tiles / ::col_flop on), or null.
struct BasePrune {
    float* energy = nullptr;
    unsigned* need = nullptr;
    unsigned long long* stats = nullptr;
    size_t k = 0;
    int ordering = 0;
    // what the second phase is billed per tile (set by the pass builder): flop and algorithmic bytes of the column launches
    // of one computed tile, bytes the masked selection reads of it; the decide kernel adds them up in `work` [3] (doubles), so
    // that shapes that differ from call to call are each billed at their own rate
    double* work = nullptr;
    double tile_flop = 0.0, tile_bytes = 0.0, select_bytes = 0.0;
};
// G of boundkey(v) = G * E[v]: every key of column v is <= it (rounded up; 0: the ordering has no bound)
float base_prune_gain(size_t w, size_t h, int ordering);
// per frame: T = a lower bound of the k-th key among the coefficients of tile 0 (index 0 excluded), then
// need[frame][t] = any line v of tile t with !(G * E[v] < T); frames with fewer than k keys in tile 0 need every tile
int launch_base_prune_decide(hipStream_t st, const float* coef, const BasePrune& bp, size_t n_frames, size_t w, size_t h);
// diagnostic: boundkey of every frequency column in natural order, out [n][W]
int launch_base_prune_bound(hipStream_t st, const float* energy, size_t n_frames, size_t w, size_t h, int ordering, float* out);

// base_energy.hip: the energies of the tail columns as a rigorous upper bound, from f16 hi + lo products.
// One class of the row pass: its operand planes (k-blocked doubles, `lines` lines), its pre-split bases (base_energy_split),
// pairs and padded sum length, the first tail pair, and the class-major output map of the row launches.
struct BaseEnergyClass {
    const double *x1 = nullptr, *x2 = nullptr;
    const void* y16 = nullptr;
    unsigned NP = 0, Kp = 0, pair0 = 0, pm = 0, c1 = 0, c2 = 0, gsh = 0, e2off = 0;
};
// bytes of a class's pre-split bases: hi | lo halves of both bases in fragment order, then the largest |entry| (one float)
size_t base_energy_split_bytes(unsigned NP, unsigned Kp, unsigned pair0);
int launch_base_energy_split(hipStream_t st, const double* y1, const double* y2, unsigned yrows, unsigned NP, unsigned Kp, unsigned pair0, void* out);
// adds the bounds of pairs pair0 .. NP - 1 of every class into energy [frames][W]; lines_per_frame = 16 * units (padded), of
// which the first `h` are image rows
int launch_base_energy_bound(hipStream_t st, int n_classes, const BaseEnergyClass* cls, size_t n_frames, size_t w, size_t h, size_t lines_per_frame,
                             float factor, float* energy);

// select.hip
struct SelectWorkspace {
    uint32_t* hist = nullptr;       // [n_frames][2048] sample histogram
    uint32_t* ctrl = nullptr;       // [n_frames][4]: threshold digit, candidate count, 2 spare
    uint64_t* cand = nullptr;       // [n_frames][cap] candidate composite keys
    size_t frames = 0, cap = 0;
    uint32_t* fallbacks = nullptr;  // (the context's) counter of frames whose finish ran the exact whole-plane select
};
size_t select_cand_capacity(size_t k);   // candidate slots per frame needed for mark length k
size_t select_max_k();
void select_ortho_scales(size_t w, size_t h, float s[2][2]);      // EnergyOrthogonal / Legacy key scales [first_row][first_column]
// need (optional): per-frame tile mask need[frame][w / need_tile], need_tile = 128 columns -- a tile whose flag is 0 holds
// stale workspace: it is not read and its elements count as +0.0f.  cand_cap (0: ws.cap): a smaller candidate list (tests).
int launch_topk(hipStream_t st, const float* coef, size_t n_frames, size_t w, size_t h, int ordering,
                size_t k, const SelectWorkspace& ws, uint32_t* indices, const unsigned* need = nullptr, unsigned need_tile = 0,
                size_t cand_cap = 0);
// attack.hip: 8-bit boundary + CatmullRom resize (third-party `image` crate semantics)
struct ResizeTaps {                 // host side
    uint32_t max_taps = 0;
    std::vector<uint32_t> left, count;
    std::vector<float> weights;     // [out_len][max_taps]
};
struct DeviceTaps {
    uint32_t* left = nullptr;
    uint32_t* count = nullptr;
    float* weights = nullptr;
    uint32_t max_taps = 0;
    uint32_t span[8] = {0};     // reach in input samples of 1, 2, 4 .. 128 consecutive outputs (host-side, for tiling)
    bool quad_uniform = false;  // every aligned group of 4 outputs shares left and count, count <= 5 (integer up-scaling)
};
void build_resize_taps(size_t in_len, size_t out_len, ResizeTaps& t);
int launch_u8_to_f32(hipStream_t st, const uint8_t* in, size_t n, float* out);
int launch_f32_to_u8(hipStream_t st, const float* in, size_t n, uint8_t* out);
int launch_rgb8_to_yiq(hipStream_t st, const uint8_t* rgb, size_t npix, float* y, float* i, float* q);
int launch_u16_to_f32(hipStream_t st, const uint16_t* in, size_t n, float* out);
int launch_f32_to_u16(hipStream_t st, const float* in, size_t n, uint16_t* out);
int launch_rgb16_to_yiq(hipStream_t st, const uint16_t* rgb, size_t npix, float* y, float* i, float* q);
int launch_yiq_to_rgb8(hipStream_t st, const float* y, const float* i, const float* q, size_t npix, uint8_t* rgb);
size_t resize_tmp_bytes(const uint8_t* in, size_t n_frames, size_t w, size_t h, size_t nw, size_t nh, const DeviceTaps& vt,
                        const DeviceTaps& ht, const uint8_t* out);
int launch_resize_rgb8(hipStream_t st, const uint8_t* in, size_t n_frames, size_t w, size_t h, size_t nw, size_t nh,
                       const DeviceTaps& vt, const DeviceTaps& ht, float* tmp, uint8_t* out);

// sort_full.hip: the first k of all W*H-1 indices of n_frames planes in the reference's order (batched LSD radix
// sort; not hot: only Reader::indices() with a large k and marks longer than the top-k limit reach it)
int full_sort_scratch_bytes(size_t plane_len, size_t n_frames, size_t* bytes);
int launch_full_sort(hipStream_t st, const float* coef, size_t n_frames, size_t w, size_t h, int ordering, void* scratch,
                     size_t scratch_bytes, uint32_t* indices_out, size_t k);
int launch_embed(hipStream_t st, float* coef, size_t n_frames, size_t plane_len,
                 const uint32_t* indices, size_t idx_stride, const float* marks,
                 const uint32_t* mark_offsets, const uint32_t* mark_lens, size_t n_marks,
                 size_t max_len, size_t mark_stride /* between marks when mark_offsets is null */, int method, float alpha);
int launch_extract(hipStream_t st, const float* base, const float* derived, size_t n_frames,
                   size_t plane_len, const uint32_t* indices, size_t k, int method, float alpha,
                   float* out);
int launch_similarity(hipStream_t st, const float* extracted, const float* marks, size_t n_pairs,
                      size_t k, float* sims);
// tracing (ssw_fingerprint_trace): extract with ONE base plane [plane_len] and ONE index list [k] against n_frames derived
// planes / compact planes; the finish of the similarity matrix (argmax, count above the threshold, exact rescoring)
int launch_extract_shared(hipStream_t st, const float* base, const float* derived, size_t n_frames, size_t plane_len,
                          const uint32_t* indices, size_t k, int method, float alpha, float* out);
int launch_extract_shared_pruned(hipStream_t st, const float* base, const float* compact, size_t n_frames, size_t w, size_t h,
                                 size_t cap, const uint32_t* pos, const uint32_t* indices, size_t k, int method, float alpha,
                                 float* out);
int launch_trace_finish(hipStream_t st, const float* sims, size_t n_rows, size_t n_marks, float threshold, const float* extracted,
                        const float* marks, size_t k, uint32_t* best, float* best_sim, uint32_t* n_exceed);
int launch_gemm_nt_f32(hipStream_t st, const float* A, size_t M, const float* B, size_t N, size_t K, float* out);
int launch_sim_den(hipStream_t st, const float* extracted, size_t n_ext, size_t k, float* den);
int launch_sim_scale(hipStream_t st, float* sims, const float* den, size_t n_ext, size_t n_marks);
int launch_widen_indices(hipStream_t st, const uint32_t* in, size_t n, uint64_t* out);

}  // namespace ssw

namespace ssw { namespace host { struct Transfer; } }

// ---- workspace ---------------------------------------------------------------
// Every device buffer a context keeps between calls is a Buf, and every Buf is a member of a group declared from a list
// (SSW_BUF_GROUP): for_each_buf (below the context) visits the groups, so teardown and the pass-size account cannot miss one.
namespace ssw {
struct Buf {       // growable scratch (grow / release: ssw_host.hpp)
    void* p = nullptr;
    size_t bytes = 0;
    template <class T> T* as() const { return static_cast<T*>(p); }
};
namespace host {
int grow(Buf& b, size_t bytes);
template <class T> int grow_as(Buf& b, size_t bytes, T*& out) { SSW_TRY(grow(b, bytes)); out = b.as<T>(); return SSW_OK; }      // grown, and typed
}

#define SSW_BUF_MEMBER(name) Buf name;
#define SSW_BUF_VISIT(name) f(#name, g.name);
#define SSW_BUF_COUNT(name) +1
#define SSW_BUF_GROUP(Group, LIST)                                                                      \
    struct Group {                                                                                      \
        LIST(SSW_BUF_MEMBER)                                                                            \
        static constexpr size_t count = 0 LIST(SSW_BUF_COUNT);                                          \
        template <class G, class F> static void each(G& g, F&& f) { LIST(SSW_BUF_VISIT) }               \
    };                                                                                                  \
    static_assert(sizeof(Group) == Group::count * sizeof(Buf), #Group ": nothing but the Bufs of its list")

// The lane's f32 planes [chunk][H][W], and who puts what into them (the sharing is deliberate: DESIGN §3):
//   slot        batch embed, fingerprint   batch extract, trace, base-prune bound, pruned handle    handles, ssw_dct2d (lane 0)
//   y           Y / coefficients           base coefficients (trace: none, the context's plane)      --
//   i_derived   I                          derived coefficients of an un-pruned chunk                --
//   q_scratch   Q                          the transforms' scratch plane                             --
//   scratch     the transforms' scratch    --                                                        the transform's scratch
#define SSW_LANE_PLANES(X) X(y) X(i_derived) X(q_scratch) X(scratch)
SSW_BUF_GROUP(LanePlanes, SSW_LANE_PLANES);
// The lane's f64 operand slots; one pass at a time uses them, as the views of Lane say (the table is above them).
#define SSW_LANE_OPERANDS(X) X(s_cop) X(odd_t2) X(ss_a1) X(sd) X(even) X(deep)
SSW_BUF_GROUP(LaneOperands, SSW_LANE_OPERANDS);
// pruned derived transform: the row pass's result, the column pass's [chunk][H][cap]
#define SSW_LANE_COMPACT(X) X(rows) X(cols)
SSW_BUF_GROUP(LaneCompact, SSW_LANE_COMPACT);
// The prune tables of one index-list set: u32 = flag [W] | pos [W] | rows [cap] (+ 64); the gathered half bases of the
// frequency classes in launch order and in the fused pass's fragment order.  A lane has one set per chunk (its two orders
// share `gathered`: a chunk takes one row route, `gathered_frag` stays empty), a trace call one for every chunk (ssw_ctx::trace).
#define SSW_PRUNE_BUFS(X) X(u32) X(gathered) X(gathered_frag)
SSW_BUF_GROUP(PruneBufs, SSW_PRUNE_BUFS);
// ssw_fingerprint_trace, what every chunk on both lanes reads: the base plane, its index list, the call's prune tables
// (TraceBufs::prune), the similarity matrix when the caller wants none
#define SSW_TRACE_BUFS(X) X(base_plane) X(base_idx) X(sims)
SSW_BUF_GROUP(TraceBufs, SSW_TRACE_BUFS);
// locate.hip: the original's luma plane | its 16 phase planes | one group's workspace (suspects R, luma, S_f, D; the ladder's
// boxes; the refinement's resized cut-outs) | keys, sums, results | (scale ladder) the original's 8 x 8 box planes | its tap tables
// angle.hip shares luma, phases (the original's one decimated plane) and group (the suspects' planes) and adds: C, S of every
// angle of a call's range | answers, rung and refinement sums, the refinement's slot lists (ssw_rotate_search_attack_rgb8: behind
// them the kept counts, the share-groups and their candidates; its turned frames lie in shared.affine)
// locate_turned.hip shares luma, group (the ladder's boxes and D), keys, box_planes and angle_tab and adds: the suspects' luma
// planes | the full-resolution template planes of one group of the refinement's searches
// locate_free.hip shares luma and taps and adds: the sums of every (suspect, size, position) of a call
#define SSW_LOCATE_BUFS(X) X(luma) X(phases) X(group) X(keys) X(box_planes) X(taps) X(angle_tab) X(angle_sums) X(turned_luma) X(turned_templates) X(free_sums)
SSW_BUF_GROUP(LocateBufs, SSW_LOCATE_BUFS);
// catalogue.hip: the blocks' top-8 lists of a match | host form: one group of frames | its signatures
#define SSW_CATALOGUE_BUFS(X) X(top8) X(frames) X(sigs)
SSW_BUF_GROUP(CatalogueBufs, SSW_CATALOGUE_BUFS);
// fingerprint.hip: line plan (u32) | T64 + gathered basis | Yr64 | mark deltas | dT of a group | handle output
#define SSW_FINGERPRINT_BUFS(X) X(line_plan) X(t64) X(yr64) X(deltas) X(dt) X(out)
SSW_BUF_GROUP(FingerprintBufs, SSW_FINGERPRINT_BUFS);
// The context's single buffers: [chunks] u32 flags of the pruned path (+ class counts) | the base reader's device counters
// (BasePruneCounters) | misc (mark offsets, sims, ...) | full-order sort (lazy, Reader::indices beyond the top-k limit) | f32
// intermediate of the resize's vertical pass | the original's pixels while a restoring trace runs | jpeg.hip: the decoded Y,
// Cb and Cr planes of one group of jobs | filter.hip: the row-blurred planes of one group of jobs | resample.hip: a call's tap
// tables, the row-resampled planes of one group of frames and (scale attack) the thumbnails of one group of jobs | affine.hip:
// the rotated frames of one group of jobs of a rotation attack | crop.hip: the pieces and thumbnails of one group of jobs
#define SSW_SHARED_BUFS(X) X(overflow) X(base_prune_stats) X(small) X(sort_scratch) X(resize_tmp) X(restore_base) X(jpeg) X(filter) X(resample) X(affine) X(crop)
SSW_BUF_GROUP(SharedBufs, SSW_SHARED_BUFS);
}  // namespace ssw

// ---- context ----------------------------------------------------------------
struct ssw_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // where every call enqueues: own_stream, or the caller's (ssw_ctx_set_stream)
    hipStream_t own_stream = nullptr;   // private non-blocking stream created with the context
    size_t chunk_frames = 0;      // frames per internal pass; 0 = automatic (~2^28 pixels)

    // basis cache: (N, inverse, f64, kind) -> device pointer (get_basis; every kind but Dense is f64)
    std::map<std::tuple<size_t, bool, bool, ssw::BasisKind>, void*> basis;
    // (row length, launch class, first tail pair) -> both bases of the class as f16 hi + lo fragments (get_split16, base_energy.hip)
    std::map<std::tuple<size_t, int, unsigned>, void*> split16;
    bool fold = true;             // use the even/odd-folded GEMMs where the shape allows
    int fold_level = SSW_DCT_FOLDING_DEFAULT;           // 1 / 2: dense; 3: operand-ready GEMMs (dct_pair_*.hip, f64 only);
                                  // 4: two levels; 5: + a third on long forward row passes; 6: on all

    using Buf = ssw::Buf;
    // A lane = the workspace of one chunk in flight.  The batch entry points keep two chunks in flight
    // (ssw_ctx_set_overlap): while one lane's basis GEMMs run on the context's stream, the other lane's
    // HBM-bound stages (operand pre-passes, selection, colour conversion) run on `aux_stream`.
    struct Lane {
        ssw::LanePlanes plane;
        ssw::LaneOperands operand;
        Buf idx;                  // [chunk][k] u32
        ssw::SelectWorkspace sel;
        ssw::LaneCompact compact;
        ssw::PruneBufs prune;     // of the chunk's index lists
        Buf base_prune;           // base-reader pruning: energy [chunk][W] f32 | need [chunk][W / 128] u32
        hipStream_t cur = nullptr;   // stream the lane's chain currently runs on
        hipEvent_t done = nullptr;   // recorded right after the lane's latest stage (borrowed from sync_events)

        template <class T> static int grown(Buf& b, size_t bytes, T*& out) { return ssw::host::grow_as(b, bytes, out); }
        // ---- the f32 planes by entry point (the table above LanePlanes); `bytes`: one plane of the chunk
        struct WriterPlanes { float *y, *i, *q, *scratch; };
        int writer_planes(size_t bytes, WriterPlanes& v) {
            SSW_TRY(grown(plane.y, bytes, v.y)); SSW_TRY(grown(plane.i_derived, bytes, v.i)); SSW_TRY(grown(plane.q_scratch, bytes, v.q));
            return grown(plane.scratch, bytes, v.scratch);
        }
        struct ReaderPlanes { float *y, *scratch; };
        int reader_planes(size_t bytes, ReaderPlanes& v) { SSW_TRY(grown(plane.y, bytes, v.y)); return grown(plane.q_scratch, bytes, v.scratch); }
        int reader_scratch(size_t bytes, float** t) { return grown(plane.q_scratch, bytes, *t); }
        int derived_plane(size_t bytes, float** d) { return grown(plane.i_derived, bytes, *d); }
        int handle_scratch(size_t bytes, float** t) { return grown(plane.scratch, bytes, *t); }

        // ---- the operand slots by strategy (dct_plan.hpp): each view grows the slots its pass uses and hands them back
        // by role.  `bytes`: one operand plane of the pass (dct_pair_operand_elems doubles).  A lane runs one pass at a
        // time, so the roles of a slot never overlap -- but a chain is BUILT before it runs, and a slot that a later pass
        // of the same chain grows is captured by the earlier one: grow() retires the old allocation instead of freeing it
        // (ssw_pipeline.hip; found in r5 as a write into freed memory).
        //   slot     one level   two levels   three levels   fused forward               semi-deep / deep inverse        pruned derived
        //   s_cop    S | E       --           S-             16 column-operand planes    --                              o[0]: S-
        //   odd_t2   D | O       D | O        x-             --                          T2 (quarter-length even half)   o[1]: x- | D
        //   ss_a1    --          SS | EE      SSS            --                          A1 (level 2: eighth-length)     o[2]: SS | SSS
        //   sd       --          SD | EO      SS-            --                          --                              o[3]: SD | SS-
        //   even     --          inverse: E   --             --                          E, unrounded                    --
        //   deep     the split odd half (AS BD AD BS) of any split pass; the numbered planes of the deep pre-passes (PairPlanes)
        struct OneLevel { double *s, *d; };
        int one_level(size_t bytes, OneLevel& v) { SSW_TRY(grown(operand.s_cop, bytes, v.s)); return grown(operand.odd_t2, bytes, v.d); }
        struct TwoLevel { double *odd, *ss, *sd, *even; };      // even: grown for an inverse pass only (unrounded E)
        int two_level(size_t bytes, bool inverse, TwoLevel& v) {
            SSW_TRY(grown(operand.odd_t2, bytes, v.odd)); SSW_TRY(grown(operand.ss_a1, bytes, v.ss)); SSW_TRY(grown(operand.sd, bytes, v.sd));
            v.even = operand.even.as<double>();
            return inverse ? grown(operand.even, bytes, v.even) : SSW_OK;
        }
        struct ThreeLevel { double *s_minus, *odd, *r1, *r2; };
        int three_level(size_t bytes, ThreeLevel& v) {
            SSW_TRY(grown(operand.s_cop, bytes, v.s_minus)); SSW_TRY(grown(operand.odd_t2, bytes, v.odd));
            SSW_TRY(grown(operand.ss_a1, bytes, v.r1)); return grown(operand.sd, bytes, v.r2);
        }
        // the fused forward transform's sixteen column-operand planes, `bytes` in all (the row launches write, the column launches read)
        int column_operands(size_t bytes, double** cop) { return grown(operand.s_cop, bytes, *cop); }
        int split_scratch(size_t bytes, double** sp) { return grown(operand.deep, bytes, *sp); }
        // What the dependent launches of an inverse pass exchange, unrounded, `lines` lines of len / 4, len / 2 and (a1: the
        // level-2 deep inverse) len / 8 doubles -- each at least a whole operand plane: the A1 slot is the two-level passes'
        // SS | EE, and a row pass that exchanges A1 is followed, in the same chain, by a column pass that asks for the
        // larger of the two; sized for both at once, the slot does not move between them.
        struct Exchange { double *t2, *even, *a1; };
        int inverse_exchange(size_t bytes, size_t lines, size_t len, bool a1, Exchange& v) {
            const size_t line = lines * sizeof(double);
            SSW_TRY(grown(operand.odd_t2, std::max(bytes, line * (len / 4)), v.t2)); SSW_TRY(grown(operand.even, std::max(bytes, line * (len / 2)), v.even));
            v.a1 = nullptr;
            return a1 ? grown(operand.ss_a1, std::max(bytes, line * (len / 8)), v.a1) : SSW_OK;
        }
        // The pruned derived transform of a chunk: o[PruneClassSrc::lane_buf], the four planes the two- / three-level row
        // pre-passes fill (operand_bytes 0, a deep row pass: none grown -- it writes the numbered planes of `sp` only), both
        // compact planes and the split scratch (split_bytes 0: not split, null).
        struct Pruned { double* o[4]; double* sp; float *rows, *cols; };
        int pruned_derived(size_t operand_bytes, size_t compact_bytes, size_t split_bytes, Pruned& v) {
            Buf* const slot[4] = {&operand.s_cop, &operand.odd_t2, &operand.ss_a1, &operand.sd};
            for (int i = 0; i < 4; ++i) SSW_TRY(operand_bytes ? grown(*slot[i], operand_bytes, v.o[i]) : (v.o[i] = slot[i]->as<double>(), SSW_OK));
            SSW_TRY(grown(compact.rows, compact_bytes, v.rows)); SSW_TRY(grown(compact.cols, compact_bytes, v.cols));
            v.sp = nullptr;
            return split_bytes ? split_scratch(split_bytes, &v.sp) : SSW_OK;
        }
    };
    // (for_each_buf lists a lane's groups and its two single Bufs: a Buf added here must be added there)
    static_assert(sizeof(Lane) == sizeof(ssw::LanePlanes) + sizeof(ssw::LaneOperands) + sizeof(ssw::LaneCompact) + sizeof(ssw::PruneBufs) +
                                  2 * sizeof(Buf) + sizeof(ssw::SelectWorkspace) + sizeof(hipStream_t) + sizeof(hipEvent_t), "the lane's Bufs");
    static constexpr int MAX_LANES = 2;
    Lane lane[MAX_LANES];
    hipStream_t aux_stream = nullptr;     // HBM-bound stages of the batch pipelines
    bool overlap = true;                  // two lanes / two streams in the batch entry points
    bool prune = true;                    // batch extract: derived transform only where the index lists need it
    bool split = true;                    // f64 GEMMs: odd halves as rotated quarter-length cosine + sine pairs
    std::vector<hipEvent_t> sync_events;  // cross-stream dependencies (ring)
    size_t sync_next = 0;
    uint64_t pruned_chunks = 0, redone_chunks = 0;
    uint64_t pruned_columns = 0;          // sum over pruned chunks of the compact plane width (cap_total)
    // base-reader pruning: what flush_timers has already billed of the device counters' doubles (shared.base_prune_stats)
    double base_prune_billed[5] = {0.0, 0.0, 0.0, 0.0, 0.0};     // column flop, bytes, selection bytes | tail row flop, bytes
    // single-image handles (ssw_lib.hip): frames cross PCIe on `copy_stream` into / out of two alternating
    // device staging buffers, so the upload of the next frame runs beside the kernels of the previous one
    hipStream_t copy_stream = nullptr;
    struct FrameStage {
        Buf buf;
        static constexpr int MAX_BANDS = 4;
        hipEvent_t uploaded[MAX_BANDS] = {nullptr, nullptr, nullptr, nullptr};   // copy_stream: band b of the frame (the whole frame: [0]) is in the buffer
        hipEvent_t consumed = nullptr;    // stream: the last kernel that reads (or writes) the buffer is enqueued before
        bool in_use = false;              // `consumed` has been recorded at least once
    };
    FrameStage frame_stage[2];
    unsigned frame_stage_next = 0;
    size_t expected_k = 0;                // mark length of the context's last Reader::extract / indices (speculative selection of the next base reader)
    // device planes of destroyed handles, kept for the next handle of the same size (hipMalloc + hipFree of
    // three 4K planes cost more than the transform); all reuse is ordered on the context's stream
    std::multimap<size_t, void*> plane_pool;
    size_t plane_pool_bytes = 0;
    // RGB staging buffers of derived readers (filled on `copy_stream`, read on `stream`): kept apart with the event that
    // says when their last reader was done, so that the next derived frame's upload waits for THAT and not for everything
    // the context's stream holds (a base reader's transform queued a moment ago)
    struct RgbSpare { void* p; size_t bytes; hipEvent_t released; };
    std::vector<RgbSpare> rgb_spares;
    // workspace buffers that grew while a chain of stages was being built: stages built earlier captured the old pointer, so
    // the old allocation stays valid until the next entry into the library frees it (grow(), CtxGuard; r5)
    std::vector<void*> retired;
    uint32_t* select_fallbacks = nullptr; // device counter: frames whose candidate count fell outside [k, capacity]
    uint64_t select_frames = 0;           // frames selected since the last ssw_ctx_reset_timing
    ssw::host::Transfer* xfer = nullptr;  // pinned staging ring + copy threads (transfer.hip)
    // host-image streaming entry points (ssw_stream.hip): groups of frames cross PCIe on `copy_stream` (up) and
    // `down_stream` into / out of two alternating device buffers while the group between them is being computed
    hipStream_t down_stream = nullptr;
    struct HostStream {
        static constexpr int NB = 3;      // ring depth
        Buf in[NB], in2[NB], out[NB];     // frames of a group: input (base), second input (derived), output
        Buf marks, ext, sims;             // the whole call's marks / extracted marks / similarities
        hipEvent_t up_done[NB] = {}, k_done[NB] = {}, down_done[NB] = {};
        bool active = false;              // a streaming call is running: the ring must stay (dev_malloc's give-back skips it)
    };
    HostStream hs;
    // the per-feature buffers and the context's single ones (the groups above the context)
    struct Trace : ssw::TraceBufs { ssw::PruneBufs prune; } trace;      // prune: the call's tables, what a lane's are to a chunk
    ssw::LocateBufs locate;
    ssw::CatalogueBufs catalogue;
    ssw::FingerprintBufs fingerprint;
    ssw::SharedBufs shared;
    std::map<std::pair<size_t, size_t>, ssw::DeviceTaps> taps;   // (in_len, out_len) -> filter taps

    // timing
    bool timing = false;
    double stage_ms[SSW_STAGE_COUNT] = {0};
    uint64_t stage_launches[SSW_STAGE_COUNT] = {0};
    double stage_bytes[SSW_STAGE_COUNT] = {0};    // algorithmic HBM bytes of every stage (ssw_ctx_get_traffic)
    double stage_work[SSW_STAGE_COUNT] = {0};     // executed flop (GEMM stages) / algorithmic bytes (HBM-bound stages)
    struct Pending {
        int stage;
        hipEvent_t a, b;
        int alias = -1;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    hipEvent_t tail_event = nullptr;      // last event a stage timer recorded; shared with the next timer while tail_fresh
    hipStream_t tail_stream = nullptr;
    bool tail_fresh = false;
};

namespace ssw {
// Every workspace Buf of a context, once: f(lane or ring slot (-1: neither), group, name, buf, counted).  `counted`: the buffer is
// part of what lane_bytes_held adds to the device's free memory for the automatic pass size -- the lanes' planes, operand
// slots, compact planes, index lists and prune tables (gathered bases included), the 44 B/px that a pass is budgeted at.
// Deliberately NOT counted: the lanes' base_prune buffers and selection workspaces (O(chunk * (W + k)), no part of the
// per-pixel budget) and everything the context owns outside the lanes -- counting them would change pass sizes under memory
// pressure.  The selection workspaces are not Bufs (three arrays sized together, select.hip): sel(lane, workspace) gets them.
template <class Ctx, class F, class S> void for_each_workspace(Ctx& c, F&& f, S&& sel) {
    for (int l = 0; l < ssw_ctx::MAX_LANES; ++l) {
        auto& ln = c.lane[l];
        sel(l, ln.sel);
        auto counted = [&](const char* group) { return [&f, l, group](const char* name, auto& b) { f(l, group, name, b, true); }; };
        LanePlanes::each(ln.plane, counted("plane"));
        LaneOperands::each(ln.operand, counted("operand"));
        LaneCompact::each(ln.compact, counted("compact"));
        PruneBufs::each(ln.prune, counted("prune"));
        f(l, "lane", "idx", ln.idx, true);
        f(l, "lane", "base_prune", ln.base_prune, false);
    }
    auto own = [&](const char* group) { return [&f, group](const char* name, auto& b) { f(-1, group, name, b, false); }; };
    TraceBufs::each(c.trace, own("trace"));
    PruneBufs::each(c.trace.prune, own("trace.prune"));
    LocateBufs::each(c.locate, own("locate"));
    CatalogueBufs::each(c.catalogue, own("catalogue"));
    FingerprintBufs::each(c.fingerprint, own("fingerprint"));
    SharedBufs::each(c.shared, own("shared"));
    for (int s = 0; s < ssw_ctx::HostStream::NB; ++s) { f(s, "hs", "in", c.hs.in[s], false); f(s, "hs", "in2", c.hs.in2[s], false); f(s, "hs", "out", c.hs.out[s], false); }
    f(-1, "hs", "marks", c.hs.marks, false); f(-1, "hs", "ext", c.hs.ext, false); f(-1, "hs", "sims", c.hs.sims, false);
    int stage = 0;
    for (auto& fs : c.frame_stage) f(stage++, "frame_stage", "buf", fs.buf, false);
}
template <class Ctx, class F> void for_each_buf(Ctx& c, F&& f) { for_each_workspace(c, f, [](int, const SelectWorkspace&) {}); }
// what the lanes hold of the pass budget (effective_chunk, ssw_pipeline.hip)
inline size_t lane_bytes_held(const ssw_ctx* ctx) {
    size_t held = 0;
    for_each_buf(*ctx, [&](int, const char*, const char*, const Buf& b, bool counted) { if (counted) held += b.bytes; });
    return held;
}
}  // namespace ssw
namespace ssw { inline PlanSettings plan_settings(const ssw_ctx* ctx) { return PlanSettings{ctx->fold, ctx->fold_level, ctx->split}; } }
