// The launch classes of the f64 pair GEMM and the cached bases, by name: ONE table (kPairClasses) says what a class is --
// pairs, sum length, output maps, template instance, class-major slot, operand planes, bases -- and everything else reads it
// (DESIGN §4.0, §4.1).  Host code only, like the planner: pair_class_args() turns a row and the facts of one launch into the
// kernel's per-class arguments.  tests/cpp/pair_class_test.cpp checks the table against ForwardClassLayout and replays a
// recording of every (class, pass, direction, layout, length) tuple.
#pragma once

#include <cstddef>

#include "dct_plan.hpp"

namespace ssw {

// Epilogues.  n = transform length, idx = output index along the transformed axis:
//   EPI_FWD    out[c1 + cs pair] = acc1, out[c2 + cs pair] = acc2          (forward, any folding level)
//   EPI_FWD_ADJ  the same with c1 = 0, c2 = 1, cs = 2 on a row pass: one 8-byte store
//   EPI_INV    out[pair] = acc1 + acc2, out[n-1-pair] = acc1 - acc2        (inverse, one level)
//   EPI_INV_E  T[pair] = acc1 + acc2, T[n/2-1-pair] = acc1 - acc2, unrounded (inverse level 2: the even half E)
//   EPI_INV_O  with n1 = pair, n2 = pair + n/4:  out[n1] = T[n1] + acc1, out[n-1-n1] = T[n1] - acc1,
//              out[n2] = T[n2] + acc2, out[n-1-n2] = T[n2] - acc2          (inverse level 2: odd part + combine)
//   EPI_INV_O_RGB  EPI_INV_O on the last pass of Writer::result (a column pass): instead of storing the Y sample it
//              converts (Y, I, Q) of that pixel to RGB like From<&YIQ32FImage> for Rgb32FImage (src/yiq.rs:187-197:
//              (y + m1 i) + m2 q per channel, clamped to [0, 1]) and stores the interleaved pixel -- f32, or
//              8-bit like into_rgb8() (round(clamp * 255)).  The colour conversion's HBM traffic (I, Q in, RGB out)
//              then runs in the shadow of the other resident block's MFMAs and the Y plane is never written.
//   EPI_INV_OT EPI_INV_O one level down (deep inverse): the odd part of the half-length transform E combined with ITS even
//              half T2 (`tmp`, length n/2 per line) into E itself, unrounded: T[n1] = T2[n1] + acc, T[n-1-n1] = T2[n1] - acc
//              (`tmp_out`, length n per line; n = the half-length transform's length)
//   EPI_FWD_COLOP (forward ROW pass of a rows-first transform whose two passes run at level 2): EPI_FWD's values --
//              rounded to f32 like the store between the passes (src/dct2d.rs:152-168), then the f32 per-index factor --
//              are not stored: the operand lines are ordered (frame, unit of the column fold, line of the unit), a 16-line
//              MFMA tile holds the sixteen rows of one unit, and the epilogue applies the column pre-pass's arithmetic
//              (dct_pair_colops.hpp: col_l2_unit) to them and stores the sixteen k-blocked COLUMN operand planes directly.
//              No f32 plane between the passes, no column pre-pass: 16 B/px of HBM traffic less per forward transform.
enum { EPI_FWD = 0, EPI_FWD_ADJ = 1, EPI_INV = 2, EPI_INV_E = 3, EPI_INV_O = 4, EPI_INV_O_RGB = 5, EPI_INV_OT = 6, EPI_FWD_COLOP = 7 };

// The bases the context caches per (length, direction): the dense N x N basis (f32 or f64); f64 only: the even / odd half basis
// (N/2 x N/2, k-blocked), the quarter-length cosine / sine bases of the split odd half (classes E and O), the rotation
// table, and sinE as the launches read it (row 0 = row N/8: class E's first and last pair share a slot).
enum class BasisKind : int { Dense, HalfEven, HalfOdd, CosE, SinE, CosO, SinO, Rot, SinELaunch };

// What the kernel gets per class (PairMulti, dct_pair_f64_kernel.hpp) ...
struct PairClassArgs {
    const double *x1, *x2, *y1, *y2;
    unsigned NP, Kp, yrows, tiles_n;
    unsigned c1, c2, cs, pm, np1, p2lo, bn32, fold0;
    unsigned gsh, e2off;               // forward class-major output map (PairOut::ft)
    unsigned tn0 = 0;                  // first tile column of the launch (the gated tail launches of a pruned base reader: 1)
};
// ... and what selects the template instance of a class: all classes of a launch must agree
struct PairInstance {
    int epi; bool samex; int subname;
    bool operator==(const PairInstance& o) const { return epi == o.epi && samex == o.samex && subname == o.subname; }
};

// The launch classes.  A transform of length n folds into the even half (a transform of n/2: it folds again) and the odd
// half, which either runs whole against the two row blocks of the odd half basis (one shared operand) or is split: rotated
// into classes E (AS x cosE, BD x sinE) and O (AD x cosO, BS x sinO) of n/8 pairs.  Level 2 folds / rotates those once more.
// The names are those of ForwardClassLayout and DESIGN §3; a digit = the class of the half- (2) / quarter-length (4) transform.
enum class PairClass : int {
    OneLevel,                  // one folding level: S x even, D x odd half basis
    EvenHalf, OddHalf,         // two levels: (SS, SD) x the half bases of n/2 | D shared x the odd half basis
    R1R2, OddHalf2,            // the half-length transform's: c[8q] | c[8q+4], and S- shared (2 mod 4)
    R1A, OddHalf4,             // the quarter-length transform's: R1+ R1- (level 2: 16i | 16i + 8)
    E, O,                      // the split odd half: AS BD | AD BS
    E2, O2,                    // ... of the half-length transform: AS2 BD2 | AD2 BS2
    E4, O4,                    // ... of the quarter-length transform (no strategy launches OddHalf4, E4, O4)
    EE, EO,                    // level 2, class E folded once more: AS+ BD- | AS- BD+
    O5, O3,                    // level 2, class O rotated once more: O rotated "+" | O rotated "-"
    R2A,                       // level 2: R2 rotated
    Count
};

struct PairMap { unsigned cs; int r1, r2; };      // pair p -> r1 + cs p (first output) | r2 + cs p (second)
struct PairClassRow {
    const char* name;
    unsigned ldiv;             // the class belongs to the transform of length leff = n / ldiv that the folding applies to the even part
                               // (level 2: the length of its bases)
    unsigned np_div, k_div;    // pairs = leff / np_div, sum length = leff / k_div
    bool split;                // two different operands against a cosine and a sine basis, outputs acc1 +/- acc2 (pm)
    bool eshape;               // class E's shape: leff/8 + 1 pairs in leff/8 slots (fold0), sine basis = its launch variant
    bool samex;                // one shared operand; the second product reads the basis's second row block, its outputs `pairs` further on
    PairMap fwd;               // frequencies of the full transform (mod cs: the residues ForwardClassLayout::res())
    PairMap inv;               // positions of the transform it serves
    unsigned inv_ndiv;         // ... which has length n / inv_ndiv (0: no inverse launch of this class)
    int inv_epi;               // EPI_INV, EPI_INV_E, or EPI_INV_O = an odd part (EPI_INV_O_RGB with a sink, EPI_INV_OT one level down)
    int sub_col, sub_row;      // SUB of the template instance on a forward column / row pass (inverse: 0, or 1 one level down)
    int slot1, slot2;          // ForwardClassLayout class of the first output at level 1 / level 2 (-1: not class-major)
    bool class_major;          // may write (forward: its slot) / exchange (inverse) the class-major plane
    signed char l1x[2], l2x[2];   // operand planes of the deep pre-passes, by number (level 1: 0..5 K8 wide, 6..9 K16 wide)
    BasisKind y1, y2;          // the cached bases it reads ...
    unsigned ydiv;             // ... of length n / ydiv
};
constexpr int kNo = -1;
inline constexpr PairClassRow kPairClasses[(int)PairClass::Count] = {
    //  name            ldiv np k  split eshape samex  fwd            inv          ndiv epi       col row  slot1 slot2 cm     l1x       l2x        y1                   y2                     ydiv
    {"one level",        1, 2, 2, false, false, false, {2, 0, 1},    {2, 0, 1},    1, EPI_INV,   0, 0,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::HalfEven, BasisKind::HalfOdd,    1},
    {"even half",        1, 4, 4, false, false, false, {4, 0, 2},    {4, 0, 2},    1, EPI_INV_E, 0, 0,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::HalfEven, BasisKind::HalfOdd,    2},
    {"odd half",         1, 4, 2, false, false, true,  {2, 1, 1},    {1, 0, 0},    1, EPI_INV_O, 0, 0,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::HalfOdd,  BasisKind::HalfOdd,    1},
    {"R1 R2",            2, 4, 4, false, false, false, {8, 0, 4},    {8, 0, 4},    2, EPI_INV_E, 1, 1,  0,   kNo, true,  {4, 5},   {-1, -1}, BasisKind::HalfEven, BasisKind::HalfOdd,    4},
    {"odd half of n/2",  2, 4, 2, false, false, true,  {4, 2, 2},    {1, 0, 0},    2, EPI_INV_O, 1, 1,  kNo, kNo, false, {6, 6},   {-1, -1}, BasisKind::HalfOdd,  BasisKind::HalfOdd,    2},
    {"R1+ R1-",          4, 4, 4, false, false, false, {16, 0, 8},   {16, 0, 8},   4, EPI_INV_E, 1, 1,  kNo, 0,   true,  {-1, -1}, {8, 9},   BasisKind::HalfEven, BasisKind::HalfOdd,    8},
    {"odd half of n/4",  4, 4, 2, false, false, true,  {8, 4, 4},    {1, 0, 0},    0, EPI_INV_O, 1, 1,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::HalfOdd,  BasisKind::HalfOdd,    4},
    {"AS BD",            1, 8, 8, true,  true,  false, {8, 1, -1},   {4, 0, -1},   1, EPI_INV_O, 3, 3,  6,   kNo, true,  {0, 1},   {-1, -1}, BasisKind::CosE,     BasisKind::SinELaunch, 1},
    {"AD BS",            1, 8, 8, true,  false, false, {8, 5, 3},    {4, 2, 1},    1, EPI_INV_O, 3, 4,  8,   kNo, true,  {2, 3},   {-1, -1}, BasisKind::CosO,     BasisKind::SinO,       1},
    {"AS2 BD2",          2, 8, 8, true,  true,  false, {16, 2, -2},  {4, 0, -1},   2, EPI_INV_O, 3, 3,  2,   4,   true,  {6, 7},   {12, 13}, BasisKind::CosE,     BasisKind::SinELaunch, 2},
    {"AD2 BS2",          2, 8, 8, true,  false, false, {16, 10, 6},  {4, 2, 1},    2, EPI_INV_O, 3, 3,  4,   6,   true,  {8, 9},   {14, 15}, BasisKind::CosO,     BasisKind::SinO,       2},
    {"AS4 BD4",          4, 8, 8, true,  true,  false, {32, 4, -4},  {4, 0, -1},   0, EPI_INV_O, 3, 3,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::CosE,     BasisKind::SinELaunch, 4},
    {"AD4 BS4",          4, 8, 8, true,  false, false, {32, 20, 12}, {4, 2, 1},    0, EPI_INV_O, 3, 3,  kNo, kNo, false, {-1, -1}, {-1, -1}, BasisKind::CosO,     BasisKind::SinO,       4},
    {"AS+ BD-",          2, 8, 8, true,  true,  false, {16, 1, -1},  {8, 0, -1},   1, EPI_INV_O, 3, 3,  kNo, 8,   true,  {-1, -1}, {0, 3},   BasisKind::CosE,     BasisKind::SinELaunch, 2},
    {"AS- BD+",          2, 8, 8, true,  false, false, {16, 9, 7},   {8, 4, 3},    1, EPI_INV_O, 3, 3,  kNo, 10,  true,  {-1, -1}, {1, 2},   BasisKind::CosO,     BasisKind::SinO,       2},
    {"O rotated \"+\"",  2, 8, 8, true,  true,  false, {16, 5, -5},  {8, 2, -3},   1, EPI_INV_O, 3, 4,  kNo, 12,  true,  {-1, -1}, {4, 5},   BasisKind::CosE,     BasisKind::SinELaunch, 2},
    {"O rotated \"-\"",  2, 8, 8, true,  true,  false, {16, 3, -3},  {8, 1, -2},   1, EPI_INV_O, 3, 3,  kNo, 14,  true,  {-1, -1}, {6, 7},   BasisKind::CosE,     BasisKind::SinELaunch, 2},
    {"R2 rotated",       2, 8, 8, true,  true,  false, {16, 4, -4},  {2, 0, -1},   4, EPI_INV_O, 3, 3,  kNo, 2,   true,  {-1, -1}, {10, 11}, BasisKind::CosE,     BasisKind::SinELaunch, 2},
};
constexpr const PairClassRow& pair_class_row(PairClass c) { return kPairClasses[(int)c]; }

// the eight classes of a level-2 pass in the order the forward launches run; the inverse runs them as R1+ R1- -> A1,
// R2 rotated + A1 -> T2, AS2 BD2 | AD2 BS2 + T2 -> E, then the odd part + E -> x
inline constexpr PairClass kLevel2Classes[8] = {PairClass::R1A, PairClass::R2A, PairClass::E2, PairClass::O2,
                                         PairClass::EE, PairClass::EO, PairClass::O3, PairClass::O5};

// The per-class arguments and the template instance of one launch of class `c` over lines of length `len`: the row, plus what
// belongs to the launch -- the pass, the direction, the layout of the plane (gsh from its tile), a sink, `tmp_out`, and
// whether 48-pair tiles are on (`tile48`).  SSW_ERR_BAD_ARG where the row does not serve that direction or layout.  The four
// pointers of `ca` are the caller's.
int pair_class_args(PairClass c, bool is_row, bool inverse, size_t len, const PairLayout& lay, bool with_sink, bool has_tmp_out, bool tile48,
                    PairClassArgs& ca, PairInstance& inst);
// executed flop of one launch of class `c`: two products of lines x pairs x sum length multiply-adds
double pair_class_flop(PairClass c, size_t lines, size_t len);

// The low-precision tail bound of a pruned base reader's row pass (base_energy.hip): whether a class's launch can be cut into
// tile column 0 (the head) and gated tail launches whose energies the bound kernel covers ...
bool base_tail_class_ok(const PairClassArgs& ca);
// ... and the same for the level-2 row pass over lines of length `len` (kLevel2Classes, in their order): eligible when every
// class is and all agree on the first tail pair and the pair count; then the numbers the bound kernel takes per class
// (BaseEnergyClass) and its chunks of 11 MFMA pair tiles.  Not eligible: every number is 0.  No device pointer in here.
struct BaseTailPlan {
    bool eligible = false;
    unsigned pair0 = 0, NP = 0, chunks = 0;
    struct Class { unsigned Kp = 0, yrows = 0, pm = 0, c1 = 0, c2 = 0, gsh = 0, e2off = 0; } cls[8];
};
int base_tail_plan(size_t len, const PairLayout& layout, bool tile48, BaseTailPlan& plan);

// The pruned derived row pass (prune.hip): the classes a row plan launches, in the plan's order, and their rows of the
// PrunePlan for `cap` gathered columns -- each class's forward frequency map as (mod, rem, rem2, radd).
struct PrunePlan;
int prune_class_list(const PassPlan& rows, PairClass out[8]);
void prune_plan_classes(const PairClass* cls, int n, unsigned cap, PrunePlan& plan);
// What the subset product of each class OF THE PLAN reads (prune_plan_classes' order: a split launch class is one class of the
// plan -- cosine and sine rows --, a folded one two), over lines of length w.  Returns the number of plan classes; 0 where
// the table does not serve a class at that length.
struct PruneClassSrc {
    signed char p1, p2;        // operand plane(s) by number at the plan's level (l1x / l2x); p2: the sine operand of a split class, else -1
    signed char lane_buf;      // a class that is neither deep nor split reads plane lane_buf of the pruned chunk's four (Lane::Pruned::o,
                               // ssw_internal.hpp) as the two- / three-level pre-passes fill them: 0 S-, 1 x- | D, 2 3 SS SD | SSS SS-;
                               // -1: the numbered plane
    bool split;
    BasisKind y1, y2;          // the bases as cached (the gather reads sinE itself, not its launch variant); y2: split only
    unsigned ydiv, src_rows, Kp, ktrue;      // bases of length w / ydiv with src_rows lines; padded / true sum length
    size_t goff = 0, goff2 = 0;              // prune_gathered_offsets: where its gathered bases lie (goff2: a split class's sine basis)
};
int prune_class_sources(const PairClass* cls, int n, const PassPlan& rows, size_t w, PruneClassSrc out[9]);
// sets the byte offsets of the classes' gathered bases in one buffer, [Kp][cap in whole tiles of 16 rows] doubles each (the
// fused pass's fragment order needs whole tiles), and returns the buffer's size
size_t prune_gathered_offsets(const PrunePlan& plan, PruneClassSrc* src);

}  // namespace ssw
