// The launch-class table's readers (dct_pair_class.hpp).  Host code only.
#include "ssw_internal.hpp"
#include "dct_pair_common.hpp"

namespace ssw {

// the table names its class-major slots by number: they are ForwardClassLayout's
typedef ForwardClassLayout F;
static_assert(pair_class_row(PairClass::R1R2).slot1 == F::R1 && pair_class_row(PairClass::E).slot1 == F::EP && pair_class_row(PairClass::O).slot1 == F::OP &&
              pair_class_row(PairClass::E2).slot1 == F::E2P && pair_class_row(PairClass::O2).slot1 == F::O2P, "level-1 slots");
static_assert(pair_class_row(PairClass::R1A).slot2 == F::R1A && pair_class_row(PairClass::R2A).slot2 == F::R2A && pair_class_row(PairClass::E2).slot2 == F::F_E2P &&
              pair_class_row(PairClass::O2).slot2 == F::F_O2P && pair_class_row(PairClass::EE).slot2 == F::EEP && pair_class_row(PairClass::EO).slot2 == F::EOP &&
              pair_class_row(PairClass::O5).slot2 == F::O5 && pair_class_row(PairClass::O3).slot2 == F::O3, "level-2 slots");

int pair_class_args(PairClass c, bool is_row, bool inverse, size_t len, const PairLayout& lay, bool with_sink, bool has_tmp_out, bool tile48,
                    PairClassArgs& ca, PairInstance& inst) {
    if ((int)c < 0 || c >= PairClass::Count) return SSW_ERR_BAD_ARG;
    const PairClassRow& r = pair_class_row(c);
    if (inverse && r.inv_ndiv == 0) return SSW_ERR_BAD_ARG;
    const bool odd_part = r.inv_epi == EPI_INV_O, down = r.inv_ndiv > 1;      // down: serves the half- / quarter-length transform
    if (inverse && down && odd_part && !has_tmp_out) return SSW_ERR_BAD_ARG;          // the odd part of E needs somewhere to put E
    const size_t leff = len / r.ldiv;
    if (r.split && leff % 8 != 0) return SSW_ERR_BAD_ARG;
    ca.NP = (unsigned)(leff / r.np_div);
    ca.Kp = (unsigned)dct_pair_kpad(leff / (r.k_div / 2));
    ca.yrows = r.samex ? 2 * ca.NP : r.eshape ? ca.NP + 1 : ca.NP;      // lines of the basis plane(s): class E's keep row leff/8
    ca.fold0 = r.eshape ? ca.NP : 0;                                    // ... whose sine basis is the launch variant (row 0 = row leff/8)
#ifdef SSW_ABL_NP128        // timing-only ablation: the 135-pair column classes without their 7-pair tail tile
    if (!is_row && ca.NP == 135) ca.NP = 128;
#endif
    ca.tiles_n = (ca.NP + 63) / 64;
    ca.np1 = 0xFFFFFFFFu; ca.p2lo = 0; ca.bn32 = 0;
    // 48-pair tiles where 64-pair ones would end in a tile of at most 16 pairs and 48 need no more tiles (135 = 48 + 48 + 39
    // instead of 64 + 64 + 7: 4K and 1080p columns)
    if (tile48 && ca.NP > 64 && (ca.NP % 64) != 0 && (ca.NP % 64) <= 16 && (ca.NP + 47) / 48 == ca.tiles_n) {
        ca.bn32 = 2;
        ca.tiles_n = (ca.NP + 47) / 48;
    }
    // the output map: frequencies (forward) or positions (inverse); a shared operand's second outputs lie `pairs` entries on
    const PairMap& m = inverse ? r.inv : r.fwd;
    ca.cs = m.cs; ca.c1 = (unsigned)m.r1; ca.c2 = (unsigned)m.r2 + (r.samex ? m.cs * ca.NP : 0u);
    ca.pm = r.split ? 1 : 0;
    ca.gsh = 31; ca.e2off = 0;
    if (lay.class_major) {
        // forward row pass of a deep transform: every class writes its frequencies side by side (ForwardClassLayout) instead
        // of 4-byte pieces 16 / 32 bytes apart -- the column pre-pass puts the columns back; inverse: the split classes write
        // (and read E) at one pair of residues mod 4 (po.cm, inverse_class_pos), the even halves keep the natural order
        if (!is_row || !r.class_major) return SSW_ERR_BAD_ARG;
        if (!inverse) {
            // po.ft = the tile: entry e of a class -> column base + (e >> gsh) * ft + (e & (2^gsh - 1)); class E's second
            // output of pair p is entry p - 1 of its "-" class (frequency 8 p - 1)
            const F fl{(unsigned)len, lay.tile, lay.rows_l2};
            const int k1 = lay.rows_l2 ? r.slot2 : r.slot1;
            if (k1 < 0) return SSW_ERR_BAD_ARG;
            ca.cs = 1;
            ca.c1 = fl.base(k1); ca.c2 = fl.base(k1 + 1);
            ca.e2off = r.eshape ? 1u : 0u;
            if (fl.t != fl.n) {
                const unsigned g = fl.group(k1);
                if (g == 0 || (g & (g - 1)) != 0) return SSW_ERR_BAD_ARG;
                ca.gsh = 0;
                while ((1u << ca.gsh) < g) ++ca.gsh;
            }
        }
    }
    if (!inverse) inst = {c == PairClass::OneLevel && is_row ? EPI_FWD_ADJ : EPI_FWD, r.samex, is_row ? r.sub_row : r.sub_col};
    else if (!odd_part) inst = {r.inv_epi, false, down ? 1 : 0};
    else if (with_sink) inst = {EPI_INV_O_RGB, r.samex, 0};
    else inst = {down ? EPI_INV_OT : EPI_INV_O, r.samex, down ? 1 : 0};
    return SSW_OK;
}

double pair_class_flop(PairClass c, size_t lines, size_t len) {
    const PairClassRow& r = pair_class_row(c);
    const size_t leff = len / r.ldiv;
    return 4.0 * (double)lines * (double)(leff / r.np_div) * (double)(leff / r.k_div);
}

// More than one tile column, of 64 or 48 pairs (not the 32-pair tiles of a small launch), in the class-major output map.
// (sums of more than 256 terms stay exact: the accumulation term of the bound grows with the sum length times the line's norm,
// and at 8K -- 480 terms -- it passed the threshold on every tail tile of the 8K benchmark frames)
// (the bound kernel adds a term for both outputs of every tail pair: that is the exact epilogue's set of outputs only while
// every pair has both -- np1 = none, p2lo = 0 -- and a class is plain or split, pm 0 / 1)
bool base_tail_class_ok(const PairClassArgs& ca) {
    return ca.tiles_n >= 2 && ca.Kp <= 256 && ca.gsh <= 16 && ca.bn32 != 1 && ca.np1 == 0xFFFFFFFFu && ca.p2lo == 0 && ca.pm <= 1;
}

int base_tail_plan(size_t len, const PairLayout& layout, bool tile48, BaseTailPlan& plan) {
    plan = BaseTailPlan();
    unsigned pair0 = 0, np = 0;
    for (int c = 0; c < 8; ++c) {
        PairClassArgs ca;
        PairInstance inst;
        SSW_TRY(pair_class_args(kLevel2Classes[c], true, false, len, layout, false, false, tile48, ca, inst));
        const unsigned p0 = ca.bn32 == 2 ? 48u : 64u;              // the head: tile column 0
        if (!base_tail_class_ok(ca) || (c > 0 && (p0 != pair0 || ca.NP != np))) { plan = BaseTailPlan(); return SSW_OK; }
        pair0 = p0; np = ca.NP;
        plan.cls[c] = {ca.Kp, ca.yrows, ca.pm, ca.c1, ca.c2, ca.gsh, ca.e2off};
    }
    plan.eligible = true;
    plan.pair0 = pair0; plan.NP = np;
    plan.chunks = ((np - pair0 + 15) / 16 + 10) / 11;
    return SSW_OK;
}

int prune_class_list(const PassPlan& rows, PairClass out[8]) {
    typedef PairClass C;
    int n = 0;
    if (plan_is_level2(rows)) {
        for (C c : {C::EE, C::EO, C::O5, C::O3, C::E2, C::O2, C::R2A, C::R1A}) out[n++] = c;
        return n;
    }
    if (rows.split) { out[n++] = C::E; out[n++] = C::O; }
    else out[n++] = C::OddHalf;
    if (plan_is_deep(rows)) { out[n++] = C::E2; out[n++] = C::O2; out[n++] = C::R1R2; }
    else if (rows.levels == 3) { out[n++] = C::OddHalf2; out[n++] = C::R1R2; }
    else out[n++] = C::EvenHalf;
    return n;
}

// frequency v is in the class when v % mod == rem or == rem2; basis row (v + radd) / mod.  A split class gathers both its
// residues into one set of rows (v = mod i +/- r -> row i of a class of E's shape); the two outputs of a folded class read
// different bases: one class each; a shared operand's outputs have one residue.
void prune_plan_classes(const PairClass* cls, int n, unsigned cap, PrunePlan& plan) {
    unsigned nc = 0, off = 0;
    auto add = [&](unsigned mod, unsigned rem, unsigned cc, unsigned rem2 = PRUNE_NO_REM, unsigned radd = 0) {
        plan.c[nc] = {mod, rem, cc, off, rem2, radd};
        off += cc;
        ++nc;
    };
    for (int i = 0; i < n; ++i) {
        const PairClassRow& r = pair_class_row(cls[i]);
        const unsigned mod = r.fwd.cs, r1 = (unsigned)r.fwd.r1 % mod, r2 = (unsigned)(r.fwd.r2 + (int)mod) % mod;
        if (r.split) add(mod, r1, 2 * cap / mod, r2, r.eshape ? r1 : 0);
        else if (r.samex) add(mod, r1, cap / mod);
        else { add(mod, r1, cap / mod); add(mod, r2, cap / mod); }
    }
    plan.n_classes = nc;
}

int prune_class_sources(const PairClass* cls, int n, const PassPlan& rows, size_t w, PruneClassSrc out[9]) {
    const bool deep = plan_is_deep(rows), level2 = plan_is_level2(rows);
    int nc = 0;
    for (int i = 0; i < n; ++i) {
        const PairClassRow& r = pair_class_row(cls[i]);
        PairClassArgs ca;
        PairInstance inst;
        if (pair_class_args(cls[i], true, false, w, PairLayout(), false, false, false, ca, inst) != SSW_OK) return 0;
        const signed char* pn = level2 ? r.l2x : r.l1x;
        const bool numbered = deep || r.split;
        const BasisKind y2 = r.y2 == BasisKind::SinELaunch ? BasisKind::SinE : r.y2;
        const unsigned ktrue = (unsigned)(w / r.ldiv / r.k_div);
        auto add = [&](int j, BasisKind y) {
            const int buf = numbered ? -1 : r.samex ? (cls[i] == PairClass::OddHalf ? 1 : 0) : 2 + j;
            PruneClassSrc& s = out[nc++] = PruneClassSrc();
            s.p1 = pn[j]; s.p2 = (signed char)(r.split ? pn[1] : -1); s.lane_buf = (signed char)buf; s.split = r.split;
            s.y1 = y; s.y2 = r.split ? y2 : y;
            s.ydiv = r.ydiv; s.src_rows = ca.yrows; s.Kp = ca.Kp; s.ktrue = ktrue;
        };
        add(0, r.y1);
        if (!r.split && !r.samex) add(1, y2);
    }
    return nc;
}

size_t prune_gathered_offsets(const PrunePlan& plan, PruneClassSrc* src) {
    size_t total = 0;
    for (unsigned c = 0; c < plan.n_classes; ++c) {
        const size_t bytes = (size_t)src[c].Kp * ((plan.c[c].cap + 15) / 16 * 16) * sizeof(double);
        src[c].goff = total; total += bytes;
        src[c].goff2 = total; if (src[c].split) total += bytes;
    }
    return total;
}

}  // namespace ssw
