// The rotation + fold of the split odd half (dct_pair_prep.hip, "Split odd half") and the operand planes of a deep
// pass: shared by the pre-pass kernels of dct_pair_prep.hip and dct_pair_prep_staged.hip.
#pragma once
#include <type_traits>

#include "dct_pair_common.hpp"

namespace ssw {

// the same for a single e (scalar kernels)
__device__ inline void split_one(double d0, double d1, double d2, double d3, const double* __restrict__ rot, unsigned e, unsigned Mh, double& as, double& bd, double& ad, double& bs) {
    const double cc = rot[e], ss = rot[Mh + e], ccm = rot[Mh - 1 - e], ssm = rot[2 * Mh - 1 - e];
    const double a = d0 * cc + d3 * ss, b = d3 * cc - d0 * ss;
    const double am = d1 * ccm + d2 * ssm, bm = d2 * ccm - d1 * ssm;
    as = a + am;
    ad = a - am;
    bs = b + bm;
    bd = b - bm;
}
// One unit of the split: four consecutive e = base .. base + 3 of a DCT-IV input d of length M (Mh = M/2) given as
// ascending quads  dA: d[base + i], dB: d[Mh-4-base + i], dC: d[Mh+base + i], dD: d[M-4-base + i];
// rot: [0, Mh) cos psi, [Mh, 2 Mh) sin psi.  Same operations in the same order as pair_rotate_kernel.
__device__ inline void split_unit(const f64x4& dA, const f64x4& dB, const f64x4& dC, const f64x4& dD,
                                  const double* __restrict__ rot, unsigned base, unsigned Mh,
                                  f64x4& as, f64x4& bd, f64x4& ad, f64x4& bs) {
    const f64x4 c = *reinterpret_cast<const f64x4*>(rot + base), s = *reinterpret_cast<const f64x4*>(rot + Mh + base);
    const f64x4 cm = *reinterpret_cast<const f64x4*>(rot + Mh - 4 - base), sm = *reinterpret_cast<const f64x4*>(rot + 2 * Mh - 4 - base);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double d0 = dA[i], d1 = dB[3 - i], d2 = dC[i], d3 = dD[3 - i];
        const double cc = c[i], ss = s[i], ccm = cm[3 - i], ssm = sm[3 - i];
        const double a = d0 * cc + d3 * ss, b = d3 * cc - d0 * ss;
        const double am = d1 * ccm + d2 * ssm, bm = d2 * ccm - d1 * ssm;
        as[i] = a + am;
        ad[i] = a - am;
        bs[i] = b + bm;
        bd[i] = b - bm;
    }
}

struct DeepPlanes {        // device pointers of one pass's operand planes
    void *as, *bd, *ad, *bs;         // K8 wide
    void *r1, *r2;                   // K8 wide
    void *as2, *bd2, *ad2, *bs2;     // K16 wide
    // forward ROW passes at level 2 (r4b, PassStrategy::DeepL2): twelve planes K16 wide replace the six K8 wide ones --
    //   asp asm_ bdp bdm   class E folded once more: AS +/- its mirror, BD +/- its mirror (exact)
    //   oap obp oam obm    class O (a DCT-IV of AD and a DST-IV of BS, length n/8) rotated once more: (a, b) of AD plus /
    //                      minus (a, b) of the reversed BS
    //   r1p r1m            R1 +/- its mirror (exact)
    //   r2a r2b            R2 (a DCT-IV input of length n/8) rotated: (a, b)
    void *asp = nullptr, *asm_ = nullptr, *bdp = nullptr, *bdm = nullptr;
    void *oap = nullptr, *obp = nullptr, *oam = nullptr, *obm = nullptr;
    void *r1p = nullptr, *r1m = nullptr, *r2a = nullptr, *r2b = nullptr;
};
// the planes in their order from `base`: AS BD AD BS R1 R2 (lines * K8 each), then AS2 BD2 AD2 BS2 (lines * K16 each)
inline DeepPlanes planes_of(double* base, size_t lines, size_t K8, size_t K16) {
    DeepPlanes dp;
    const size_t p8 = lines * K8, p16 = lines * K16;
    double* q = base + 6 * p8;
    dp.as = base; dp.bd = base + p8; dp.ad = base + 2 * p8; dp.bs = base + 3 * p8; dp.r1 = base + 4 * p8; dp.r2 = base + 5 * p8;
    dp.as2 = q; dp.bd2 = q + p16; dp.ad2 = q + 2 * p16; dp.bs2 = q + 3 * p16;
    return dp;
}

// The run-time source of a row pre-pass as compile-time constants: launch(std::integral_constant<RowSrc, ..>, std::bool_constant<with
// I/Q>) for the kernel instance that reads `in` -- the one place the source x I/Q cross product is spelled out.  An f32 plane has
// no I and Q: SSW_ERR_BAD_ARG, and no such instance exists.
template <class Launch>
int dispatch_row_src(const RowInput& in, Launch&& launch) {
    const bool iq = in.i && in.q;
    auto rgb = [&](auto src) {
        if (iq) launch(src, std::true_type{}); else launch(src, std::false_type{});
        return SSW_OK;
    };
    switch (in.kind) {
        case RowSrc::Plane:
            if (iq) return SSW_ERR_BAD_ARG;
            launch(std::integral_constant<RowSrc, RowSrc::Plane>{}, std::false_type{});
            return SSW_OK;
        case RowSrc::RgbF32: return rgb(std::integral_constant<RowSrc, RowSrc::RgbF32>{});
        case RowSrc::RgbU8:  return rgb(std::integral_constant<RowSrc, RowSrc::RgbU8>{});
        case RowSrc::RgbU16: return rgb(std::integral_constant<RowSrc, RowSrc::RgbU16>{});
    }
    return SSW_ERR_BAD_ARG;
}

// dct_pair_prep_light.hip: the level-2 row pre-pass in the form that fits beside the GEMMs
bool dct_pair_prep_light_ok(size_t w, size_t lines);          // of a row pass at level 2
int launch_dct_pair_prep16_rows_light(hipStream_t st, const RowInput& in, const DeepPlanes& dp, const double* rot1, const double* rot2,
                                      const double* rot3, size_t rows, size_t w, unsigned K16, unsigned unit_h, unsigned unit_hup);
// dct_pair_derived.hip: the derived frame's pruned row pass in one kernel (marks of up to 1024 entries)
struct DerivedFusedClass {
    const double *y1, *y2;     // gathered bases (y2: the sine part of a split class)
    unsigned p1, p2;           // operand planes by number
    unsigned cap, off;         // gathered rows = compact columns off .. off + cap - 1
    bool split;
};
bool dct_pair_derived_fused_fits(unsigned n_classes, const DerivedFusedClass* cls);
int launch_dct_pair_derived_fused(hipStream_t st, const RowInput& in, size_t lines, size_t w, const double* rot1,
                                  const double* rot2, const double* rot3, unsigned n_classes, const DerivedFusedClass* cls,
                                  float* out, unsigned cap_total);

}  // namespace ssw
