// The inverse instances of pair_gemm_f64_kernel in four parts (SSW_INV_PART 0 .. 3: one translation unit each --
// dct_pair_f64_inv.hip, _inv2.hip, _inv3.hip, _inv4.hip -- the template body is instantiated ~16 times per part and one unit took
// 4.5 minutes to compile), or all of them in dct_pair_f64.hip in the -DSSW_TILE_TRACE diagnostic build (SSW_INV_PART -1).
namespace ssw {

int launch_pair_gemm_inverse_part1(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk);
int launch_pair_gemm_inverse_part2(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk);
int launch_pair_gemm_inverse_part3(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk);

#if SSW_INV_PART == 0 || SSW_INV_PART == -1
int launch_pair_gemm_inverse_instances(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                       unsigned long long nblk) {
    switch (inst.epi) {
    case EPI_INV: SSW_LAUNCH_ROWCOL(EPI_INV, false); break;
    case EPI_INV_E: SSW_LAUNCH_ROWCOL(EPI_INV_E, false); break;
    case EPI_INV_OT: return launch_pair_gemm_inverse_part1(st, ml, ep, inst, is_row, small, nblk);
    case EPI_INV_O_RGB: return launch_pair_gemm_inverse_part3(st, ml, ep, inst, is_row, small, nblk);
    case EPI_INV_O: return is_row ? launch_pair_gemm_inverse_part2(st, ml, ep, inst, is_row, small, nblk)
                                  : launch_pair_gemm_inverse_part3(st, ml, ep, inst, is_row, small, nblk);
    default: return SSW_ERR_BAD_ARG;
    }
    return SSW_OK;
}
#endif

#if SSW_INV_PART == 1 || SSW_INV_PART == -1
int launch_pair_gemm_inverse_part1(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk) {
    if (inst.samex) { if (is_row) return SSW_ERR_BAD_ARG; SSW_LAUNCH_PAIR_SUB(true, EPI_INV_OT, true, 1); }
    else if (is_row) SSW_LAUNCH_PAIR_SUB(false, EPI_INV_OT, false, 1);
    else SSW_LAUNCH_PAIR_SUB(true, EPI_INV_OT, false, 1);
    return SSW_OK;
}
#endif

#if SSW_INV_PART == 2 || SSW_INV_PART == -1
int launch_pair_gemm_inverse_part2(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk) {
    (void)is_row;                                   // row passes
    if (inst.samex) SSW_LAUNCH_PAIR(false, EPI_INV_O, true); else SSW_LAUNCH_PAIR(false, EPI_INV_O, false);
    return SSW_OK;
}
#endif

#if SSW_INV_PART == 3 || SSW_INV_PART == -1
int launch_pair_gemm_inverse_part3(hipStream_t st, const PairMulti& ml, Epilogue ep, const PairInstance& inst, bool is_row, bool small,
                                   unsigned long long nblk) {
    (void)is_row;                                   // column passes, with or without Writer::result's RGB epilogue
    if (inst.epi == EPI_INV_O_RGB) {
        if (inst.samex) SSW_LAUNCH_PAIR_SUB(true, EPI_INV_O_RGB, true, 0); else SSW_LAUNCH_PAIR_SUB(true, EPI_INV_O_RGB, false, 0);
    } else {
        if (inst.samex) SSW_LAUNCH_PAIR(true, EPI_INV_O, true); else SSW_LAUNCH_PAIR(true, EPI_INV_O, false);
    }
    return SSW_OK;
}
#endif

}  // namespace ssw
