// The insert functions of Writer::embed_watermark (src/algorithm.rs:414-432), shared by embed_kernel (select.hip) and the
// per-copy coefficient changes of the fingerprint path (fingerprint.hip): one definition, so both compute the same f32 value
// (built with -ffp-contract=off like every translation unit of the library).
#pragma once
#include "ssw_internal.hpp"

namespace ssw {

__device__ inline float insert_fn(int method, float alpha, float original, float mark) {
    if (method == SSW_OPTION1) return original + alpha * mark;              // :414-416
    if (method == SSW_OPTION2) return original * (1.0f + alpha * mark);     // :420-424
    return original * expf(alpha * mark);                                   // :428-432
}

}  // namespace ssw
