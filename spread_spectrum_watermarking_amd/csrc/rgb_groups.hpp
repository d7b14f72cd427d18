// Groups of four 8-bit RGB pixels -- twelve bytes, one load of three dwords at any alignment -- and their lumas, shared by the
// kernels that read frames as bytes (collude.hip, ssim.hip).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace ssw {

__device__ inline void load12(const uint8_t* __restrict__ p, uint32_t (&v)[3]) { __builtin_memcpy(v, p, 12); }
__device__ inline uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
// the luma of ssw_locate_rgb8 / ssw_quality_rgb8 / ssw_ssim_rgb8
__device__ inline uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }
// the lumas of the four pixels of a group: weights 77, 150, 29 on three consecutive bytes
__device__ inline void luma4(const uint32_t (&v)[3], uint32_t (&l)[4]) {
    const uint32_t p1 = (uint32_t)((((uint64_t)v[1] << 32) | v[0]) >> 24), p2 = (uint32_t)((((uint64_t)v[2] << 32) | v[1]) >> 16);
    l[0] = dot4(v[0], 0x001D964Du, 128u) >> 8;
    l[1] = dot4(p1, 0x001D964Du, 128u) >> 8;
    l[2] = dot4(p2, 0x001D964Du, 128u) >> 8;
    l[3] = dot4(v[2], 0x1D964D00u, 128u) >> 8;
}

}  // namespace ssw
