// What the CatmullRom resize kernels of attack.hip (ssw_resize_rgb8) and restore.hip (ssw_restore_rgb8) share: the tile
// shape, the vertical pass of a block, the per-pixel horizontal accumulation and the clamp + round to a byte.  Both files
// take these from here and nowhere else, so the two resizes cannot drift apart in bits (`image 0.24.3` semantics,
// restated from the crate's published behaviour: vertical pass into f32, horizontal pass, every product and sum rounded
// on its own, taps in ascending order; parity unpinned -- see attack.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "ssw_internal.hpp"

namespace ssw {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float rz_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4r __attribute__((ext_vector_type(4)));

// One block = one tile of OYB x OXB output pixels (resize_fused_kernel, restore_resize_kernel)
struct ResizeTile {
    unsigned oyb, oxb;            // output tile (powers of two, oxb >= 4)
    unsigned pitch;               // elements (bytes of s_in, floats of s_v) per LDS row, multiple of 16
    unsigned in_rows;             // LDS rows of the input tile
    unsigned tiles_x, tiles_y;
    unsigned oxb_log2;
};

// round(clamp(t, 0, 255)) with halves away from zero, as an integer -- exactly: scaling by 2^16 is exact, the
// conversion truncates, and floor(c * 2^16) still tells whether the fraction reaches 1/2
__device__ inline uint32_t resize_to_u8(float t) {
    const float c = __builtin_amdgcn_fmed3f(t, 0.0f, 255.0f);     // = clamp for the finite sums this sees
    return ((uint32_t)(c * 65536.0f) + 0x8000u) >> 16;
}

// vertical pass of one block (vertical_sample of the crate): t = sum_i (float)in[left + i][e] * w[i], i ascending, mul and
// add rounded separately; pieces of NW 32-bit words (4 NW bytes) per thread.  Bytes are bytes: any channel count.
template <int NW>
__device__ inline void resize_vertical_pieces(const unsigned char* s_in, float* s_v, const float* s_wv, const uint32_t* s_lv,
                                              const uint32_t* s_cv, unsigned r0, unsigned noy, unsigned pieces, unsigned vmax,
                                              unsigned pitch, unsigned tid) {
    typedef unsigned int uvec __attribute__((ext_vector_type(NW)));
    for (unsigned it = tid; it < noy * pieces; it += 256) {
        const unsigned j = it / pieces, ck = it - j * pieces;
        const unsigned n = s_cv[j];
        const unsigned char* col = s_in + (s_lv[j] - r0) * pitch + 4 * NW * ck;
        const float* wv = s_wv + j * vmax;
        rz_f32x2 t[2 * NW];
#pragma unroll
        for (int u = 0; u < 2 * NW; ++u) t[u] = (rz_f32x2){0.0f, 0.0f};
#pragma unroll 2
        for (unsigned i = 0; i < n; ++i) {
            const uvec v = *reinterpret_cast<const uvec*>(col + i * pitch);
            const float wi = wv[i];
            const rz_f32x2 ww = {wi, wi};
#pragma unroll
            for (int u = 0; u < NW; ++u) {
                const rz_f32x2 a = {(float)(v[u] & 0xFF), (float)((v[u] >> 8) & 0xFF)};
                const rz_f32x2 b = {(float)((v[u] >> 16) & 0xFF), (float)(v[u] >> 24)};
                t[2 * u] += a * ww;
                t[2 * u + 1] += b * ww;
            }
        }
        f32x4* o = reinterpret_cast<f32x4*>(s_v + j * pitch + 4 * NW * ck);
#pragma unroll
        for (int u = 0; u < NW; ++u) o[u] = (f32x4){t[2 * u][0], t[2 * u][1], t[2 * u + 1][0], t[2 * u + 1][1]};
    }
}

// horizontal pass of one output pixel with C interleaved channels (horizontal_sample): t_c = sum_i strip[left + i][c] * w[i];
// src: the strip at the pixel's first tap, wh: the pixel's column of the tap-major weight table (stride oxb)
template <int C>
__device__ inline void resize_horizontal_pixel(const float* src, const float* wh, unsigned n, unsigned oxb, float (&t)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = 0.0f;
#pragma unroll 4
    for (unsigned i = 0; i < n; ++i) {
        const float wi = wh[i * oxb];
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] += src[C * i + c] * wi;
    }
}

// bytes of dynamic LDS in front of the input tile: s_v f32 [oyb][pitch] | s_wh f32 [hmax][oxb] | s_wv f32 [oyb][vmax] |
// meta u32 [2 oyb + 2 oxb], rounded up to 16
__host__ __device__ inline unsigned resize_lds_in_offset(const ResizeTile& tl, unsigned hmax, unsigned vmax) {
    return ((tl.oyb * tl.pitch + tl.oxb * hmax + tl.oyb * vmax + 2 * tl.oyb + 2 * tl.oxb) * 4 + 15) & ~15u;
}

// reach in input samples of 1, 2, 4 .. 128 consecutive outputs, the maximum over all aligned groups (DeviceTaps::span)
inline void resize_spans(const ResizeTaps& t, size_t out_len, uint32_t (&span)[8]) {
    for (int e = 0; e < 8; ++e) {
        const size_t g = (size_t)1 << e;
        uint32_t m = 0;
        for (size_t o = 0; o < out_len; o += g) {
            const size_t last = (o + g < out_len ? o + g : out_len) - 1;
            m = m > t.left[last] + t.count[last] - t.left[o] ? m : t.left[last] + t.count[last] - t.left[o];
        }
        span[e] = m;
    }
}

// tile shape: the cheapest one (input bytes loaded + vertical taps per output pixel) whose LDS footprint lets two
// blocks share a CU; spans = reach (in input samples) of 1, 2, 4, ... 128 consecutive outputs (DeviceTaps::span);
// ch interleaved input channels, 3 output bytes per pixel.  ey_min / ex_min: the smallest tile (log2) the caller can use --
// locate_rung_kernel wants whole 8 x 8 boxes in a tile
inline bool pick_resize_tile(const DeviceTaps& vt, const DeviceTaps& ht, size_t nw, size_t nh, unsigned ch, ResizeTile* out,
                             size_t* lds_bytes, int ey_min = 0, int ex_min = 2) {
    double best = 1e300;
    bool found = false;
    const double vtaps = (double)(vt.span[0] ? vt.span[0] : 1);
    for (int ey = ey_min; ey < 8; ++ey)
        for (int ex = ex_min; ex < 8; ++ex) {                           // OXB >= 4 (a multiple of 4)
            const unsigned oyb = 1u << ey, oxb = 1u << ex;
            if (oyb > 2 * nh || oxb > 2 * nw) continue;
            const unsigned rows = vt.span[ey], px = ht.span[ex];
            if (!rows || !px) continue;
            const unsigned pitch = (px * ch + 3 + 2 * ch + 15) / 16 * 16;   // + up to 3 bytes of alignment slack + 2 pixels the quad path may read past the reach; 16-byte LDS accesses
            const size_t out_tile = (size_t)oyb * oxb * 3;
            const size_t in_tile = (size_t)rows * pitch;
            const size_t lds = (size_t)oyb * pitch * 4 + ((size_t)oxb * ht.max_taps + (size_t)oyb * vt.max_taps) * 4 +
                               (2 * (size_t)oyb + 2 * (size_t)oxb) * 4 + (in_tile > out_tile ? in_tile : out_tile) + 16;
            if ((size_t)oxb * ht.max_taps > 1024 || (size_t)oyb * vt.max_taps > 1024) continue;   // tap tables: <= 4 values per thread
            if (lds > 78 * 1024) continue;                               // two blocks per CU (160 KB of LDS)
            const double cost = ((double)rows * pitch + (double)oyb * pitch * vtaps) / ((double)oyb * oxb);
            if (cost < best) {
                best = cost;
                found = true;
                *out = ResizeTile{oyb, oxb, pitch, rows, (unsigned)((nw + oxb - 1) / oxb), (unsigned)((nh + oyb - 1) / oyb), (unsigned)ex};
                *lds_bytes = lds;
            }
        }
    return found;
}

}  // namespace ssw
