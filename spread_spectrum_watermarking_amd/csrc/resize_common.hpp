// The fused CatmullRom tile of attack.hip (ssw_resize_rgb8), restore.hip (ssw_restore_rgb8) and locate.hip (the rungs of
// ssw_locate_scaled_rgb8): its shape and LDS layout, the reach of a block, the tile's front end (tap tables and input tile
// into LDS, vertical pass), the per-pixel horizontal accumulation and the clamp + round to a byte, and on the host the
// choice of the tile and the dynamic-LDS limit it needs.  The three files take these from here and nowhere else, so the
// resizes cannot drift apart in bits or in layout (`image 0.24.3` semantics, restated from the crate's published
// behaviour: vertical pass into f32, horizontal pass, every product and sum rounded on its own, taps in ascending order;
// parity unpinned -- see attack.hip).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <utility>
#include <vector>

#include "ssw_internal.hpp"

namespace ssw {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float rz_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4r __attribute__((ext_vector_type(4)));

// One block = one tile of OYB x OXB output pixels (resize_fused_kernel, restore_resize_kernel, locate_rung_kernel)
struct ResizeTile {
    unsigned oyb, oxb;            // output tile (powers of two, oxb >= 4)
    unsigned pitch;               // elements (bytes of s_in, floats of s_v) per LDS row, multiple of 16
    unsigned in_rows;             // LDS rows of the input tile
    unsigned tiles_x, tiles_y;
    unsigned oxb_log2;
};

// the tap tables of the two passes ([out_len] left, count; [out_len][max] weights), device pointers; a kernel argument
struct ResizeTapPtrs {
    const uint32_t* vleft; const uint32_t* vcount; const float* vweights; unsigned vmax;
    const uint32_t* hleft; const uint32_t* hcount; const float* hweights; unsigned hmax;
};
inline ResizeTapPtrs resize_tap_ptrs(const DeviceTaps& vt, const DeviceTaps& ht) {
    return ResizeTapPtrs{vt.left, vt.count, vt.weights, vt.max_taps, ht.left, ht.count, ht.weights, ht.max_taps};
}
// tables that lie in one buffer of 32-bit words (the scale ladder's upload): offsets in words; shape: max_taps and span only
struct TapRef { uint32_t left, count, weights; DeviceTaps shape; };
inline ResizeTapPtrs resize_tap_ptrs(const uint32_t* words, const TapRef& vt, const TapRef& ht) {
    return ResizeTapPtrs{words + vt.left, words + vt.count, reinterpret_cast<const float*>(words + vt.weights), vt.shape.max_taps,
                         words + ht.left, words + ht.count, reinterpret_cast<const float*>(words + ht.weights), ht.shape.max_taps};
}

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
// the dynamic LDS of a block; pitch is a multiple of 16: 16-byte LDS accesses throughout.  `in` is free again after the
// vertical pass: the callers stage their output tile there
struct ResizeLds {
    float* v;                     // f32 strip of the vertical pass [oyb][pitch]
    float* wh;                    // [hmax][oxb] (tap-major)
    float* wv;                    // [oyb][vmax]
    uint32_t *lv, *cv, *lh, *ch;  // left / count of the tile's rows and columns
    unsigned char* in;            // u8 input tile [in_rows][pitch]
};
// (offset arithmetic on `smem` itself: a pointer rebuilt from an integer loses its LDS address space and every access
//  through it becomes a flat load)
__device__ __forceinline__ ResizeLds resize_lds_carve(unsigned char* smem, const ResizeTile& tl, unsigned hmax, unsigned vmax) {
    ResizeLds l;
    l.v = reinterpret_cast<float*>(smem);
    l.wh = l.v + (size_t)tl.oyb * tl.pitch;
    l.wv = l.wh + (size_t)tl.oxb * hmax;
    l.lv = reinterpret_cast<uint32_t*>(l.wv + (size_t)tl.oyb * vmax);
    l.cv = l.lv + tl.oyb;
    l.lh = l.cv + tl.oyb;
    l.ch = l.lh + tl.oxb;
    l.in = smem + resize_lds_in_offset(tl, hmax, vmax);
    return l;
}

// What tile `tile` of an out_w x out_h output covers and reaches in its input of C interleaved channels: output pixels
// [oy0, oy0 + noy) x [ox0, ox0 + nox), input rows [r0, r0 + nrows) and `words` 32-bit words of each from byte a0 (a multiple
// of 4) on.  Left / right bounds grow with the output index, so the reach is first left .. last right (block-uniform scalar
// loads; everything after is addressed from them).
struct ResizeReach { unsigned oy0, ox0, noy, nox, r0, nrows, a0, words; };
template <int C>
__device__ __forceinline__ ResizeReach resize_tile_reach(const ResizeTapPtrs& t, const ResizeTile& tl, unsigned tile, unsigned out_w,
                                                         unsigned out_h) {
    ResizeReach r;
    const unsigned tx = tile % tl.tiles_x, ty = tile / tl.tiles_x;
    r.oy0 = ty * tl.oyb; r.ox0 = tx * tl.oxb;
    r.noy = out_h - r.oy0 < tl.oyb ? out_h - r.oy0 : tl.oyb;
    r.nox = out_w - r.ox0 < tl.oxb ? out_w - r.ox0 : tl.oxb;
    r.r0 = t.vleft[r.oy0];
    r.nrows = t.vleft[r.oy0 + r.noy - 1] + t.vcount[r.oy0 + r.noy - 1] - r.r0;
    const unsigned b0 = t.hleft[r.ox0] * C, b1 = (t.hleft[r.ox0 + r.nox - 1] + t.hcount[r.ox0 + r.nox - 1]) * C;
    r.a0 = b0 & ~3u;
    r.words = (b1 - r.a0 + 3) / 4;
    return r;
}

// tap tables and input tile -> LDS with no alignment assumed of the input [..][sw][C]: 32-bit loads where the rows ARE 4-byte
// aligned, bytes elsewhere
template <int C>
__device__ __forceinline__ void resize_tile_load_any(const ResizeLds& l, const ResizeTapPtrs& t, const ResizeTile& tl, const ResizeReach& r,
                                                     const uint8_t* __restrict__ in, unsigned sw, unsigned tid) {
    const unsigned row_bytes = sw * C;
    for (unsigned i = tid; i < r.nox * t.hmax; i += 256) { const unsigned x = i / t.hmax, tp = i - x * t.hmax; l.wh[tp * tl.oxb + x] = t.hweights[(size_t)r.ox0 * t.hmax + i]; }   // tap-major
    for (unsigned i = tid; i < r.noy * t.vmax; i += 256) l.wv[i] = t.vweights[(size_t)r.oy0 * t.vmax + i];
    if (tid < r.noy) { l.lv[tid] = t.vleft[r.oy0 + tid]; l.cv[tid] = t.vcount[r.oy0 + tid]; }
    if (tid < r.nox) { l.lh[tid] = t.hleft[r.ox0 + tid]; l.ch[tid] = t.hcount[r.ox0 + tid]; }
    const uint8_t* __restrict__ src = in + (size_t)r.r0 * row_bytes + r.a0;
    const unsigned avail = row_bytes - r.a0;                        // bytes from a0 to the end of the input's row
    const bool rows_aligned = (reinterpret_cast<uintptr_t>(src) & 3) == 0 && (row_bytes & 3) == 0;
    for (unsigned it = tid; it < r.nrows * r.words; it += 256) {
        const unsigned row = it / r.words, wd = it - row * r.words;
        const uint8_t* p = src + (size_t)row * row_bytes + 4 * wd;
        uint32_t v = 0;
        if (rows_aligned && 4 * wd + 4 <= avail) v = *reinterpret_cast<const uint32_t*>(p);
        else {                                                      // stay inside the row: never past the input's last byte
#pragma unroll
            for (unsigned e = 0; e < 4; ++e) if (4 * wd + e < avail) v |= (uint32_t)p[e] << (8 * e);
        }
        *reinterpret_cast<uint32_t*>(l.in + row * tl.pitch + 4 * wd) = v;
    }
}

// vertical pass of a block over whole LDS rows, slack included: every strip element the horizontal pass may touch is then a
// finite sum (bytes the tile did not load give sums nobody reads).  One thread = 16 (or, when that leaves half the block
// idle, 8) consecutive bytes of one output row: that many independent sums per LDS read.
__device__ __forceinline__ void resize_vertical_pass(const ResizeLds& l, const ResizeTile& tl, const ResizeReach& r, unsigned vmax,
                                                     unsigned tid) {
    const unsigned chunks16 = tl.pitch / 16;
    if (r.noy * chunks16 >= 192) resize_vertical_pieces<4>(l.in, l.v, l.wv, l.lv, l.cv, r.r0, r.noy, chunks16, vmax, tl.pitch, tid);
    else                         resize_vertical_pieces<2>(l.in, l.v, l.wv, l.lv, l.cv, r.r0, r.noy, tl.pitch / 8, vmax, tl.pitch, tid);
}

// The front end of a fused tile: reach, tables and input tile -> LDS, vertical pass.  On return the strip l.v is complete and
// l.in is free; the caller's horizontal pass follows.
template <int C>
__device__ __forceinline__ ResizeReach resize_tile_front(const ResizeLds& l, const ResizeTapPtrs& t, const ResizeTile& tl, unsigned tile,
                                                         unsigned out_w, unsigned out_h, const uint8_t* __restrict__ in, unsigned sw) {
    const unsigned tid = threadIdx.x;
    const ResizeReach r = resize_tile_reach<C>(t, tl, tile, out_w, out_h);
    resize_tile_load_any<C>(l, t, tl, r, in, sw, tid);
    __syncthreads();
    resize_vertical_pass(l, tl, r, t.vmax, tid);
    __syncthreads();
    return r;
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

// every tap table of a call (the scale ladder of locate.hip, the sizes of locate_free.hip) in one host buffer: one upload, one wait
struct LadderTaps {
    std::vector<uint32_t> words;
    std::map<std::pair<size_t, size_t>, TapRef> refs;
    const TapRef& get(size_t in_len, size_t out_len) {
        const auto key = std::make_pair(in_len, out_len);
        const auto it = refs.find(key);
        if (it != refs.end()) return it->second;
        ResizeTaps t;
        build_resize_taps(in_len, out_len, t);
        TapRef r;
        r.left = (uint32_t)words.size();   words.insert(words.end(), t.left.begin(), t.left.end());
        r.count = (uint32_t)words.size();  words.insert(words.end(), t.count.begin(), t.count.end());
        r.weights = (uint32_t)words.size();
        words.resize(words.size() + t.weights.size());
        std::memcpy(words.data() + r.weights, t.weights.data(), t.weights.size() * sizeof(float));
        r.shape.max_taps = t.max_taps;
        resize_spans(t, out_len, r.shape.span);
        return refs[key] = r;
    }
};

// The dynamic LDS a fused kernel may ask for: above the 64 KB a kernel gets by default, so every kernel that takes a tile of
// pick_resize_tile needs the per-device function attribute -- set once per device (`done`: the caller's static flags; two
// host threads, two contexts: no plain bools)
constexpr size_t RESIZE_LDS_LIMIT = 80 * 1024;
inline int resize_raise_lds_limit(std::initializer_list<const void*> kernels, std::atomic<bool> (&done)[64]) {
    int dev = 0;
    SSW_HIP_CHECK(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < 64;
    if (known && done[dev].load(std::memory_order_acquire)) return SSW_OK;
    for (const void* k : kernels) SSW_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RESIZE_LDS_LIMIT));
    if (known) done[dev].store(true, std::memory_order_release);
    return SSW_OK;
}

// tile shape: the cheapest one (input bytes loaded + vertical taps per output pixel) whose LDS footprint lets two
// blocks share a CU; spans = reach (in input samples) of 1, 2, 4, ... 128 consecutive outputs (DeviceTaps::span);
// ch interleaved input channels, 3 output bytes per pixel.  ey_min / ex_min: the smallest tile (log2) the caller can use --
// locate_rung_kernel wants whole 8 x 8 boxes in a tile.  extra(oyb, oxb): bytes of LDS the caller puts behind the tile
// (locate_free_kernel's window of the original), counted against the same budget; *lds_bytes stays the tile's own
inline bool pick_resize_tile(const DeviceTaps& vt, const DeviceTaps& ht, size_t nw, size_t nh, unsigned ch, ResizeTile* out,
                             size_t* lds_bytes, int ey_min = 0, int ex_min = 2, size_t (*extra)(unsigned, unsigned) = nullptr) {
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
            const ResizeTile tl{oyb, oxb, pitch, rows, (unsigned)((nw + oxb - 1) / oxb), (unsigned)((nh + oyb - 1) / oyb), (unsigned)ex};
            const size_t lds = resize_lds_in_offset(tl, ht.max_taps, vt.max_taps) + (in_tile > out_tile ? in_tile : out_tile);
            if ((size_t)oxb * ht.max_taps > 1024 || (size_t)oyb * vt.max_taps > 1024) continue;   // tap tables: <= 4 values per thread
            if (lds + (extra ? extra(oyb, oxb) : 0) > RESIZE_LDS_LIMIT - 2 * 1024) continue;   // two blocks per CU (160 KB of LDS)
            const double cost = ((double)rows * pitch + (double)oyb * pitch * vtaps) / ((double)oyb * oxb);
            if (cost < best) {
                best = cost;
                found = true;
                *out = tl;
                *lds_bytes = lds;
            }
        }
    return found;
}

}  // namespace ssw
