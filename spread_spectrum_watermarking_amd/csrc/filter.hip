// The filter-menu attacks (ssw_filter_rgb8): a marked copy after a photo editor's Gaussian blur, unsharp mask or 3 x 3 median.
// include/ssw.h states the definitions; they are Pillow's (ImageFilter.GaussianBlur, UnsharpMask, MedianFilter(3)), integer
// arithmetic on the bytes, so the frames equal the numpy restatement of tests/test_filter_cpu.py -- and with it Pillow -- exactly.
// The reference has no counterpart.
//
// Kernels (grid z: the jobs of a launch, FL_BATCH at most, their constants as kernel arguments):
//   blur_rows_kernel    a block owns FL_RW x FL_RH pixels and loads them with 3 (r + 1) pixels more on either side (rounded up to
//                       whole groups of four pixels on the left, so that the tile starts on a dword of LDS) as interleaved bytes.
//                       Three box passes ping-pong between two LDS buffers; the span a pass writes shrinks by r + 1 on either
//                       side.  A thread takes a run of FL_RUN outputs of one channel of FOUR rows (q, q + 4, q + 8, q + 12) with
//                       sliding sums: per output two byte reads and one byte write whatever r is, the index arithmetic shared by
//                       the four.  12 lines x 19 .. 21 runs fill the 256 threads once per pass.  The result goes to the plane in
//                       the context's workspace.
//   blur_cols_kernel    the same along y on the plane, which it reads as an h x 3w matrix of bytes: every byte column is a line.
//                       A block owns FL_CW bytes x FL_CH rows (+ 3 (r + 1) rows above and below); a thread takes a run of FL_CRUN
//                       outputs of four adjacent byte columns -- one dword of LDS per read and write -- and consecutive lanes take
//                       consecutive dwords.  Rows of the tile lie 51 dwords apart, so the 48 lanes of one run and the 16 of the
//                       next fall on 64 different banks.  Its epilogue writes the frame: the blurred bytes, or UNSHARP against the
//                       original pixel, which it loads itself.
//   Both take one of two forms per run: box_run4_inside where no index needs the clamp and the run is whole (constant strides, an
//   unrolled loop: every LDS address is a register plus an immediate), box_run4 at the frame's edges and for the last, shorter run.
//   median_kernel       a tile of FL_MW x FL_MH pixels with a one-pixel border, edge pixels repeated while loading.  A thread
//                       takes twelve bytes of a row: per output dword the nine neighbours are nine dwords (the ones 3 bytes to
//                       the left and right cut out of two aligned LDS dwords), split into even and odd bytes as pairs of 16 bits;
//                       the 19-comparator median-of-9 network runs on the pairs with packed 16-bit min / max.
// At a frame edge the clamp is applied to the index of EVERY pass's input (at()): the second pass sees the first pass's edge
// output repeated, as the full-frame restatement does; positions outside the frame are never computed or read.
// Multiplications: sums stay below 2^13 and the weights below 2^24 (ww == 2^24, which a radius below about 1e-4 gives, is passed
// as a flag: the pass is then the identity), so the 24-bit multiply applies and every value fits 32 bits unsigned.
#include <algorithm>
#include <cmath>

#include "filter_tables.hpp"
#include "rgb_groups.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned FL_BATCH = 16;                       // jobs per launch
constexpr size_t FL_GROUP_BYTES = (size_t)64 << 20;     // planes kept at a time (one job's, if it is larger)
constexpr size_t FL_SIDE_MAX = 65535;
constexpr unsigned FL_HALO = 3 * (FILTER_R_MAX + 1);    // 24 samples: what three passes reach
constexpr unsigned FL_RW = 256, FL_RH = 16;             // the row kernel's tile, pixels
constexpr unsigned FL_RUN = 14;                         // outputs of a thread's run along a row: 12 x 19 .. 21 runs fill 256 threads once
constexpr unsigned FL_RPITCH = 3 * (FL_RW + 2 * FL_HALO);   // bytes of a tile row in LDS, a multiple of 12
constexpr unsigned FL_CW = 192, FL_CH = 96;             // the column kernel's tile: bytes (16 groups of four pixels) x rows
constexpr unsigned FL_CRUN = 16;                        // outputs of a thread's run along a column
constexpr unsigned FL_CROWS = FL_CH + 2 * FL_HALO;
constexpr unsigned FL_CPITCH = FL_CW + 12;              // bytes of a tile row in LDS: 51 dwords, so that runs 16 rows apart start 48 banks apart
constexpr unsigned FL_MW = 64, FL_MH = 32;              // the median kernel's tile, pixels
constexpr unsigned FL_MPITCH = 208;                     // 4 (a pad byte + the left pixel) + 192 + 3 (the right pixel), rounded up
static_assert(FL_RH == 16, "a thread of blur_rows_kernel takes rows q, q + 4, q + 8 and q + 12");
static_assert(FL_HALO % 4 == 0 && FL_RW % 4 == 0 && FL_RPITCH % 12 == 0 && FL_CW % 12 == 0 && FL_CPITCH % 4 == 0 && FL_RH % 4 == 0,
              "tiles start on a dword of LDS");

struct BlurDesc { uint32_t frame, out, r, ww, fw, percent, threshold, unsharp; };   // out: the job's index in the call
struct BlurBatch { BlurDesc it[FL_BATCH]; };
struct MedianDesc { uint32_t frame, out; };
struct MedianBatch { MedianDesc it[FL_BATCH]; };

struct BoxWeights { uint32_t ww, fw, whole; };          // whole: ww == 2^24 (then fw == 0 and r == 0)

// One run of a box pass along FOUR lines that share their indices: outputs xs .. xe - 1 of each.  DWORD: the lines are the four
// bytes of a dword (adjacent byte columns), read and written as one; else they lie `lstride` bytes apart.  in / out point at the
// first line's sample a_lo; samples lie `stride` bytes apart; n is the frame's length along the lines.  The index arithmetic and
// the clamp are paid once for four outputs.
template <bool DWORD>
__device__ inline void box_run4(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int stride, int lstride, int a_lo, int n, int xs,
                                int xe, int r, BoxWeights k) {
    auto at = [&](int a, uint32_t (&v)[4]) {
        const int o = (min(max(a, 0), n - 1) - a_lo) * stride;
        if (DWORD) {
            const uint32_t d = *reinterpret_cast<const uint32_t*>(in + o);
            v[0] = d & 0xFFu; v[1] = (d >> 8) & 0xFFu; v[2] = (d >> 16) & 0xFFu; v[3] = d >> 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = in[o + j * lstride];
        }
    };
    uint32_t acc[4] = {0, 0, 0, 0}, left[4], right[4];
    for (int d = -r; d <= r; ++d) {
        at(xs + d, right);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += right[j];
    }
    at(xs - r - 1, left);
    for (int x = xs; x < xe; ++x) {
        at(x + r + 1, right);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = (__umul24(k.ww, acc[j]) + __umul24(k.fw, left[j] + right[j]) + (k.whole ? acc[j] << 24 : 0u) + (1u << 23)) >> 24;
        const int o = (x - a_lo) * stride;
        if (DWORD) {
            *reinterpret_cast<uint32_t*>(out + o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[o + j * lstride] = (uint8_t)v[j];
        }
        at(x - r, left);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += right[j] - left[j];
    }
}

// The same where no index needs the clamp and the run is whole (RUN outputs from sample `rel` of the tile on): the strides are
// compile-time constants and the loop is unrolled, so every LDS address is one of three registers plus an immediate offset.
template <bool DWORD, int STRIDE, int LSTRIDE, int RUN>
__device__ inline void box_run4_inside(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int rel, int r, BoxWeights k) {
    auto load = [](const uint8_t* p, uint32_t (&v)[4]) {
        if (DWORD) {
            const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
            v[0] = d & 0xFFu; v[1] = (d >> 8) & 0xFFu; v[2] = (d >> 16) & 0xFFu; v[3] = d >> 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = p[j * LSTRIDE];
        }
    };
    const uint8_t* __restrict__ pr = in + (rel + r + 1) * STRIDE;            // the sample entering the sum after output 0
    const uint8_t* __restrict__ pl = in + (rel - r) * STRIDE;                // the one leaving it
    uint8_t* __restrict__ po = out + rel * STRIDE;
    uint32_t acc[4] = {0, 0, 0, 0}, left[4], right[4];
    for (const uint8_t* p = pl; p != pr; p += STRIDE) {
        load(p, right);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += right[j];
    }
    load(pl - STRIDE, left);
#pragma unroll
    for (int i = 0; i < RUN; ++i) {
        load(pr + i * STRIDE, right);
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = (__umul24(k.ww, acc[j]) + __umul24(k.fw, left[j] + right[j]) + (k.whole ? acc[j] << 24 : 0u) + (1u << 23)) >> 24;
        if (DWORD) {
            *reinterpret_cast<uint32_t*>(po + i * STRIDE) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) po[i * STRIDE + j * LSTRIDE] = (uint8_t)v[j];
        }
        load(pl + i * STRIDE, left);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += right[j] - left[j];
    }
}
// the run xs .. of a pass over [lo, hi) of a line of n samples needs no clamp and is whole
__device__ inline bool run_inside(int xs, int hi, int n, int r, int run) { return xs - r - 1 >= 0 && xs + run + r < n && xs + run <= hi; }

__device__ inline void lds_store12(uint8_t* p, const uint32_t (&v)[3]) {      // p: a multiple of 4
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
}
__device__ inline void lds_load12(const uint8_t* p, uint32_t (&v)[3]) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
}

// grid: (tiles of FL_RW pixels, bands of FL_RH rows, jobs of the launch); block: 256.  planes: [jobs of the launch][fb]
__global__ __launch_bounds__(256) void blur_rows_kernel(BlurBatch b, const uint8_t* __restrict__ frames, size_t fb, uint32_t w, uint32_t h,
                                                        uint8_t* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) uint8_t s[2][FL_RH * FL_RPITCH];
    const unsigned t = threadIdx.x;
    const BlurDesc& d = b.it[blockIdx.z];
    const int r = (int)d.r, reach = r + 1, halo = 3 * reach;
    const BoxWeights k{d.ww, d.fw, d.ww >> 24};
    const int t0 = (int)(blockIdx.x * FL_RW), t1 = (int)min(blockIdx.x * FL_RW + FL_RW, w);
    const unsigned y0 = blockIdx.y * FL_RH, rows = min(FL_RH, h - y0);
    const int hp = (halo + 3) & ~3;
    const int a_lo = max(t0 - hp, 0), a_hi = min(t1 + halo, (int)w);
    const uint8_t* __restrict__ src = frames + (size_t)d.frame * fb + ((size_t)y0 * w + (size_t)a_lo) * 3;
    const size_t row_bytes = (size_t)w * 3;

    // ---- the tile and its halo: groups of twelve bytes, then the up to nine bytes left of a row
    const unsigned nbytes = 3u * (unsigned)(a_hi - a_lo), groups = nbytes / 12, tail = nbytes - 12 * groups;
    for (unsigned i = t; i < rows * groups; i += 256) {
        const unsigned row = i / groups, g = i - row * groups;
        uint32_t v[3];
        load12(src + row * row_bytes + 12 * g, v);
        lds_store12(&s[0][row * FL_RPITCH + 12 * g], v);
    }
    for (unsigned i = t; i < rows * tail; i += 256) {
        const unsigned row = i / tail, j = 12 * groups + (i - row * tail);
        s[0][row * FL_RPITCH + j] = src[row * row_bytes + j];
    }
    __syncthreads();

    // ---- three passes: 0 -> 1 -> 0 -> 1
#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
        const int e = (2 - p) * reach, lo = max(t0 - e, 0), hi = min(t1 + e, (int)w);
        const unsigned runs = (unsigned)(hi - lo + FL_RUN - 1) / FL_RUN;
        const uint8_t* in = s[p & 1];
        uint8_t* out = s[(p & 1) ^ 1];
        for (unsigned i = t; i < 12 * runs; i += 256) {                    // rows q, q + 4, q + 8, q + 12 of one channel: rows beyond
            const unsigned line = i / runs, run = i - line * runs, q = line / 3, c = line - q * 3;     // the frame's are computed on whatever
            if (q >= rows) continue;                                                                     // LDS holds and never stored
            const int xs = lo + (int)(run * FL_RUN);
            const uint8_t* pi = in + q * FL_RPITCH + c;
            uint8_t* po = out + q * FL_RPITCH + c;
            if (run_inside(xs, hi, (int)w, r, FL_RUN)) box_run4_inside<false, 3, 4 * FL_RPITCH, FL_RUN>(pi, po, xs - a_lo, r, k);
            else box_run4<false>(pi, po, 3, 4 * FL_RPITCH, a_lo, (int)w, xs, min(xs + (int)FL_RUN, hi), r, k);
        }
        __syncthreads();
    }

    // ---- the tile's pixels to the plane
    uint8_t* __restrict__ dst = planes + (size_t)blockIdx.z * fb + ((size_t)y0 * w + (size_t)t0) * 3;
    const unsigned off = 3u * (unsigned)(t0 - a_lo), obytes = 3u * (unsigned)(t1 - t0), ogroups = obytes / 12, otail = obytes - 12 * ogroups;
    for (unsigned i = t; i < rows * ogroups; i += 256) {
        const unsigned row = i / ogroups, g = i - row * ogroups;
        uint32_t v[3];
        lds_load12(&s[1][row * FL_RPITCH + off + 12 * g], v);
        __builtin_memcpy(dst + row * row_bytes + 12 * g, v, 12);
    }
    for (unsigned i = t; i < rows * otail; i += 256) {
        const unsigned row = i / otail, j = 12 * ogroups + (i - row * otail);
        dst[row * row_bytes + j] = s[1][row * FL_RPITCH + off + j];
    }
}

__device__ inline uint32_t unsharp_byte(uint32_t in, uint32_t blurred, int percent, int threshold) {
    const int diff = (int)in - (int)blurred;
    if (abs(diff) <= threshold) return in;
    return (uint32_t)min(max((int)in + diff * percent / 100, 0), 255);      // the division truncates toward zero
}
__device__ inline uint32_t unsharp_dword(uint32_t in, uint32_t blurred, int percent, int threshold) {
    uint32_t o = 0;
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) o |= unsharp_byte((in >> (8 * j)) & 0xFFu, (blurred >> (8 * j)) & 0xFFu, percent, threshold) << (8 * j);
    return o;
}

// grid: (tiles of FL_CW bytes of a row, bands of FL_CH rows, jobs of the launch); block: 256.  out_all: the call's dev_out
__global__ __launch_bounds__(256) void blur_cols_kernel(BlurBatch b, const uint8_t* __restrict__ planes, const uint8_t* __restrict__ frames,
                                                        size_t fb, uint32_t w, uint32_t h, uint8_t* __restrict__ out_all) {
    __shared__ __attribute__((aligned(16))) uint8_t s[2][FL_CROWS * FL_CPITCH];
    const unsigned t = threadIdx.x;
    const BlurDesc& d = b.it[blockIdx.z];
    const int r = (int)d.r, reach = r + 1, halo = 3 * reach;
    const BoxWeights k{d.ww, d.fw, d.ww >> 24};
    const size_t row_bytes = (size_t)w * 3;
    const unsigned c0 = blockIdx.x * FL_CW, cb = min(FL_CW, 3 * w - c0);
    const int t0 = (int)(blockIdx.y * FL_CH), t1 = (int)min(blockIdx.y * FL_CH + FL_CH, h);
    const int a_lo = max(t0 - halo, 0), a_hi = min(t1 + halo, (int)h);
    const unsigned lrows = (unsigned)(a_hi - a_lo), groups = cb / 12, tail = cb - 12 * groups, dwords = (cb + 3) / 4;
    const uint8_t* __restrict__ src = planes + (size_t)blockIdx.z * fb + (size_t)a_lo * row_bytes + c0;

    for (unsigned i = t; i < lrows * groups; i += 256) {
        const unsigned row = i / groups, g = i - row * groups;
        uint32_t v[3];
        load12(src + row * row_bytes + 12 * g, v);
        lds_store12(&s[0][row * FL_CPITCH + 12 * g], v);
    }
    for (unsigned i = t; i < lrows * tail; i += 256) {
        const unsigned row = i / tail, j = 12 * groups + (i - row * tail);
        s[0][row * FL_CPITCH + j] = src[row * row_bytes + j];
    }
    __syncthreads();

#pragma unroll 1
    for (int p = 0; p < 3; ++p) {
        const int e = (2 - p) * reach, lo = max(t0 - e, 0), hi = min(t1 + e, (int)h);
        const unsigned runs = (unsigned)(hi - lo + FL_CRUN - 1) / FL_CRUN;
        const uint8_t* in = s[p & 1];
        uint8_t* out = s[(p & 1) ^ 1];
        for (unsigned i = t; i < dwords * runs; i += 256) {                 // four byte columns, one dword: the last of a narrow tile
            const unsigned run = i / dwords, col = i - run * dwords;        // may hold bytes beyond it, which are never stored
            const int xs = lo + (int)(run * FL_CRUN);
            if (run_inside(xs, hi, (int)h, r, FL_CRUN)) box_run4_inside<true, FL_CPITCH, 0, FL_CRUN>(in + 4 * col, out + 4 * col, xs - a_lo, r, k);
            else box_run4<true>(in + 4 * col, out + 4 * col, (int)FL_CPITCH, 0, a_lo, (int)h, xs, min(xs + (int)FL_CRUN, hi), r, k);
        }
        __syncthreads();
    }

    // ---- the frame: the blurred bytes, or UNSHARP against the original
    const size_t at0 = (size_t)t0 * row_bytes + c0;
    const uint8_t* __restrict__ orig = frames + (size_t)d.frame * fb + at0;
    uint8_t* __restrict__ dst = out_all + (size_t)d.out * fb + at0;
    const uint8_t* res = s[1] + (unsigned)(t0 - a_lo) * FL_CPITCH;
    const unsigned orows = (unsigned)(t1 - t0);
    const int percent = (int)d.percent, threshold = (int)d.threshold;
    for (unsigned i = t; i < orows * groups; i += 256) {
        const unsigned row = i / groups, g = i - row * groups;
        uint32_t v[3];
        lds_load12(res + row * FL_CPITCH + 12 * g, v);
        if (d.unsharp) {
            uint32_t o[3];
            load12(orig + row * row_bytes + 12 * g, o);
#pragma unroll
            for (unsigned j = 0; j < 3; ++j) v[j] = unsharp_dword(o[j], v[j], percent, threshold);
        }
        __builtin_memcpy(dst + row * row_bytes + 12 * g, v, 12);
    }
    for (unsigned i = t; i < orows * tail; i += 256) {
        const unsigned row = i / tail, j = 12 * groups + (i - row * tail);
        const uint32_t bl = res[row * FL_CPITCH + j];
        dst[row * row_bytes + j] = (uint8_t)(d.unsharp ? unsharp_byte(orig[row * row_bytes + j], bl, percent, threshold) : bl);
    }
}

typedef unsigned short fl_pk16 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t fl_pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(fl_pk16, a), __builtin_bit_cast(fl_pk16, b)));
}
__device__ inline uint32_t fl_pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(fl_pk16, a), __builtin_bit_cast(fl_pk16, b)));
}
__device__ inline void fl_sort2(uint32_t& a, uint32_t& b) {
    const uint32_t lo = fl_pk_min(a, b), hi = fl_pk_max(a, b);
    a = lo; b = hi;
}
// the median of nine, per 16-bit half: the 19-comparator network
__device__ inline uint32_t median9(uint32_t (&p)[9]) {
    fl_sort2(p[1], p[2]); fl_sort2(p[4], p[5]); fl_sort2(p[7], p[8]);
    fl_sort2(p[0], p[1]); fl_sort2(p[3], p[4]); fl_sort2(p[6], p[7]);
    fl_sort2(p[1], p[2]); fl_sort2(p[4], p[5]); fl_sort2(p[7], p[8]);
    fl_sort2(p[0], p[3]); fl_sort2(p[5], p[8]); fl_sort2(p[4], p[7]);
    fl_sort2(p[3], p[6]); fl_sort2(p[1], p[4]); fl_sort2(p[2], p[5]);
    fl_sort2(p[4], p[7]); fl_sort2(p[4], p[2]); fl_sort2(p[6], p[4]);
    fl_sort2(p[4], p[2]);
    return p[4];
}

// grid: (tiles of FL_MW pixels, bands of FL_MH rows, jobs of the launch); block: 256
__global__ __launch_bounds__(256) void median_kernel(MedianBatch b, const uint8_t* __restrict__ frames, size_t fb, uint32_t w, uint32_t h,
                                                     uint8_t* __restrict__ out_all) {
    // row j of the tile is row clamp(y0 - 1 + j) of the frame: byte 0 unused, 1 .. 3 the pixel left of the tile, 4 .. the tile's
    // bytes, then the pixel right of it -- the frame's own edge pixel where there is none
    __shared__ __attribute__((aligned(16))) uint8_t s[(FL_MH + 2) * FL_MPITCH];
    const unsigned t = threadIdx.x;
    const MedianDesc& d = b.it[blockIdx.z];
    const unsigned x0 = blockIdx.x * FL_MW, tw = min(FL_MW, w - x0), y0 = blockIdx.y * FL_MH, th = min(FL_MH, h - y0);
    const size_t row_bytes = (size_t)w * 3;
    const uint8_t* __restrict__ src = frames + (size_t)d.frame * fb;
    const unsigned tbytes = 3 * tw, groups = tbytes / 12, tail = tbytes - 12 * groups;
    auto frame_row = [&](unsigned j) -> const uint8_t* {
        return src + (size_t)min(max((int)(y0 + j) - 1, 0), (int)h - 1) * row_bytes;
    };
    for (unsigned i = t; i < (th + 2) * groups; i += 256) {
        const unsigned j = i / groups, g = i - j * groups;
        uint32_t v[3];
        load12(frame_row(j) + (size_t)x0 * 3 + 12 * g, v);
        lds_store12(&s[j * FL_MPITCH + 4 + 12 * g], v);
    }
    for (unsigned i = t; i < (th + 2) * tail; i += 256) {
        const unsigned j = i / tail, q = 12 * groups + (i - j * tail);
        s[j * FL_MPITCH + 4 + q] = frame_row(j)[(size_t)x0 * 3 + q];
    }
    for (unsigned i = t; i < (th + 2) * 6; i += 256) {
        const unsigned j = i / 6, q = i - j * 6, c = q % 3;
        if (q < 3) s[j * FL_MPITCH + 1 + c] = frame_row(j)[(size_t)(x0 ? x0 - 1 : 0) * 3 + c];
        else s[j * FL_MPITCH + 4 + tbytes + c] = frame_row(j)[(size_t)min(x0 + tw, w - 1) * 3 + c];
    }
    __syncthreads();

    const unsigned ogroups = (tbytes + 11) / 12;
    uint8_t* __restrict__ dst = out_all + (size_t)d.out * fb + ((size_t)y0 * w + x0) * 3;
    for (unsigned i = t; i < th * ogroups; i += 256) {
        const unsigned row = i / ogroups, g = i - row * ogroups;
        uint32_t D[3][5];                                     // rows above, at, below: the dwords at bytes 12 g .. 12 g + 19 of the LDS row
#pragma unroll
        for (unsigned v = 0; v < 3; ++v) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(&s[(row + v) * FL_MPITCH + 12 * g]);
#pragma unroll
            for (unsigned m = 0; m < 5; ++m) D[v][m] = q[m];
        }
        uint32_t o[3];
#pragma unroll
        for (unsigned m = 0; m < 3; ++m) {
            uint32_t e[9], od[9];
#pragma unroll
            for (unsigned v = 0; v < 3; ++v) {
                const uint32_t n[3] = {(uint32_t)(((((uint64_t)D[v][m + 1]) << 32) | D[v][m]) >> 8), D[v][m + 1],
                                       (uint32_t)(((((uint64_t)D[v][m + 2]) << 32) | D[v][m + 1]) >> 24)};
#pragma unroll
                for (unsigned j = 0; j < 3; ++j) {
                    e[3 * v + j] = n[j] & 0x00FF00FFu;
                    od[3 * v + j] = (n[j] >> 8) & 0x00FF00FFu;
                }
            }
            o[m] = median9(e) | (median9(od) << 8);
        }
        uint8_t* p = dst + row * row_bytes + 12 * g;
        if (12 * g + 12 <= tbytes) {
            __builtin_memcpy(p, o, 12);
        } else {
            for (unsigned j = 0; 12 * g + j < tbytes; ++j) p[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
        }
    }
}

}  // namespace ssw

extern "C" int ssw_filter_rgb8(ssw_ctx* ctx, const uint8_t* dev_frames, size_t n_frames, size_t w, size_t h, const ssw_filter_job* jobs,
                               size_t n_jobs, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_jobs == 0) return SSW_OK;
    if (!dev_frames || !jobs || !dev_out) return SSW_ERR_BAD_ARG;
    if (w == 0 || h == 0 || w > ssw::FL_SIDE_MAX || h > ssw::FL_SIDE_MAX) return SSW_ERR_BAD_DIMS;
    for (size_t i = 0; i < n_jobs; ++i) {
        const ssw_filter_job& j = jobs[i];
        if (j.frame >= n_frames) return SSW_ERR_BAD_ARG;
        const bool radius_ok = std::isfinite(j.radius) && j.radius > 0.0f && j.radius <= ssw::FILTER_RADIUS_MAX;
        switch (j.kind) {
            case SSW_FILTER_BLUR: if (!radius_ok || j.percent || j.threshold) return SSW_ERR_BAD_ARG; break;
            case SSW_FILTER_UNSHARP: if (!radius_ok || j.percent < 1 || j.percent > 1000 || j.threshold > 255) return SSW_ERR_BAD_ARG; break;
            case SSW_FILTER_MEDIAN3: if (!(j.radius == 0.0f) || j.percent || j.threshold) return SSW_ERR_BAD_ARG; break;
            default: return SSW_ERR_BAD_ARG;
        }
    }
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const size_t fb = w * h * 3;
    const size_t group = std::min<size_t>({ssw::FL_BATCH, n_jobs, std::max<size_t>(1, ssw::FL_GROUP_BYTES / fb)});
    bool any_blur = false;
    for (size_t i = 0; i < n_jobs; ++i) any_blur |= jobs[i].kind != SSW_FILTER_MEDIAN3;
    if (any_blur) SSW_TRY(grow(ctx->shared.filter, group * fb));
    uint8_t* planes = ctx->shared.filter.as<uint8_t>();
    const uint32_t W = (uint32_t)w, H = (uint32_t)h;
    // per job: the frame in and the frame out, whatever the kind
    StageTimer t(ctx, SSW_STAGE_CONVERT, st, (double)n_jobs * (double)(2 * fb));
    for (size_t i0 = 0; i0 < n_jobs; i0 += group) {
        const size_t i1 = std::min(i0 + group, n_jobs);
        ssw::BlurBatch bb{};
        ssw::MedianBatch mb{};
        unsigned nb = 0, nm = 0;
        for (size_t i = i0; i < i1; ++i) {
            const ssw_filter_job& j = jobs[i];
            if (j.kind == SSW_FILTER_MEDIAN3) { mb.it[nm++] = ssw::MedianDesc{j.frame, (uint32_t)i}; continue; }
            const ssw::BlurConstants c = ssw::blur_constants(j.radius);
            bb.it[nb++] = ssw::BlurDesc{j.frame, (uint32_t)i, c.r, c.ww, c.fw, j.percent, j.threshold, j.kind == SSW_FILTER_UNSHARP ? 1u : 0u};
        }
        if (nb) {
            ssw::blur_rows_kernel<<<dim3((W + ssw::FL_RW - 1) / ssw::FL_RW, (H + ssw::FL_RH - 1) / ssw::FL_RH, nb), 256, 0, st>>>(
                bb, dev_frames, fb, W, H, planes);
            SSW_HIP_CHECK(hipGetLastError());
            ssw::blur_cols_kernel<<<dim3((3 * W + ssw::FL_CW - 1) / ssw::FL_CW, (H + ssw::FL_CH - 1) / ssw::FL_CH, nb), 256, 0, st>>>(
                bb, planes, dev_frames, fb, W, H, dev_out);
            SSW_HIP_CHECK(hipGetLastError());
        }
        if (nm) {
            ssw::median_kernel<<<dim3((W + ssw::FL_MW - 1) / ssw::FL_MW, (H + ssw::FL_MH - 1) / ssw::FL_MH, nm), 256, 0, st>>>(
                mb, dev_frames, fb, W, H, dev_out);
            SSW_HIP_CHECK(hipGetLastError());
        }
    }
    return SSW_OK;
}
