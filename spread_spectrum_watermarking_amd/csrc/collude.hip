// Strength of a mark before a copy ships (ssw_quality_rgb8, ssw_collude_rgb8): how far is a marked copy from its original, and
// what is left of the marks when several recipients pool their copies?  include/ssw.h states both definitions; every quantity is
// an integer, so nothing here depends on the order of a sum and the results equal the numpy restatement of
// tests/test_collude_cpu.py exactly.  The reference has no counterpart; it is the evaluation its N(0, 1) marks are chosen for
// (src/algorithm.rs:604-606, Cox et al. IV-D); :389-393, its note on what several marks in one image leave of each, is the nearest
// it comes to measuring it.
//
// Both kernels see a frame as w h 3 bytes in a row and give a thread groups of 12 of them (four whole pixels, one load of three
// dwords; no alignment is assumed of anything).  The bytes of a group are kept as six registers of two 16-bit lanes -- the even
// and the odd bytes of each dword -- so that minimum, maximum, sum and difference run on two bytes per instruction; the up to
// nine bytes behind the last whole group take a byte-at-a-time path.
//
// Kernels:
//   quality_kernel   a block owns a piece of 1024 groups (12 KiB): it reads that piece of the original once, keeps its bytes and
//                    lumas in registers and goes over the copies with it -- (1 + n) 3 B/px when one original serves all copies.
//                    Per copy: thread partials (32 bits suffice for a piece) -> wave -> block -> one 64-bit atomic per statistic;
//                    block b starts with copy b % n, so that the grid's atomics spread over the rows of stats.
//   collude_kernel   coalition descriptors as kernel arguments, 32 per launch (like restore.hip's); blockIdx.y is the coalition.
//                    `count` is uniform in a block and selects an instantiation that holds the count values of every byte in
//                    registers; MEDIAN is Batcher's odd-even merge sort network cut down to `count` inputs.  MOSAIC reads the
//                    one member a pixel takes.
#include <algorithm>

#include "rgb_groups.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned CL_BATCH = 32;                 // coalitions per launch
constexpr unsigned CL_MAX = 16;                   // members of a coalition
constexpr unsigned CL_TILE_SHIFT = 5;             // MOSAIC: tiles of 32 x 32 pixels
constexpr unsigned CL_GRID = 2048;                // blocks of a launch, all coalitions together (groups beyond: grid stride)
constexpr unsigned QL_GROUPS = 4;                 // groups of a thread in quality_kernel
constexpr unsigned QL_PIECE = 256 * QL_GROUPS;    // groups of a block
constexpr uint32_t EVEN = 0x00FF00FFu;

struct ColludeBatch { ssw_coalition it[CL_BATCH]; };

typedef unsigned short pk16 __attribute__((ext_vector_type(2)));
__device__ inline uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(pk16, a), __builtin_bit_cast(pk16, b)));
}
__device__ inline uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pk16, a), __builtin_bit_cast(pk16, b)));
}

// twelve bytes at p as six registers of two bytes each: e[k] = bytes 4k, 4k + 2; o[k] = bytes 4k + 1, 4k + 3
struct Planes { uint32_t e[3], o[3]; };
__device__ inline Planes planes(const uint32_t (&v)[3]) {
    Planes r;
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) { r.e[k] = v[k] & EVEN; r.o[k] = (v[k] >> 8) & EVEN; }
    return r;
}
__device__ inline void store12(uint8_t* __restrict__ p, const Planes& r) {
    uint32_t v[3];
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) v[k] = r.e[k] | (r.o[k] << 8);
    __builtin_memcpy(p, v, 12);
}

// ---- quality ---------------------------------------------------------------------------------------------------------------------
struct QStat { uint32_t sse[3], luma, changed, max2; };      // max2: the maximum as two 16-bit lanes

__device__ inline void quality_group(const Planes& b, const uint32_t (&bl)[4], const uint32_t (&cv)[3], QStat& s) {
    const Planes c = planes(cv);
    uint32_t d[3];
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) {
        const uint32_t de = pk_max(c.e[k], b.e[k]) - pk_min(c.e[k], b.e[k]), dod = pk_max(c.o[k], b.o[k]) - pk_min(c.o[k], b.o[k]);
        s.max2 = pk_max(s.max2, pk_max(de, dod));
        s.changed = dot4(pk_min(de, 0x00010001u) | (pk_min(dod, 0x00010001u) << 8), 0x01010101u, s.changed);
        d[k] = de | (dod << 8);                                // |copy - base| of the four bytes of dword k
    }
    // byte i of the group belongs to channel i % 3: dword 0 is R G B R, dword 1 is G B R G, dword 2 is B R G B
    s.sse[0] = dot4(d[0] & 0xFF0000FFu, d[0], dot4(d[1] & 0x00FF0000u, d[1], dot4(d[2] & 0x0000FF00u, d[2], s.sse[0])));
    s.sse[1] = dot4(d[0] & 0x0000FF00u, d[0], dot4(d[1] & 0xFF0000FFu, d[1], dot4(d[2] & 0x00FF0000u, d[2], s.sse[1])));
    s.sse[2] = dot4(d[0] & 0x00FF0000u, d[0], dot4(d[1] & 0x0000FF00u, d[1], dot4(d[2] & 0xFF0000FFu, d[2], s.sse[2])));
    uint32_t cl[4];
    luma4(cv, cl);
#pragma unroll
    for (unsigned q = 0; q < 4; ++q) { const int dl = (int)cl[q] - (int)bl[q]; s.luma += (uint32_t)(dl * dl); }
}

__device__ inline void quality_pixel(const uint8_t* __restrict__ b, const uint8_t* __restrict__ c, QStat& s) {
#pragma unroll
    for (unsigned ch = 0; ch < 3; ++ch) {
        const int d = (int)c[ch] - (int)b[ch];
        const uint32_t a = (uint32_t)(d < 0 ? -d : d);
        s.sse[ch] += a * a;
        s.changed += a ? 1u : 0u;
        s.max2 = pk_max(s.max2, a);
    }
    const int dl = (int)luma(c[0], c[1], c[2]) - (int)luma(b[0], b[1], b[2]);
    s.luma += (uint32_t)(dl * dl);
}

__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint32_t u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

// base_stride: 0 (one original for every copy) or the frame's bytes.  fb: bytes of a frame; groups = fb / 12; the pixels behind
// the last whole group belong to the last block.  stats: [n][6], zero on entry.  grid: (ceil(groups / QL_PIECE), at least 1)
__global__ __launch_bounds__(256) void quality_kernel(const uint8_t* __restrict__ base, size_t base_stride, const uint8_t* __restrict__ copies,
                                                      unsigned n, size_t fb, size_t groups, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t s_part[2][4][6];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    size_t g[QL_GROUPS];
#pragma unroll
    for (unsigned q = 0; q < QL_GROUPS; ++q) g[q] = ((size_t)blockIdx.x * QL_GROUPS + q) * 256 + t;
    const size_t tail_px = (fb - groups * 12) / 3;             // 0 .. 3
    const bool tail = blockIdx.x == gridDim.x - 1 && t < tail_px;
    const size_t tail_off = groups * 12 + (size_t)t * 3;
    Planes bp[QL_GROUPS];
    uint32_t bl[QL_GROUPS][4];
    // blocks start at different copies: at any time the atomics of the grid go to many rows of stats, not to one
    const unsigned first = blockIdx.x % n;
    for (unsigned it = 0; it < n; ++it) {
        const unsigned i = first + it < n ? first + it : first + it - n;
        const uint8_t* __restrict__ b = base + (size_t)i * base_stride;
        const uint8_t* __restrict__ c = copies + (size_t)i * fb;
        if (it == 0 || base_stride) {                           // uniform: the original's piece once when it serves every copy
#pragma unroll
            for (unsigned q = 0; q < QL_GROUPS; ++q)
                if (g[q] < groups) {
                    uint32_t v[3];
                    load12(b + g[q] * 12, v);
                    bp[q] = planes(v);
                    luma4(v, bl[q]);
                }
        }
        QStat s = {{0, 0, 0}, 0, 0, 0};
        uint32_t cv[QL_GROUPS][3];
#pragma unroll
        for (unsigned q = 0; q < QL_GROUPS; ++q) if (g[q] < groups) load12(c + g[q] * 12, cv[q]);
#pragma unroll
        for (unsigned q = 0; q < QL_GROUPS; ++q) if (g[q] < groups) quality_group(bp[q], bl[q], cv[q], s);
        if (tail) quality_pixel(b + tail_off, c + tail_off, s);
        // a thread's sums stay below 2^21, a block's below 2^29
        uint32_t r[6] = {wave_sum(s.sse[0]), wave_sum(s.sse[1]), wave_sum(s.sse[2]), wave_sum(s.luma), wave_sum(s.changed),
                         wave_max(s.max2 & 0xFFFFu) };
        const uint32_t hi = wave_max(s.max2 >> 16);
        r[5] = hi > r[5] ? hi : r[5];
        uint32_t (&part)[4][6] = s_part[it & 1];                // two buffers: one barrier per copy
        if (lane == 0) {
#pragma unroll
            for (unsigned k = 0; k < 6; ++k) part[wave][k] = r[k];
        }
        __syncthreads();
        if (t < 5) {
            const uint32_t v = part[0][t] + part[1][t] + part[2][t] + part[3][t];
            if (v) atomicAdd(&stats[(size_t)i * 6 + t], (unsigned long long)v);
        } else if (t == 5) {
            uint32_t v = part[0][5];
#pragma unroll
            for (unsigned k = 1; k < 4; ++k) v = part[k][5] > v ? part[k][5] : v;
            if (v) atomicMax(&stats[(size_t)i * 6 + 5], (unsigned long long)v);
        }
    }
}

// ---- collude ---------------------------------------------------------------------------------------------------------------------
// Batcher's odd-even merge sort for 16 inputs; a comparator that touches an index >= C is dropped, which is the network run
// on C inputs followed by 16 - C values larger than any byte (such a value never moves down).  Fully unrolled: a[] are registers.
template <unsigned C>
__device__ inline void sort_network(uint32_t (&a)[C]) {
    // stage (p, k), p = 1, 2, 4, 8 and k = p, p / 2, .. 1: the comparators (x, x + k) with x = k % p + 2 k m + i, i < k, inside one
    // block of 2 p; stages with p >= C would merge the sorted inputs with nothing.  Constant trip counts: every condition folds away.
#pragma unroll
    for (unsigned pi = 0; pi < 4; ++pi)
#pragma unroll
        for (unsigned ki = 0; ki < 4; ++ki)
#pragma unroll
            for (unsigned x = 0; x < CL_MAX; ++x) {
                const unsigned p = 1u << pi, k = p >> ki, y = x + k, j0 = k ? k % p : 0;
                if (k && p < C && y < C && x >= j0 && (x - j0) % (2 * k) < k && x / (2 * p) == y / (2 * p)) {
                    const uint32_t lo = pk_min(a[x], a[y]), hi = pk_max(a[x], a[y]);
                    a[x] = lo;
                    a[y] = hi;
                }
            }
}

// one register of two 16-bit lanes, each the value of one byte position in the C members -> that byte pair of the forgery
template <unsigned C>
__device__ inline uint32_t collude_pair(unsigned method, uint32_t (&a)[C]) {
    if (method == SSW_COLLUDE_AVERAGE) {
        uint32_t s = (C / 2) * 0x00010001u;                    // 16 x 255 + 8 fits a lane
#pragma unroll
        for (unsigned j = 0; j < C; ++j) s += a[j];
        return ((s & 0xFFFFu) / C) | (((s >> 16) / C) << 16);
    }
    if (method == SSW_COLLUDE_MEDIAN) {
        sort_network<C>(a);
        return ((a[(C - 1) / 2] + a[C / 2] + 0x00010001u) >> 1) & EVEN;
    }
    uint32_t lo = a[0], hi = a[0];
#pragma unroll
    for (unsigned j = 1; j < C; ++j) { lo = pk_min(lo, a[j]); hi = pk_max(hi, a[j]); }
    if (method == SSW_COLLUDE_MIN) return lo;
    if (method == SSW_COLLUDE_MAX) return hi;
    return ((lo + hi + 0x00010001u) >> 1) & EVEN;             // MINMAX
}

template <unsigned C>
__device__ inline void collude_groups(const ssw_coalition& d, const uint8_t* __restrict__ copies, size_t fb, size_t groups, uint8_t* __restrict__ out) {
    const uint8_t* src[C];
#pragma unroll
    for (unsigned j = 0; j < C; ++j) src[j] = copies + (size_t)d.member[j] * fb;
    const unsigned method = d.method;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        Planes m[C];
#pragma unroll
        for (unsigned j = 0; j < C; ++j) {
            uint32_t v[3];
            load12(src[j] + g * 12, v);
            m[j] = planes(v);
        }
        Planes r;
#pragma unroll
        for (unsigned k = 0; k < 3; ++k) {
            uint32_t a[C];
#pragma unroll
            for (unsigned j = 0; j < C; ++j) a[j] = m[j].e[k];
            r.e[k] = collude_pair<C>(method, a);
#pragma unroll
            for (unsigned j = 0; j < C; ++j) a[j] = m[j].o[k];
            r.o[k] = collude_pair<C>(method, a);
        }
        store12(out + g * 12, r);
    }
}

__device__ inline unsigned mosaic_member(const ssw_coalition& d, uint32_t x, uint32_t y) {
    return d.member[((x >> CL_TILE_SHIFT) + (y >> CL_TILE_SHIFT)) % d.count];
}

// cut-and-paste: every pixel from the one member its tile names.  A group inside one tile of one row is one 12-byte copy.
__device__ inline void mosaic_groups(const ssw_coalition& d, const uint8_t* __restrict__ copies, size_t fb, size_t groups, uint32_t w,
                                     uint8_t* __restrict__ out) {
    const size_t g0 = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    if (g0 >= groups) return;
    // the position of the group's first pixel, carried along the grid stride without a division per group
    uint32_t x = (uint32_t)((g0 * 4) % w), y = (uint32_t)((g0 * 4) / w);
    const uint32_t dx = (uint32_t)((step * 4) % w), dy = (uint32_t)((step * 4) / w);
    for (size_t g = g0; g < groups; g += step) {
        const size_t off = g * 12;
        if (x + 3 < w && (x >> CL_TILE_SHIFT) == ((x + 3) >> CL_TILE_SHIFT)) {
            uint32_t v[3];
            load12(copies + (size_t)mosaic_member(d, x, y) * fb + off, v);
            __builtin_memcpy(out + off, v, 12);
        } else {
            uint32_t px = x, py = y;
            for (unsigned q = 0; q < 4; ++q) {
                while (px >= w) { px -= w; ++py; }
                const uint8_t* __restrict__ s = copies + (size_t)mosaic_member(d, px, py) * fb + off + q * 3;
                out[off + q * 3] = s[0]; out[off + q * 3 + 1] = s[1]; out[off + q * 3 + 2] = s[2];
                ++px;
            }
        }
        x += dx; y += dy;
        if (x >= w) { x -= w; ++y; }
    }
}

// the t-th smallest (from 0) of the members' values at byte `off`, by counting ranks: no array, any count
__device__ inline uint32_t kth_byte(const ssw_coalition& d, const uint8_t* __restrict__ copies, size_t fb, size_t off, unsigned t) {
    for (unsigned j = 0; j < d.count; ++j) {
        const uint32_t v = copies[(size_t)d.member[j] * fb + off];
        unsigned less = 0, leq = 0;
        for (unsigned i = 0; i < d.count; ++i) {
            const uint32_t u = copies[(size_t)d.member[i] * fb + off];
            less += u < v ? 1u : 0u;
            leq += u <= v ? 1u : 0u;
        }
        if (less <= t && t < leq) return v;
    }
    return 0;                                                  // not reached: some value holds every rank
}

// the definition of include/ssw.h for one byte (the bytes behind the last whole group)
__device__ inline uint8_t collude_byte(const ssw_coalition& d, const uint8_t* __restrict__ copies, size_t fb, size_t off, uint32_t w) {
    const unsigned c = d.count;
    switch (d.method) {
        case SSW_COLLUDE_AVERAGE: {
            uint32_t s = c / 2;
            for (unsigned j = 0; j < c; ++j) s += copies[(size_t)d.member[j] * fb + off];
            return (uint8_t)(s / c);
        }
        case SSW_COLLUDE_MEDIAN: return (uint8_t)((kth_byte(d, copies, fb, off, (c - 1) / 2) + kth_byte(d, copies, fb, off, c / 2) + 1) >> 1);
        case SSW_COLLUDE_MIN: return (uint8_t)kth_byte(d, copies, fb, off, 0);
        case SSW_COLLUDE_MAX: return (uint8_t)kth_byte(d, copies, fb, off, c - 1);
        case SSW_COLLUDE_MINMAX: return (uint8_t)((kth_byte(d, copies, fb, off, 0) + kth_byte(d, copies, fb, off, c - 1) + 1) >> 1);
        default: {
            const size_t p = off / 3;
            return copies[(size_t)mosaic_member(d, (uint32_t)(p % w), (uint32_t)(p / w)) * fb + off];
        }
    }
}

// grid: (blocks over the groups, coalitions of the launch).  out: [coalitions of the launch][fb]
__global__ __launch_bounds__(256) void collude_kernel(ColludeBatch b, const uint8_t* __restrict__ copies, size_t fb, size_t groups, uint32_t w,
                                                      uint8_t* __restrict__ out_all) {
    const ssw_coalition& d = b.it[blockIdx.y];
    uint8_t* __restrict__ out = out_all + (size_t)blockIdx.y * fb;
    if (blockIdx.x == 0) {
        const size_t off = groups * 12 + threadIdx.x;
        if (off < fb) out[off] = collude_byte(d, copies, fb, off, w);
    }
    if (d.method == SSW_COLLUDE_MOSAIC) { mosaic_groups(d, copies, fb, groups, w, out); return; }
    switch (d.count) {                                         // uniform
#define SSW_COLLUDE_CASE(C) case C: collude_groups<C>(d, copies, fb, groups, out); break;
        SSW_COLLUDE_CASE(1) SSW_COLLUDE_CASE(2) SSW_COLLUDE_CASE(3) SSW_COLLUDE_CASE(4) SSW_COLLUDE_CASE(5) SSW_COLLUDE_CASE(6)
        SSW_COLLUDE_CASE(7) SSW_COLLUDE_CASE(8) SSW_COLLUDE_CASE(9) SSW_COLLUDE_CASE(10) SSW_COLLUDE_CASE(11) SSW_COLLUDE_CASE(12)
        SSW_COLLUDE_CASE(13) SSW_COLLUDE_CASE(14) SSW_COLLUDE_CASE(15) SSW_COLLUDE_CASE(16)
#undef SSW_COLLUDE_CASE
        default: break;
    }
}

namespace host {
namespace {

// a frame's bytes, or 0 when the frame is empty or too large: w, h <= 2^31 keeps every sum of two 32-bit coordinates of
// mosaic_groups (x + 3, x + dx with x, dx < w) from wrapping, and w h 3 has to fit size_t
size_t frame_bytes(size_t w, size_t h) {
    constexpr size_t SIDE_MAX = (size_t)1 << 31;
    if (w == 0 || h == 0 || w > SIDE_MAX || h > SIDE_MAX) return 0;
    if (w > SIZE_MAX / 3 / h) return 0;
    return w * h * 3;
}

}  // namespace
}  // namespace host
}  // namespace ssw

extern "C" int ssw_quality_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h,
                                uint64_t* dev_stats) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_copies || !dev_stats || (n_base != 1 && n_base != n) || n > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    const size_t fb = frame_bytes(w, h);
    if (!fb) return SSW_ERR_BAD_DIMS;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const size_t groups = fb / 12, pieces = std::max<size_t>(1, (groups + ssw::QL_PIECE - 1) / ssw::QL_PIECE);
    if (pieces > 0x7FFFFFFFull) return SSW_ERR_BAD_DIMS;
    StageTimer t(ctx, SSW_STAGE_CONVERT, st, (double)(n_base + n) * (double)fb + 48.0 * (double)n);
    SSW_HIP_CHECK(hipMemsetAsync(dev_stats, 0, n * 6 * sizeof(uint64_t), st));
    ssw::quality_kernel<<<(unsigned)pieces, 256, 0, st>>>(dev_base, n_base == 1 ? 0 : fb, dev_copies, (unsigned)n, fb, groups,
                                                          reinterpret_cast<unsigned long long*>(dev_stats));
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}

extern "C" int ssw_collude_rgb8(ssw_ctx* ctx, const uint8_t* dev_copies, size_t n_copies, size_t w, size_t h, const ssw_coalition* coalitions,
                                size_t n_coalitions, uint8_t* dev_out) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n_coalitions == 0) return SSW_OK;
    if (!dev_copies || !coalitions || !dev_out) return SSW_ERR_BAD_ARG;
    double bytes = 0.0;
    const size_t fb = frame_bytes(w, h);
    for (size_t i = 0; i < n_coalitions; ++i) {
        const ssw_coalition& c = coalitions[i];
        if (c.method > SSW_COLLUDE_MOSAIC || c.count < 1 || c.count > ssw::CL_MAX) return SSW_ERR_BAD_ARG;
        for (unsigned j = 0; j < c.count; ++j) if (c.member[j] >= n_copies) return SSW_ERR_BAD_ARG;
        bytes += (double)(c.count + 1) * (double)fb;
    }
    if (!fb) return SSW_ERR_BAD_DIMS;
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    const size_t groups = fb / 12;
    StageTimer t(ctx, SSW_STAGE_CONVERT, st, bytes);
    for (size_t i0 = 0; i0 < n_coalitions; i0 += ssw::CL_BATCH) {
        const unsigned m = (unsigned)std::min<size_t>(ssw::CL_BATCH, n_coalitions - i0);
        ssw::ColludeBatch b{};
        std::copy(coalitions + i0, coalitions + i0 + m, b.it);
        const unsigned bx = (unsigned)std::min<size_t>(std::max<size_t>(1, (groups + 255) / 256), std::max(1u, ssw::CL_GRID / m));
        ssw::collude_kernel<<<dim3(bx, m), 256, 0, st>>>(b, dev_copies, fb, groups, (uint32_t)w, dev_out + i0 * fb);
        SSW_HIP_CHECK(hipGetLastError());
    }
    return SSW_OK;
}
