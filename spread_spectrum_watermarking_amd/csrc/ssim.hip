// A perceptual score beside PSNR (ssw_ssim_rgb8): the structural similarity of marked copies and their original, on the luma, in
// 8 x 8 windows at a stride of 4 pixels.  include/ssw.h states the definition; the sums are integers, every window takes one
// correctly rounded f64 division and becomes a fixed-point integer, and those are summed as integers -- nothing depends on the
// order of a sum and the results equal the numpy restatement of tests/test_ssim_cpu.py exactly.  The reference has no counterpart.
//
// ssim_kernel   a block owns SS_WX x SS_WY windows and reads the SS_CX x SS_CY cells of 4 x 4 pixels under them -- one more
//               column and row of cells than windows: windows straddle blocks and the cells they share are read by both, 8 %
//               more bytes than the frame holds.  A thread takes SS_SLOTS cells, one per four cell rows, so that a wave reads
//               64 consecutive groups of twelve bytes of one pixel row.  It keeps the packed lumas of its cells of the
//               original and their sums in registers and goes over the copies with them -- (1 + n) 3 B/px when one original
//               serves all copies.  Per copy: cell sums -> LDS, barrier, a thread adds 2 x 2 cells per window and evaluates
//               it, thread partials -> wave -> block -> one 64-bit atomicAdd and one atomicMin; block b starts with copy
//               b % n, so that the grid's atomics spread over the rows of stats.
#include <algorithm>

#include "rgb_groups.hpp"
#include "ssw_host.hpp"

namespace ssw {

constexpr unsigned SS_CX = 64, SS_CY = 16;                 // cells a block reads: 256 x 64 pixels
constexpr unsigned SS_WX = SS_CX - 1, SS_WY = SS_CY - 1;   // windows a block owns: its stride is SSW_SSIM_TILE_W x _H pixels
constexpr unsigned SS_SLOTS = SS_CX * SS_CY / 256;         // cells, and windows, of a thread
static_assert(SS_WX * 4 == SSW_SSIM_TILE_W && SS_WY * 4 == SSW_SSIM_TILE_H, "include/ssw.h states the tile");
static_assert(SS_CX == 64 && SS_SLOTS * 256 == SS_CX * SS_CY, "a wave is one row of cells");

// one window from its four sums (include/ssw.h): 32-bit integers up to the two products, which are exact as products of doubles
// and rounded once; one IEEE division
__device__ inline int32_t ssim_window(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12) {
    const int32_t vars = (int32_t)(64u * ss - s1 * s1 - s2 * s2), covar = (int32_t)(64u * s12 - s1 * s2);
    const int32_t n1 = (int32_t)(2u * s1 * s2 + 416u), n2 = 2 * covar + 235963;
    const int32_t d1 = (int32_t)(s1 * s1 + s2 * s2 + 416u), d2 = vars + 235963;
    const double q = ((double)n1 * (double)n2) / ((double)d1 * (double)d2);
    return (int32_t)floor(q * (double)SSW_SSIM_ONE + 0.5);
}

__device__ inline long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}

// stats: [n][2]
__global__ __launch_bounds__(256) void ssim_init_kernel(unsigned long long* __restrict__ stats, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { stats[2 * i] = 0; stats[2 * i + 1] = ~0ull; }
}

// base_stride: 0 (one original for every copy) or the frame's bytes fb.  ncx, ncy: whole cells of a frame (>= 2 each); the
// windows are (ncx - 1) x (ncy - 1).  stats: [n][2], initialised.  map: [n][ncy - 1][ncx - 1] or null.
// grid: tiles_x * ceil((ncy - 1) / SS_WY) with tiles_x = ceil((ncx - 1) / SS_WX)
__global__ __launch_bounds__(256) void ssim_kernel(const uint8_t* __restrict__ base, size_t base_stride, const uint8_t* __restrict__ copies,
                                                   unsigned n, size_t fb, size_t row, uint32_t ncx, uint32_t ncy, uint32_t tiles_x,
                                                   unsigned long long* __restrict__ stats, int32_t* __restrict__ map) {
    __shared__ uint4 s_cell[SS_CY * SS_CX];                    // s1, s2, ss, s12 of a cell
    __shared__ long long s_sum[4];
    __shared__ unsigned long long s_min[4];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const uint32_t nx = ncx - 1, ny = ncy - 1;
    // slot q: the cell (lane, 4 q + wave) of the block, and the window whose upper left cell that is
    const uint32_t gx = tile_x * SS_WX + lane;
    size_t off[SS_SLOTS];
    uint32_t index[SS_SLOTS];
    bool cell[SS_SLOTS], window[SS_SLOTS];
#pragma unroll
    for (unsigned q = 0; q < SS_SLOTS; ++q) {
        const uint32_t cy = 4 * q + wave, gy = tile_y * SS_WY + cy;
        cell[q] = gx < ncx && gy < ncy;                         // whole cells only: every byte of a cell is inside the frame
        window[q] = lane < SS_WX && cy < SS_WY && gx < nx && gy < ny;
        off[q] = (size_t)gy * 4 * row + (size_t)gx * 12;
        index[q] = gy * nx + gx;                                // below 2^32 where window[q] holds
    }
    uint32_t al[SS_SLOTS][4], sa[SS_SLOTS], saa[SS_SLOTS];      // the original's cells: four lumas per dword, a row each
    const size_t windows = (size_t)nx * ny;
    // blocks start at different copies: at any time the atomics of the grid go to many rows of stats, not to one
    const unsigned first = blockIdx.x % n;
    for (unsigned it = 0; it < n; ++it) {
        const unsigned i = first + it < n ? first + it : first + it - n;
        const uint8_t* __restrict__ b = base + (size_t)i * base_stride;
        const uint8_t* __restrict__ c = copies + (size_t)i * fb;
        if (it == 0 || base_stride) {                           // uniform: the original's cells once when it serves every copy
#pragma unroll
            for (unsigned q = 0; q < SS_SLOTS; ++q) {
                sa[q] = saa[q] = 0;
                if (cell[q]) {
#pragma unroll
                    for (unsigned r = 0; r < 4; ++r) {
                        uint32_t v[3], l[4];
                        load12(b + off[q] + r * row, v);
                        luma4(v, l);
                        al[q][r] = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
                        sa[q] = dot4(al[q][r], 0x01010101u, sa[q]);
                        saa[q] = dot4(al[q][r], al[q][r], saa[q]);
                    }
                }
            }
        }
        uint32_t cv[SS_SLOTS][4][3];
#pragma unroll
        for (unsigned q = 0; q < SS_SLOTS; ++q)
            if (cell[q]) {
#pragma unroll
                for (unsigned r = 0; r < 4; ++r) load12(c + off[q] + r * row, cv[q][r]);
            }
#pragma unroll
        for (unsigned q = 0; q < SS_SLOTS; ++q)
            if (cell[q]) {
                uint32_t sb = 0, sbb = 0, sab = 0;
#pragma unroll
                for (unsigned r = 0; r < 4; ++r) {
                    uint32_t l[4];
                    luma4(cv[q][r], l);
                    const uint32_t bl = l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24);
                    sb = dot4(bl, 0x01010101u, sb);
                    sbb = dot4(bl, bl, sbb);
                    sab = dot4(al[q][r], bl, sab);
                }
                s_cell[(4 * q + wave) * SS_CX + lane] = make_uint4(sa[q], sb, saa[q] + sbb, sab);
            }
        __syncthreads();
        long long sum = 0;
        unsigned long long worst = ~0ull;
#pragma unroll
        for (unsigned q = 0; q < SS_SLOTS; ++q)
            if (window[q]) {                                    // its four cells are inside the block and inside the frame
                const unsigned k = (4 * q + wave) * SS_CX + lane;
                const uint4 c00 = s_cell[k], c01 = s_cell[k + 1], c10 = s_cell[k + SS_CX], c11 = s_cell[k + SS_CX + 1];
                const int32_t v = ssim_window(c00.x + c01.x + c10.x + c11.x, c00.y + c01.y + c10.y + c11.y, c00.z + c01.z + c10.z + c11.z,
                                              c00.w + c01.w + c10.w + c11.w);
                sum += v;
                const unsigned long long key = ((unsigned long long)((uint32_t)v + (uint32_t)SSW_SSIM_ONE) << 32) | index[q];
                worst = key < worst ? key : worst;
                if (map) map[(size_t)i * windows + index[q]] = v;
            }
        sum = wave_sum64(sum);
        worst = wave_min64(worst);
        if (lane == 0) { s_sum[wave] = sum; s_min[wave] = worst; }
        __syncthreads();                                        // also: every window of this copy is read before the next one's cells
        if (t == 0) {
            unsigned long long m = s_min[0];
#pragma unroll
            for (unsigned k = 1; k < 4; ++k) m = s_min[k] < m ? s_min[k] : m;
            atomicAdd(&stats[(size_t)i * 2], (unsigned long long)(s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]));   // two's complement
            atomicMin(&stats[(size_t)i * 2 + 1], m);
        }
    }
}

}  // namespace ssw

extern "C" int ssw_ssim_rgb8(ssw_ctx* ctx, const uint8_t* dev_base, size_t n_base, const uint8_t* dev_copies, size_t n, size_t w, size_t h,
                             uint64_t* dev_stats, int32_t* dev_map) {
    using namespace ssw::host;
    if (!ctx) return SSW_ERR_BAD_ARG;
    if (n == 0) return SSW_OK;
    if (!dev_base || !dev_copies || !dev_stats || (n_base != 1 && n_base != n) || n > 0xFFFFFFFFull) return SSW_ERR_BAD_ARG;
    constexpr size_t SIDE_MAX = (size_t)1 << 31;
    if (w == 0 || h == 0 || w > SIDE_MAX || h > SIDE_MAX || w > SIZE_MAX / 3 / h) return SSW_ERR_BAD_DIMS;
    if (w < SSW_SSIM_MIN_SIDE || h < SSW_SSIM_MIN_SIDE) return SSW_ERR_BAD_ARG;
    const size_t ncx = w / 4, ncy = h / 4, nx = ncx - 1, ny = ncy - 1, fb = w * h * 3;
    if (nx * ny > 0xFFFFFFFFull) return SSW_ERR_BAD_DIMS;        // a window's index is 32 bits of stats[1]
    const size_t tiles_x = (nx + ssw::SS_WX - 1) / ssw::SS_WX, tiles = tiles_x * ((ny + ssw::SS_WY - 1) / ssw::SS_WY);   // below 2^23
    CtxGuard g(ctx);
    hipStream_t st = ctx->stream;
    StageTimer t(ctx, SSW_STAGE_CONVERT, st, (double)(n_base + n) * (double)fb + 16.0 * (double)n + (dev_map ? 4.0 * (double)(nx * ny) * (double)n : 0.0));
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(dev_stats);
    ssw::ssim_init_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(stats, n);
    SSW_HIP_CHECK(hipGetLastError());
    ssw::ssim_kernel<<<(unsigned)tiles, 256, 0, st>>>(dev_base, n_base == 1 ? 0 : fb, dev_copies, (unsigned)n, fb, w * 3, (uint32_t)ncx, (uint32_t)ncy,
                                                      (uint32_t)tiles_x, stats, dev_map);
    SSW_HIP_CHECK(hipGetLastError());
    return SSW_OK;
}
